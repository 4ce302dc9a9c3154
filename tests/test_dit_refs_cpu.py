"""The references, bounds and guard bands of tests/dit_refs.py must be right and must bite (no GPU needed).

(a) each new reference equals the restatement the existing kernel tests compute, on the cases those tests use;
(b) for EVERY GRID_* case that tests/test_dit_kernel_edges_gpu.py runs, a correct bf16 stand-in with another summation order
    passes the bound the GPU test applies (frac_exact included);
(c) each subtly wrong stand-in (a mutant) fails that bound on at least one grid case of its family, and a store outside the
    logical output is found by assert_guard_intact while a clean store leaves it passing."""
import pytest
import torch
import torch.nn.functional as F

import dit_refs as R
from oracle import dit_oracle as O

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ (a) references
@pytest.mark.parametrize("M,N,K,epi,seeds", [(1000, 256, 256, 0, (1, 2)), (512, 256, 256, 1, (5, 6)), (640, 256, 512, 2, (7, 8))])
def test_gemm_ref_equals_the_fp32_restatement(M, N, K, epi, seeds):
    """test_gemm_plain / _gelu_epilogue / _gate_residual_epilogue_inplace form lin from an fp32 product; the fp64 product rounds to
    another bf16 value only where the fp32 sum (error ~ sqrt(K) 2^-24 of the terms) sits on a rounding boundary: a share below
    1e-3 of the elements, one ulp each (more only where the terms cancel to nearly zero: the comparator's rms allowance)."""
    a, w = R.rnd((M, K), seed=seeds[0]), R.rnd((N, K), 0.1 if epi < 2 else 0.05, seed=seeds[1])
    x, gate = R.rnd((M, N), seed=9), R.rnd((1, N), 0.5, seed=10)
    lin = (a.float() @ w.float().t()).to(BF)
    old = lin if epi == 0 else (F.gelu(lin) if epi == 1 else x + gate * lin)
    new, mag = R.gemm_ref(a, w, epi, gate, x, M)
    new_lin, _ = R.gemm_ref(a, w, 0)
    ok, msg = R.ulp_diff_ok(new_lin, lin, max_ulp=1, frac_exact=0.999)
    assert ok, msg
    same = new_lin == lin
    assert torch.equal(new[same], old[same]), "the op chain after the product is the existing tests', bit for bit"
    if epi == 2:
        assert torch.equal(mag, torch.maximum(x.abs(), (gate * R.gemm_ref(a, w, 0)[0]).abs()))


def test_gemm_ref_takes_the_gate_of_each_rows_clip():
    a, w = R.rnd((10, 64), seed=1), R.rnd((128, 64), 0.1, seed=2)
    x, gate = R.rnd((10, 128), seed=3), R.rnd((3, 128), seed=4)
    ref, _ = R.gemm_ref(a, w, 2, gate, x, 4)
    lin, _ = R.gemm_ref(a, w, 0)
    for r in range(10):
        assert torch.equal(ref[r], x[r] + gate[r // 4] * lin[r])


@pytest.mark.parametrize("heads,Sq,Sk", [(2, 128, 128), (1, 513, 77)])
def test_attention_ref_equals_attn_ref_at_the_default_scale(heads, Sq, Sk):
    q, k, v = (R.rnd((1, S, heads * 128), seed=29 + i) for i, S in enumerate((Sq, Sk, Sk)))
    old = R._attn_ref(q, k, v, heads)
    old_mag = R._attn_ref.mag
    new, mag = R.attention_ref(q, k, v, heads)
    assert R.rel_l2(old, new) < 2e-6 and R.rel_l2(old_mag, mag) < 2e-6          # fp32 against fp64
    assert R._attn_ref.mag is mag
    assert (new.to(BF) != old.to(BF)).float().mean().item() < 1e-3


@pytest.mark.parametrize("heads,T,H,W", [(2, 2, 8, 8), (4, 1, 6, 10), (32, 1, 4, 4)])
def test_qk_norm_rope_ref_equals_the_oracle_restatement(heads, T, H, W):
    """test_qk_norm_rope_matches_oracle's reference; and two clips with an offset == each clip alone on the offset table rows."""
    S, D = T * H * W, heads * 128
    qkv = R.rnd((S, 3 * D), 1.5, seed=26)
    wq = 1 + 0.1 * R.rnd((128,), seed=27)
    oc, os_ = O.rope_cos_sin(O.rope_angles(T, H, W, 128, torch.arange(512, dtype=torch.float32).to(BF), BF), BF)
    old = O.apply_rope(O.rms_norm(qkv[:, :D].reshape(S, 1, heads, 128), wq), oc, os_).reshape(S, D)
    assert torch.equal(R.qk_norm_rope_ref(qkv[:, :D], wq, oc, os_, heads), old)
    tpb, pos = S // 2 - 3, 3
    two = R.qk_norm_rope_ref(qkv[:2 * tpb, :D], wq, oc, os_, heads, tpb, pos)
    for b in range(2):
        x = qkv[b * tpb:(b + 1) * tpb, :D].reshape(tpb, 1, heads, 128)
        one = O.apply_rope(O.rms_norm(x, wq), oc[pos:pos + tpb], os_[pos:pos + tpb]).reshape(tpb, D)
        assert torch.equal(two[b * tpb:(b + 1) * tpb], one)
    assert torch.equal(R.qk_norm_rope_ref(qkv[:, :D], wq, None, None, heads), O.rms_norm(qkv[:, :D].reshape(S, heads, 128), wq).reshape(S, D))


@pytest.mark.parametrize("rows,D,with_add", [(37, 256, False), (300, 4096, True), (7, 2048, True)])
def test_ln_modulate_ref_equals_the_existing_restatement(rows, D, with_add):
    x = R.rnd((rows, D), 2.0, seed=17)
    shift, scale = R.rnd((1, D), 0.7, seed=18), R.rnd((1, D), 0.7, seed=19)
    add = R.rnd((1, D), 0.5, seed=21) if with_add else None
    x2 = x + add if with_add else x
    old = O.modulate(F.layer_norm(x2.unsqueeze(1), (D,), eps=1e-6), shift, scale).squeeze(1)
    xa, h = R.ln_modulate_ref(x, shift, scale, add)
    assert torch.equal(xa, x2) and torch.equal(h, old)
    # per-clip rows: == each clip alone
    s3, c3 = R.rnd((3, D), 0.7, seed=1), R.rnd((3, D), 0.7, seed=2)
    rpb = -(-rows // 3)
    _, h3 = R.ln_modulate_ref(x, s3, c3, None, rpb)
    for b in range(3):
        sl = slice(b * rpb, min((b + 1) * rpb, rows))
        assert torch.equal(h3[sl], R.ln_modulate_ref(x[sl], s3[b:b + 1], c3[b:b + 1])[1])


def test_gemv_ref_equals_the_existing_restatement():
    x, w = R.rnd((5, 1, 256), seed=11), R.rnd((5, 384, 256), 0.1, seed=12)
    add, mul = R.rnd((1, 1, 384), seed=13), R.rnd((5, 1, 384), seed=14)
    lin = torch.einsum("gbk,gnk->gbn", F.silu(x).float(), w.float()).to(BF)
    old = mul * (lin + add)
    new = R.gemv_ref(x, w, add, mul, 1)
    assert (new != old).float().mean().item() < 2e-3
    ok, msg = R.ulp_diff_ok(new, old, max_ulp=1, frac_exact=0.998, atol_rel=0.0)
    assert ok, msg


# ------------------------------------------------------------------------------------------------ guard bands
def test_guarded_window_geometry_and_sentinel():
    buf, v = R.guarded(5, 24, 32, 2, "cpu", batches=3, batch_gap=16)
    assert v.shape == (3, 5, 24) and v.stride() == (5 * 32 + 16, 32, 1) and v.storage_offset() == 64
    assert buf.numel() == 4 * 32 + 3 * (5 * 32 + 16) and R.is_sentinel(buf).all() and torch.isnan(buf.float()).all()
    R.assert_guard_intact(buf, v)
    buf2, v2 = R.guarded(7, 8, 8, 1, "cpu")
    assert v2.shape == (7, 8) and v2.is_contiguous()
    bu8, vu8 = R.guarded(4, 6, 6, 1, "cpu", dtype=torch.uint8)
    vu8.fill_(3)
    R.assert_guard_intact(bu8, vu8)
    bu8[2] = 0
    with pytest.raises(AssertionError):
        R.assert_guard_intact(bu8, vu8)


STORE_MUTANTS = ["row_past_M", "cols_past_N", "batch_gap"]


@pytest.mark.parametrize("mutant", STORE_MUTANTS)
def test_store_outside_the_window_is_caught(mutant):
    """One row stored past M, 8 columns past N, a store into the batch gap: found by assert_guard_intact; a clean store passes."""
    for batches, rows, cols, ld, gap in ((2, 129, 256, 320, 128), (3, 1, 128, 192, 64)):
        val = R.rnd((batches, rows, cols), seed=7)
        buf, v = R.guarded(rows, cols, ld, 2, "cpu", batches=batches, batch_gap=gap)
        R.store_standin(buf, v, val)
        R.assert_guard_intact(buf, v)
        assert torch.equal(v, val)
        buf, v = R.guarded(rows, cols, ld, 2, "cpu", batches=batches, batch_gap=gap)
        R.store_standin(buf, v, val, mutant)
        assert torch.equal(v, val), "the window itself holds the right values: only the guard can see this"
        with pytest.raises(AssertionError, match="outside the window"):
            R.assert_guard_intact(buf, v)


# ------------------------------------------------------------------------------------------------ GEMM
def _gemm_tile_rows(c):
    return {"tile": R.GEMM_TILE_ROWS.get(c.tile, 128), "splitk": 128, "tall0": 256, "tall1": 128, "batched": 256}[c.path]


def _gemm_case(c, mutant=None):
    a, w, gate, res = R.gemm_inputs(c)
    ldc, ldr = c.N + 64, c.N + 128
    if mutant == "res_ldc":                            # the residual where the GPU test puts it: a window with its own row stride
        _, win = R.guarded(c.M, c.N, ldr, 2, "cpu")
        win.copy_(res)
        res = win
    ref, mag = R.gemm_ref(a, w, c.epi, gate, res, c.rpb)
    out = R.gemm_standin(a, w, c.epi, gate, res, c.rpb, slices=max(c.splits, 2 + c.seed % 15), tile_rows=_gemm_tile_rows(c),
                         mutant=mutant, ldc=ldc)
    ok, msg = R.ulp_diff_ok(out, ref, mag=mag, **R.GEMM_BOUND[c.epi])
    return ok, f"{msg}  {R.figures(out, ref, mag)}"


@pytest.mark.parametrize("c", R.GRID_GEMM, ids=R.gemm_id)
def test_gemm_standin_passes(c):
    ok, msg = _gemm_case(c)
    print(f"dit-kernel-edge stand-in gemm {R.gemm_id(c)}: {msg}")
    assert ok, msg


@pytest.mark.parametrize("mutant", ["gate_clip_pm1", "rpb_ignored", "res_ldc"])
def test_gemm_mutants_are_caught(mutant):
    caught = []
    for c in R.GRID_GEMM:
        if c.epi != R.EPI_GATE_RES or c.M > 600 or c.N > 512 or (mutant == "res_ldc" and not c.strided):
            continue
        ok, msg = _gemm_case(c, mutant)
        if not ok:
            caught.append(R.gemm_id(c))
    print(f"gemm mutant {mutant}: caught by {len(caught)} cases, e.g. {caught[:3]}")
    assert caught, mutant


# ------------------------------------------------------------------------------------------------ attention
def _attn_case(c, mutant=None):
    q, k, v = R.attn_views(R.attn_packed(c), c)
    out = R.attention_standin(q, k, v, c.H, c.scale, c.ns, mutant)
    ref, _ = R.attention_ref(q, k, v, c.H, c.scale)
    R._attn_check(out, ref, R.attn_id(c))
    return out


@pytest.mark.parametrize("c", R.GRID_ATTN, ids=R.attn_id)
def test_attention_standin_passes(c):
    out = _attn_case(c)
    if c.Sk == 1:
        v = R.attn_views(R.attn_packed(c), c)[2]
        assert torch.equal(out, v.expand(-1, c.Sq, -1)), "one key: the output is V[0] bit for bit"


@pytest.mark.parametrize("mutant", ["kv_clip0", "scale_default", "drop_last_key", "combine_requested"])
def test_attention_mutants_are_caught(mutant):
    caught = []
    for c in R.GRID_ATTN:
        try:
            _attn_case(c, mutant)
        except AssertionError:
            caught.append(R.attn_id(c))
    print(f"attention mutant {mutant}: caught by {len(caught)} cases, e.g. {caught[:3]}")
    assert caught, mutant
    if mutant == "combine_requested":
        assert all("Sk77" in i for i in caught), "only where the launcher runs fewer chunks than requested"


def test_attn_splits_follow_the_launcher():
    assert R.attn_splits(77, 4) == (64, 2) and R.attn_splits(641, 4) == (192, 4) and R.attn_splits(300, 2) == (192, 2)
    assert R.attn_splits(4100, 4) == (1088, 4) and R.attn_splits(65, 1) == (65, 1)


# ------------------------------------------------------------------------------------------------ q/k RMSNorm + RoPE
def _rope_case(c, mutant=None, order="torch"):
    qkv, wq, wk, cos, sin = R.rope_inputs(c)
    D = c.heads * 128
    cs = (cos, sin) if c.rope else (None, None)
    res = []
    for idx, wn, tag in ((0, wq, "q"), (1, wk, "k")):
        if tag not in c.which:
            continue
        x = qkv[:, idx * D:(idx + 1) * D]
        ref = R.qk_norm_rope_ref(x, wn, *cs, c.heads, c.tpb, c.pos)
        out = R.qk_norm_rope_standin(x, wn, *cs, c.heads, c.tpb, c.pos, mutant, order)
        ok, msg = R.ulp_diff_ok(out, ref, **R.ROPE_BOUND)
        res.append((ok, f"{tag}: {msg}  {R.figures(out, ref)}"))
    return all(r[0] for r in res), " | ".join(r[1] for r in res)


@pytest.mark.parametrize("order", ["torch", "kernel"])
@pytest.mark.parametrize("c", R.GRID_ROPE, ids=R.rope_id)
def test_qk_norm_rope_standin_passes(c, order):
    """Two correct fp32 stand-ins, the mean square summed as torch does and as the kernel does: both inside the bound."""
    ok, msg = _rope_case(c, order=order)
    print(f"dit-kernel-edge stand-in qk_norm_rope {R.rope_id(c)} ({order} order): {msg}")
    assert ok, msg


def test_qk_norm_rope_exact_inputs_leave_one_correct_answer():
    """With the multiples of 1/4 of an `exact` case every summation order gives the same mean square: the kernel-order stand-in
    equals the oracle's ops bit for bit, while the normalised values still exercise the bf16 roundings (few are exact)."""
    c = next(c for c in R.GRID_ROPE if c.exact and c.clips * c.tpb < 1000)
    qkv, wq, wk, cos, sin = R.rope_inputs(c)
    x = qkv[:, :c.heads * 128]
    ref = R.qk_norm_rope_ref(x, wq, cos, sin, c.heads, c.tpb, c.pos)
    assert torch.equal(R.qk_norm_rope_standin(x, wq, cos, sin, c.heads, c.tpb, c.pos, order="kernel"), ref)
    n32 = x.float().reshape(-1, c.heads, 128)
    n32 = n32 * torch.rsqrt(n32.pow(2).mean(-1, keepdim=True) + 1e-6) * wq.float()
    assert (n32.to(BF).float() != n32).float().mean().item() > 0.9


@pytest.mark.parametrize("mutant", ["tok_row", "pos_dropped", "pos_off1"])
def test_qk_norm_rope_mutants_are_caught(mutant):
    caught = [R.rope_id(c) for c in R.GRID_ROPE if c.clips * c.tpb < 1000 and not _rope_case(c, mutant)[0]]
    print(f"qk_norm_rope mutant {mutant}: caught by {len(caught)} cases, e.g. {caught[:3]}")
    assert caught, mutant


# ------------------------------------------------------------------------------------------------ LayerNorm + modulate
def _ln_case(c, mutant=None, order="torch"):
    x, shift, scale, add = R.ln_inputs(c)
    xr, href = R.ln_modulate_ref(x, shift, scale, add, R.ln_rpb(c))
    xs, h = R.ln_modulate_standin(x, shift, scale, add, R.ln_rpb(c), mutant, order)
    ok, msg = R.ulp_diff_ok(h, href, **R.LN_BOUND)
    return ok and torch.equal(xs, xr), f"{msg}  x {'==' if torch.equal(xs, xr) else '!='}  {R.figures(h, href)}"


@pytest.mark.parametrize("order", ["torch", "kernel"])
@pytest.mark.parametrize("c", R.GRID_LN, ids=R.ln_id)
def test_ln_modulate_standin_passes(c, order):
    ok, msg = _ln_case(c, order=order)
    print(f"dit-kernel-edge stand-in ln_modulate {R.ln_id(c)} ({order} order): {msg}")
    assert ok, msg


@pytest.mark.parametrize("mutant", ["clip_pm1", "rpb_ignored"])
def test_ln_modulate_mutants_are_caught(mutant):
    caught = [R.ln_id(c) for c in R.GRID_LN if not _ln_case(c, mutant)[0]]
    print(f"ln_modulate mutant {mutant}: caught by {len(caught)} cases, e.g. {caught[:3]}")
    assert caught, mutant


# ------------------------------------------------------------------------------------------------ GEMV, RMSNorm
@pytest.mark.parametrize("c", R.GRID_GEMV, ids=R.gemv_id)
def test_gemv_standin_passes(c):
    x, w, add, mul = R.gemv_inputs(c)
    ref, out = R.gemv_ref(x, w, add, mul, c.act), R.gemv_standin(x, w, add, mul, c.act)
    ok, msg = R.ulp_diff_ok(out, ref, **R.gemv_bound(c))
    print(f"dit-kernel-edge stand-in gemv {R.gemv_id(c)}: {msg}  {R.figures(out, ref)}")
    assert ok, msg
    if c.G > 1 and c.Gx == 1:                          # a shared x with per-group weights: group 0's weights everywhere is caught
        bad = R.gemv_standin(x, w[:1].expand_as(w), add, mul, c.act)
        assert not R.ulp_diff_ok(bad, ref, **R.gemv_bound(c))[0]


@pytest.mark.parametrize("rows,D,seed", R.GRID_RMSNORM)
def test_rmsnorm_standin_passes(rows, D, seed):
    x, w = R.rnd((rows, D), seed=seed), R.rnd((D,), seed=seed + 1)
    ref, out = O.rms_norm(x, w), R.rmsnorm_standin(x, w)
    ok, msg = R.ulp_diff_ok(out, ref, **R.RMSNORM_BOUND)
    print(f"dit-kernel-edge stand-in rmsnorm {rows}x{D}: {msg}  {R.figures(out, ref)}")
    assert ok, msg
    assert not R.ulp_diff_ok(R.rmsnorm_standin(x, torch.roll(w, 1)), ref, **R.RMSNORM_BOUND)[0]
