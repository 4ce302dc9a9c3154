"""Per-kernel parity of libdrn.so (through the C ABI) against the CPU oracle / fp32 torch references.

Bit-exact where the op is an index map or a restatement of unfused fp32 ops (patchify, unpatchify, EDM step,
CFG, uint8 post-process); for reductions / MFMA products the result must equal the reference rounded to bf16 up to
accumulation-order flips: <= 1 bf16 ulp everywhere, and rel-L2 against the fp32 value <= the stated tolerance.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from dit_refs import ATTN_REL_L2, _attn_check, _attn_ref, ulp_diff_ok          # comparators shared with the edge-geometry tests
from oracle import dit_oracle as O

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(params=["32x32x16", "16x16x32"])
def att_body(request, pkg):
    """Every attention test runs on both kernel bodies (csrc/attention.hip, csrc/attention16.hip)."""
    lib = pkg.native.load_library()
    lib.drn_attention_force_shape16(1 if request.param == "16x16x32" else 0)
    yield request.param
    lib.drn_attention_force_shape16(-1)


def rnd(shape, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF).to(dev)


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 192), (1000, 256, 256), (2304, 1024, 512), (77, 128, 128)])
def test_gemm_plain(pkg, gpu, M, N, K):
    a, w = rnd((M, K), gpu, seed=1), rnd((N, K), gpu, 0.1, seed=2)
    out = pkg.native.gemm(a, w)
    ref32 = a.float() @ w.float().t()
    ok, msg = ulp_diff_ok(out, ref32.to(BF))
    assert ok, msg
    assert rel_l2(out, ref32) < 3e-3          # bf16 output rounding alone is ~1.1e-3 rms


def test_gemm_identity_asymmetric(pkg, gpu):
    """A = I with an asymmetric W catches a transposed fragment or C map (cdna guide, section 3)."""
    K = N = 128
    a = torch.eye(128, K, dtype=BF, device=gpu)
    w = (torch.arange(N * K, device=gpu).reshape(N, K) % 251).to(BF)
    out = pkg.native.gemm(a, w)
    assert torch.equal(out, w.t().contiguous())


def test_gemm_strided_views_and_tail(pkg, gpu):
    M, D = 300, 256
    big = rnd((M, 3 * D), gpu, seed=3)
    w = rnd((128, D), gpu, 0.1, seed=4)
    out = pkg.native.gemm(big[:, D:2 * D], w)
    ref = (big[:, D:2 * D].float() @ w.float().t()).to(BF)
    ok, msg = ulp_diff_ok(out, ref)
    assert ok, msg


def test_gemm_gelu_epilogue(pkg, gpu):
    M, N, K = 512, 256, 256
    a, w = rnd((M, K), gpu, seed=5), rnd((N, K), gpu, 0.1, seed=6)
    out = pkg.native.gemm(a, w, epilogue=pkg.native.EPI_GELU)
    lin = (a.float() @ w.float().t()).to(BF)
    ref = F.gelu(lin.cpu()).to(gpu)            # torch CPU bf16 erf-GELU: what the reference runs
    ok, msg = ulp_diff_ok(out, ref, max_ulp=2, frac_exact=0.97)
    assert ok, msg


def test_gemm_gate_residual_epilogue_inplace(pkg, gpu):
    M, N, K = 640, 256, 512
    a, w = rnd((M, K), gpu, seed=7), rnd((N, K), gpu, 0.05, seed=8)
    x = rnd((M, N), gpu, seed=9)
    gate = rnd((1, N), gpu, 0.5, seed=10)
    lin = (a.float() @ w.float().t()).to(BF)
    ref = x + gate * lin                        # bf16 torch ops: two roundings, as CleanGeneralDIT.py:517
    xs = x.clone()
    pkg.native.gemm(a, w, out=xs, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=xs)
    ok, msg = ulp_diff_ok(xs, ref, max_ulp=2, frac_exact=0.97)
    assert ok, msg


def test_gemm_rejects_bad_shapes(pkg, gpu):
    a, w = rnd((64, 100), gpu), rnd((128, 100), gpu)
    with pytest.raises(RuntimeError, match="unsupported"):
        pkg.native.gemm(a, w)


# ------------------------------------------------------------------------------------------------ GEMV
def test_gemv_grouped_silu_add_mul(pkg, gpu):
    G, B, Nn, K = 5, 1, 384, 256
    x = rnd((G, B, K), gpu, seed=11)
    w = rnd((G, Nn, K), gpu, 0.1, seed=12)
    add = rnd((1, B, Nn), gpu, seed=13)
    mul = rnd((G, B, Nn), gpu, seed=14)
    out = pkg.native.gemv(x, w, add=add, mul=mul, act=pkg.native.ACT_SILU)
    xa = F.silu(x.cpu()).float()                                   # bf16 rounding of silu as torch CPU does
    lin = torch.einsum("gbk,gnk->gbn", xa, w.cpu().float()).to(BF)
    ref = (mul.cpu() * (lin + add.cpu())).to(gpu)
    ok, msg = ulp_diff_ok(out, ref, max_ulp=2, frac_exact=0.95)
    assert ok, msg


def test_gemv_shared_input(pkg, gpu):
    x = rnd((1, 1, 4096), gpu, seed=15)
    w = rnd((1, 1024, 4096), gpu, 0.02, seed=16)
    out = pkg.native.gemv(x, w)
    ref = (x.float().view(1, 4096) @ w.float().view(1024, 4096).t()).to(BF).view(1, 1, 1024)
    ok, msg = ulp_diff_ok(out, ref)
    assert ok, msg


# ------------------------------------------------------------------------------------------------ norms / RoPE
@pytest.mark.parametrize("rows,D", [(37, 256), (64, 512), (300, 4096)])
def test_ln_modulate_matches_oracle(pkg, gpu, rows, D):
    x = rnd((rows, D), gpu, 2.0, seed=17)
    shift, scale = rnd((1, D), gpu, 0.7, seed=18), rnd((1, D), gpu, 0.7, seed=19)
    out = pkg.native.ln_modulate(x.clone(), shift, scale)
    xc = x.cpu().unsqueeze(1)
    ref = O.modulate(F.layer_norm(xc, (D,), eps=1e-6), shift.cpu(), scale.cpu()).squeeze(1)
    ok, msg = ulp_diff_ok(out.cpu(), ref, max_ulp=1, frac_exact=0.995)
    assert ok, msg


@pytest.mark.parametrize("rows,D,with_add", [(256, 4096, False), (300, 4096, True), (7, 2048, True), (130, 8192, False), (513, 3072, True)])
def test_ln_modulate_four_waves_per_row_equals_one_wave_per_row(pkg, gpu, rows, D, with_add):
    """The two LayerNorm kernels (one wave per row for many rows, four waves per row for few) share one summation tree: same
    bits, so the launcher may pick by row count - and both stay within 1 ulp of the reference ops."""
    lib = pkg.native.load_library()
    x = rnd((rows, D), gpu, 2.0, seed=170)
    B = 2 if rows % 2 == 0 else 1
    shift, scale = rnd((B, D), gpu, 0.7, seed=171), rnd((B, D), gpu, 0.7, seed=172)
    add = rnd((B, D), gpu, 0.5, seed=173) if with_add else None
    outs, xs = {}, {}
    for which in (0, 1):
        lib.drn_ln_force_kernel(which)
        try:
            xs[which] = x.clone()
            outs[which] = pkg.native.ln_modulate(xs[which], shift, scale, add_vec=add, rows_per_batch=rows // B)
        finally:
            lib.drn_ln_force_kernel(-1)
    assert torch.equal(outs[0], outs[1]) and torch.equal(xs[0], xs[1])
    x2 = x.cpu().float()
    if with_add:
        x2 = (x.cpu() + add.cpu().repeat_interleave(rows // B, 0)).float()
        assert torch.equal(xs[1].cpu().float(), x2)
    n = F.layer_norm(x2.to(BF).unsqueeze(1), (D,), eps=1e-6)
    ref = torch.cat([O.modulate(n[b * (rows // B):(b + 1) * (rows // B)], shift[b:b + 1].cpu(), scale[b:b + 1].cpu()) for b in range(B)], 0).squeeze(1)
    ok, msg = ulp_diff_ok(outs[1].cpu(), ref, max_ulp=1, frac_exact=0.995)
    assert ok, msg


@pytest.mark.parametrize("rows,D,K,with_add", [(256, 4096, 4096, True), (256, 4096, 16384, False), (512, 2048, 2048, True), (256, 8192, 2048, False)])
def test_splitk_sum_gated_residual_layernorm_in_one_pass(pkg, gpu, rows, D, K, with_add):
    """drn_gemm_bf16_splitk_partials + drn_splitk_gate_res_ln_modulate (what drn_dit_forward runs for few-token linears) against
    drn_gemm_bf16_splitk(DRN_EPI_GATE_RES) followed by drn_ln_modulate: X and H bit for bit."""
    import ctypes
    N = pkg.native
    lib = N.load_library()
    a, w = rnd((rows, K), gpu, seed=180), rnd((D, K), gpu, K ** -0.5, seed=181)
    x0, gate = rnd((rows, D), gpu, seed=182), rnd((1, D), gpu, 0.5, seed=183)
    shift, scale = rnd((1, D), gpu, 0.7, seed=184), rnd((1, D), gpu, 0.7, seed=185)
    add = rnd((1, D), gpu, 0.5, seed=186) if with_add else None
    splits = lib.drn_gemm_splitk_choice(rows, D, K)
    assert splits > 1, "the shape must take the split-K path"
    # reference: two launches
    x_ref = x0.clone()
    N.gemm(a, w, out=x_ref, epilogue=N.EPI_GATE_RES, gate=gate, residual=x_ref, rows_per_batch=rows)
    h_ref = N.ln_modulate(x_ref, shift, scale, add_vec=add, rows_per_batch=rows)
    # fused: slices only, then one pass
    ws = torch.empty(lib.drn_gemm_splitk_workspace_bytes(rows, D, splits), dtype=torch.uint8, device=gpu)
    st = torch.cuda.current_stream().cuda_stream
    N._check(lib.drn_gemm_bf16_splitk_partials(a.data_ptr(), w.data_ptr(), rows, D, K, K, K, rows, splits, ws.data_ptr(), st), "partials")
    x = x0.clone()
    h = torch.empty_like(x)
    N._check(lib.drn_splitk_gate_res_ln_modulate(ws.data_ptr(), splits, x.data_ptr(), gate.data_ptr(),
                                                 add.data_ptr() if add is not None else None, shift.data_ptr(), scale.data_ptr(),
                                                 h.data_ptr(), rows, D, rows, 1e-6, st), "fused")
    torch.cuda.synchronize()
    assert torch.equal(x, x_ref) and torch.equal(h, h_ref)


def test_ln_modulate_with_broadcast_add(pkg, gpu):
    rows, D = 129, 512
    x = rnd((rows, D), gpu, 2.0, seed=20)
    add = rnd((1, D), gpu, 0.5, seed=21)
    shift, scale = rnd((1, D), gpu, 0.7, seed=22), rnd((1, D), gpu, 0.7, seed=23)
    xs = x.clone()
    out = pkg.native.ln_modulate(xs, shift, scale, add_vec=add)
    x2 = x.cpu() + add.cpu()
    assert torch.equal(xs.cpu(), x2)
    ref = O.modulate(F.layer_norm(x2.unsqueeze(1), (D,), eps=1e-6), shift.cpu(), scale.cpu()).squeeze(1)
    ok, msg = ulp_diff_ok(out.cpu(), ref, max_ulp=1, frac_exact=0.995)
    assert ok, msg
    x3 = x.clone()
    pkg.native.bcast_add(x3, add)
    assert torch.equal(x3.cpu(), x2)


def test_rmsnorm_matches_oracle(pkg, gpu):
    x, w = rnd((3, 4096), gpu, seed=24), rnd((4096,), gpu, seed=25)
    out = pkg.native.rmsnorm(x, w)
    ok, msg = ulp_diff_ok(out.cpu(), O.rms_norm(x.cpu(), w.cpu()), max_ulp=1, frac_exact=0.995)
    assert ok, msg


@pytest.mark.parametrize("heads,T,H,W", [(2, 2, 8, 8), (4, 1, 6, 10), (32, 1, 4, 4)])
def test_qk_norm_rope_matches_oracle(pkg, gpu, heads, T, H, W):
    S, D = T * H * W, heads * 128
    qkv = rnd((S, 3 * D), gpu, 1.5, seed=26)
    wq, wk = 1 + 0.1 * rnd((128,), gpu, seed=27), 1 + 0.1 * rnd((128,), gpu, seed=28)
    seq = torch.arange(512, dtype=torch.float32).to(BF)
    cos, sin = pkg.host_tables.rope_cos_sin(T, H, W, 128, seq)
    ang = O.rope_angles(T, H, W, 128, seq, BF)
    oc, os_ = O.rope_cos_sin(ang, BF)
    assert torch.equal(cos, oc) and torch.equal(sin, os_)           # host tables are bit-exact restatements
    ref_in = qkv.cpu()
    work = qkv.clone()
    pkg.native.qk_norm_rope(work[:, :D], work[:, D:2 * D], wq, wk, cos.to(gpu), sin.to(gpu), heads)
    for idx, wn in ((0, wq), (1, wk)):
        t = ref_in[:, idx * D:(idx + 1) * D].reshape(S, 1, heads, 128)
        ref = O.apply_rope(O.rms_norm(t, wn.cpu()), oc, os_).reshape(S, D)
        ok, msg = ulp_diff_ok(work[:, idx * D:(idx + 1) * D].cpu(), ref, max_ulp=1, frac_exact=0.99)
        assert ok, msg
    assert torch.equal(work[:, 2 * D:], qkv[:, 2 * D:])              # v untouched


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("heads,Sq,Sk", [(2, 256, 256), (2, 128, 128), (4, 300, 300), (1, 513, 77), (32, 256, 1024), (2, 512, 4160)])
def test_attention_matches_fp32(pkg, gpu, heads, Sq, Sk, att_body):
    q = rnd((1, Sq, heads * 128), gpu, seed=29)
    k = rnd((1, Sk, heads * 128), gpu, seed=30)
    v = rnd((1, Sk, heads * 128), gpu, seed=31)
    out = pkg.native.attention(q, k, v, heads=heads)
    _attn_check(out, _attn_ref(q, k, v, heads), f"h{heads} Sq{Sq} Sk{Sk}")


def test_attention_exact_integers_asymmetric(pkg, gpu, att_body):
    """Small-integer Q/K/V with a softmax that is exactly one-hot (one key per query scores far above the rest): O must be
    that key's V row bit for bit - catches any permutation slip in the K / V^T fragment order, the DMA swizzles and the
    LDS-transposed epilogue (asymmetric data: every row and column differs)."""
    heads, S = 2, 320
    D = heads * 128
    q = torch.zeros((1, S, D), dtype=BF, device=gpu)
    k = torch.zeros((1, S, D), dtype=BF, device=gpu)
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(5)).to(gpu)
    cols = torch.arange(S, device=gpu) % 128
    for h in range(heads):
        # query i matches key perm[i]: both carry 40 at column (perm[i] % 128) of head h, plus a tag that separates keys
        # sharing that column
        k[0, torch.arange(S, device=gpu), h * 128 + cols] = 40.0
        k[0, torch.arange(S, device=gpu), h * 128 + (cols + 1 + torch.arange(S, device=gpu) // 128) % 128] = 24.0
        q[0, torch.arange(S, device=gpu), h * 128 + cols[perm]] = 40.0
        q[0, torch.arange(S, device=gpu), h * 128 + (cols[perm] + 1 + perm // 128) % 128] = 24.0
    v = (torch.arange(S * D, device=gpu).reshape(1, S, D) % 251 - 125).to(BF)
    out = pkg.native.attention(q, k, v, heads=heads)
    ref = _attn_ref(q, k, v, heads)
    # (the other keys weigh 2^-73: exact up to that, also where V is 0)
    assert (out.float() - ref).abs().max().item() < 1e-18
    assert (out.float() - v[:, perm].float()).abs().max().item() < 1e-18, "softmax is one-hot here: O[i] == V[perm[i]]"


def test_attention_strided_qkv_buffer(pkg, gpu, att_body):
    heads, S = 2, 320
    D = heads * 128
    qkv = rnd((S, 3 * D), gpu, seed=32)
    q, k, v = (qkv[:, i * D:(i + 1) * D].unsqueeze(0) for i in range(3))
    out = pkg.native.attention(q, k, v, heads=heads)
    _attn_check(out, _attn_ref(q, k, v, heads), "strided qkv")


def test_attention_online_softmax_rescale_spike(pkg, gpu, att_body):
    """Force the running max to jump at a late KV tile (guide rule 26): one key strongly aligned with one query."""
    heads, S = 1, 512
    q = rnd((1, S, 128), gpu, 0.3, seed=33)
    k = rnd((1, S, 128), gpu, 0.3, seed=34)
    v = rnd((1, S, 128), gpu, 1.0, seed=35)
    k[0, 400] = (q[0, 17].float() * 40).to(BF)       # score jumps by a large margin in tile 6
    k[0, 130] = (q[0, 200].float() * 25).to(BF)
    out = pkg.native.attention(q, k, v, heads=heads)
    _attn_check(out, _attn_ref(q, k, v, heads), "rescale spike")


def test_attention_large_scores_no_overflow(pkg, gpu, att_body):
    heads, S = 2, 256
    q = rnd((1, S, heads * 128), gpu, 6.0, seed=36)
    k = rnd((1, S, heads * 128), gpu, 6.0, seed=37)
    v = rnd((1, S, heads * 128), gpu, seed=38)
    out = pkg.native.attention(q, k, v, heads=heads)
    assert torch.isfinite(out.float()).all()
    # scores of +-70: a near one-hot softmax amplifies the bf16 rounding of P on the few surviving keys
    _attn_check(out, _attn_ref(q, k, v, heads), "large scores", rel=6e-3, max_ulp=3, frac_exact=0.4)


# ------------------------------------------------------------------------------------------------ index ops (bit-exact)
@pytest.mark.parametrize("Cc,T,H,W", [(16, 2, 16, 16), (136, 1, 8, 12)])
def test_patchify_concat_bit_exact(pkg, gpu, Cc, T, H, W):
    x = rnd((1, 16, T, H, W), gpu, seed=39)
    cond = rnd((1, Cc, T, H, W), gpu, seed=40)
    C = 16 + Cc + 1
    ldo = (C * 4 + 63) // 64 * 64
    out = pkg.native.patchify_concat(x, cond, True, 1, 2, ldo).cpu()
    xc = torch.cat([x.cpu(), cond.cpu(), torch.ones(1, 1, T, H, W, dtype=BF)], 1)
    ref = O.patchify(xc, 1, 2).reshape(-1, C * 4)
    assert torch.equal(out[:, : C * 4], ref)
    assert (out[:, C * 4:] == 0).all()


def test_unpatchify_bit_exact(pkg, gpu):
    Tp, Hp, Wp = 2, 5, 7
    y = rnd((Tp * Hp * Wp, 128), gpu, seed=41)
    out = pkg.native.unpatchify(y, 1, 16, Tp, Hp, Wp, 1, 2).cpu()
    ref = O.unpatchify(y[:, :64].cpu().reshape(Tp, Hp * Wp, 64), 1, Tp, Hp, Wp, 1, 2, 16)
    assert torch.equal(out, ref)


# ------------------------------------------------------------------------------------------------ sampler / post-process (bit-exact)
def test_edm_kernels_bit_exact(pkg, gpu):
    x = rnd((1, 16, 2, 9, 11), gpu, 40.0, seed=42)
    mo = rnd((1, 16, 2, 9, 11), gpu, 1.0, seed=43)
    sig = O.edm_sigmas(6)
    for i in range(6):
        s, sn = sig[i], sig[i + 1]
        c_in = (1 / torch.sqrt(s ** 2 + 0.5 ** 2)).item()
        assert torch.equal(pkg.native.edm_scale_input(x, c_in).cpu(), O.edm_scale_input(x.cpu(), s))
        c_skip = (0.5 ** 2 / (s ** 2 + 0.5 ** 2)).item()
        c_out = ((s * 0.5) / torch.sqrt(s ** 2 + 0.5 ** 2)).item()
        got = pkg.native.edm_step(mo, x, c_skip, c_out, s.item(), (sn - s).item()).cpu()
        assert torch.equal(got, O.edm_step(mo.cpu(), s, sn, x.cpu())), f"step {i}"


def test_cfg_combine_bit_exact(pkg, gpu):
    c, u = rnd((4096,), gpu, seed=44), rnd((4096,), gpu, seed=45)
    for g in (2.0, 0.7):
        ref = c.cpu() + g * (c.cpu() - u.cpu())
        assert torch.equal(pkg.native.cfg_combine(c, u, g).cpu(), ref)


@pytest.mark.parametrize("normalize", [False, True])
def test_postprocess_u8_bit_exact(pkg, gpu, normalize):
    v = rnd((1, 3, 3, 20, 24), gpu, 0.8, seed=46)
    v[0, :, 0, 0, :4] = 0                       # zero-norm pixels (clamp(min=1e-12) path)
    v[0, :, 0, 1, :8] *= 0.3                    # norms inside the 0.2..0.4 blend band
    got = pkg.native.postprocess_u8(v, normalize).cpu()
    ref = O.postprocess(v.cpu(), normalize)
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} differ"


def test_postprocess_all_bf16_values(pkg, gpu):
    """Every bf16 value in [-1.5, 1.5] through the uint8 conversion."""
    bits = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(BF)
    vals = bits[torch.isfinite(bits.float()) & (bits.float().abs() <= 1.5)]
    n = vals.numel() // 3 * 3
    v = vals[:n].reshape(1, 3, 1, 1, n // 3).contiguous()
    got = pkg.native.postprocess_u8(v.to(gpu), False).cpu()
    assert torch.equal(got, O.postprocess(v, False))


# ------------------------------------------------------------------------------------------------ streamed 256x256 GEMM (M >= 1024)
@pytest.mark.parametrize("M,N,K,epi", [(1024, 256, 64, 0), (1100, 512, 128, 0), (2304, 768, 192, 1), (1537, 256, 320, 2),
                                       (4096, 1024, 1024, 2)])
def test_gemm256_kernel(pkg, gpu, M, N, K, epi, tile=1):
    a, w = rnd((M, K), gpu, seed=50), rnd((N, K), gpu, K ** -0.5, seed=51)
    lin = (a.float() @ w.float().t()).to(BF)
    mag = None
    pkg.native.load_library().drn_gemm_force_tile(tile)
    try:
        if epi == 0:
            out, ref = pkg.native.gemm(a, w), lin
        elif epi == 1:
            out, ref = pkg.native.gemm(a, w, epilogue=pkg.native.EPI_GELU), F.gelu(lin.cpu()).to(gpu)
        else:
            x, gate = rnd((M, N), gpu, seed=52), rnd((1, N), gpu, 0.5, seed=53)
            ref = x + gate * lin
            mag = torch.maximum(x.abs(), (gate * lin).abs())
            out = x.clone()
            pkg.native.gemm(a, w, out=out, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=out)
    finally:
        pkg.native.load_library().drn_gemm_force_tile(-1)
    ok, msg = ulp_diff_ok(out, ref, max_ulp=2, frac_exact=0.97, mag=mag)
    assert ok, msg


@pytest.mark.parametrize("M,N,K,epi", [(300, 256, 4096, 1), (18432, 512, 448, 0)])
def test_gemm256_streamed_kernel_more_k_steps(pkg, gpu, M, N, K, epi):
    """With the cases above: 1, 2, 3, 5, 7, 16, 64 K steps (prologue-only, odd and even step counts)."""
    test_gemm256_kernel(pkg, gpu, M, N, K, epi, tile=1)


def test_gemm256_streamed_identity(pkg, gpu):
    lib = pkg.native.load_library()
    M = K = 1024
    N = 512
    a = torch.eye(M, K, dtype=BF, device=gpu)
    w = (torch.arange(N * K, device=gpu).reshape(N, K) % 251).to(BF)
    lib.drn_gemm_force_tile(1)
    try:
        out = pkg.native.gemm(a, w)
    finally:
        lib.drn_gemm_force_tile(-1)
    assert torch.equal(out, w.t().contiguous())


def test_gemm256_blocked_layouts(pkg, gpu):
    """The rank-major plane layouts of the sequence-parallel exchange (drn_gemm_bf16_blocked) == the plain product."""
    lib = pkg.native.load_library()
    M, N, K, P = 4352, 4096, 512, 4
    a, w = rnd((M, K), gpu, seed=140), rnd((N, K), gpu, K ** -0.5, seed=141)
    a_pl = a.view(M, P, K // P).permute(1, 0, 2).contiguous()
    lib.drn_gemm_force_tile(1)
    try:
        c_pl = torch.empty(P, M, N // P, dtype=BF, device=gpu)
        pkg.native.gemm_blocked(a_pl, w, c_pl, M, a_planes=True, c_planes=True)
        plain = pkg.native.gemm(a, w)
    finally:
        lib.drn_gemm_force_tile(-1)
    assert torch.equal(c_pl.permute(1, 0, 2).reshape(M, N), plain)


@pytest.mark.parametrize("M,N,K,rpb,in_place", [(512, 512, 256, None, False), (2560, 4096, 4096, 1280, True),
                                                 (18432, 4096, 512, 2304, True), (4608, 4096, 16384, None, False)])
def test_gemm256_residual_prefetch_same_bits(pkg, gpu, M, N, K, rpb, in_place):
    """The gated-residual epilogue with the residual tile requested into LDS under the last two K steps == the epilogue that loads
    it after the loop, bit for bit (4 ... 256 K steps, several clips, C aliasing R), and == torch on the rounded linear."""
    lib = pkg.native.load_library()
    a, w = rnd((M, K), gpu, seed=150), rnd((N, K), gpu, K ** -0.5, seed=151)
    B = M // rpb if rpb else 1
    gate, res = rnd((B, N), gpu, seed=152), rnd((M, N), gpu, seed=153)
    outs = []
    lib.drn_gemm_force_tile(1)
    try:
        for on in (1, 0):
            lib.drn_gemm_force_res_prefetch(on)
            x = res.clone()
            out = pkg.native.gemm(a, w, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=x, out=x if in_place else None,
                                  rows_per_batch=rpb, splitk=1)
            outs.append(out.clone())
    finally:
        lib.drn_gemm_force_tile(-1)
        lib.drn_gemm_force_res_prefetch(1)
    assert torch.equal(outs[0], outs[1])
    lin = (a.float() @ w.float().t()).to(BF)
    g = gate.repeat_interleave(M // B, dim=0)
    ref = (res.float() + (g.float() * lin.float()).to(BF).float()).to(BF)
    bad = (outs[0] != ref).float().mean().item()          # the fp32 product may round differently from torch's in a few places
    assert bad < 2e-3, bad


def test_gemm256_residual_prefetch_blocked_a(pkg, gpu):
    """Same check with A stored as rank-major planes (the sequence-parallel output projection's operand layout)."""
    lib = pkg.native.load_library()
    M, N, K, P = 2304, 4096, 4096, 8
    a, w = rnd((M, K), gpu, seed=160), rnd((N, K), gpu, K ** -0.5, seed=161)
    gate, res = rnd((1, N), gpu, seed=162), rnd((M, N), gpu, seed=163)
    a_pl = a.view(M, P, K // P).permute(1, 0, 2).contiguous()
    outs = []
    lib.drn_gemm_force_tile(1)
    try:
        for on in (1, 0):
            lib.drn_gemm_force_res_prefetch(on)
            x = res.clone()
            pkg.native.gemm_blocked(a_pl, w, x, M, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=x, a_planes=True)
            outs.append(x)
        plain = pkg.native.gemm(a, w, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=res)
    finally:
        lib.drn_gemm_force_tile(-1)
        lib.drn_gemm_force_res_prefetch(1)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], plain)


@pytest.mark.parametrize("M,N,K,rpb", [(4352, 4096, 256, 2176), (18432, 4096, 512, None)])
def test_gemm256_gated_residual_in_place(pkg, gpu, M, N, K, rpb):
    """Gated residual in place (C aliases R) on many rounds of tiles, also with a tile that straddles two clips
    (rows_per_batch = 8.5 tiles)."""
    a, w = rnd((M, K), gpu, seed=130), rnd((N, K), gpu, K ** -0.5, seed=131)
    lin = (a.float() @ w.float().t()).to(BF)
    B = M // rpb if rpb else 1
    x, gate = rnd((M, N), gpu, seed=132), rnd((B, N), gpu, 0.5, seed=133)
    out = x.clone()
    pkg.native.gemm(a, w, out=out, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=out, rows_per_batch=rpb)
    g = gate.repeat_interleave(M // B, dim=0)
    ok, msg = ulp_diff_ok(out, x + g * lin, max_ulp=2, frac_exact=0.97, mag=torch.maximum(x.abs(), (g * lin).abs()))
    assert ok, msg


# ------------------------------------------------------------------------------------------------ 144x256 GEMM (token bands, M = 2304 k)
@pytest.mark.parametrize("M,N,K,epi", [(144, 256, 64, 0), (2304, 256, 128, 0), (1000, 512, 192, 0), (2304, 768, 256, 1),
                                       (1537, 256, 320, 2), (2304, 4096, 1024, 2), (150, 256, 4096, 0)])
def test_gemm144_kernel(pkg, gpu, M, N, K, epi):
    test_gemm256_kernel(pkg, gpu, M, N, K, epi, tile=2)


@pytest.mark.parametrize("tile", [1, 2, 3])
def test_gemm_blocked_layouts(pkg, gpu, tile):
    """drn_gemm_bf16_blocked: C written as planes of columns / A read from planes of columns == the plain product regrouped
    (the rank-major slabs either side of the sequence-parallel all-to-all)."""
    lib = pkg.native.load_library()
    M, N, K, P = 1152, 2048, 1024, 4
    a, w = rnd((M, K), gpu, seed=90), rnd((N, K), gpu, K ** -0.5, seed=91)
    lib.drn_gemm_force_tile(tile)
    try:
        plain = pkg.native.gemm(a, w)
        cp = torch.zeros((P, M, N // P), dtype=BF, device=gpu)
        pkg.native.gemm_blocked(a, w, cp, M, c_planes=True)
        assert torch.equal(cp, plain.view(M, P, N // P).permute(1, 0, 2).contiguous())
        ap = a.view(M, P, K // P).permute(1, 0, 2).contiguous()              # [P, M, K/P]
        x, gate = rnd((M, N), gpu, seed=92), rnd((1, N), gpu, 0.5, seed=93)
        ref = x.clone()
        pkg.native.gemm(a, w, out=ref, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=ref)
        out = x.clone()
        pkg.native.gemm_blocked(ap, w, out, M, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=out, a_planes=True)
        assert torch.equal(out, ref)
        assert pkg.native.gemm_blocked_ok(M, N)
    finally:
        lib.drn_gemm_force_tile(-1)
    with pytest.raises(RuntimeError, match="unsupported"):
        pkg.native.gemm_blocked(a[:64], w, torch.zeros((P, 64, N // P), dtype=BF, device=gpu), 64, c_planes=True)   # 128x128 kernel


@pytest.mark.parametrize("M,N,K,epi,splits", [(256, 4096, 4096, 0, 4), (256, 4096, 16384, 2, 8), (200, 512, 2048, 1, 2),
                                              (512, 1024, 1024, 2, None), (77, 256, 4096, 1, 4),
                                              # the cfg-1 linears whose slices run on the streamed 256 x 256 kernel (automatic)
                                              (256, 12288, 4096, 0, None), (256, 16384, 4096, 1, None), (256, 4096, 16384, 2, None),
                                              (512, 12288, 2048, 2, None)])
def test_gemm_splitk_small_m(pkg, gpu, M, N, K, epi, splits):
    """Few tokens (cfg 1): K split over several workgroups per tile, fp32 partials summed by the epilogue kernel."""
    a, w = rnd((M, K), gpu, seed=95), rnd((N, K), gpu, K ** -0.5, seed=96)
    lin = (a.float() @ w.float().t()).to(BF)
    mag = None
    kw = {"splitk": splits}
    if epi == 0:
        out, ref = pkg.native.gemm(a, w, **kw), lin
    elif epi == 1:
        out, ref = pkg.native.gemm(a, w, epilogue=pkg.native.EPI_GELU, **kw), F.gelu(lin.cpu()).to(gpu)
    else:
        x, gate = rnd((M, N), gpu, seed=97), rnd((1, N), gpu, 0.5, seed=98)
        ref = x + gate * lin
        mag = torch.maximum(x.abs(), (gate * lin).abs())
        out = x.clone()
        pkg.native.gemm(a, w, out=out, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=out, **kw)
    ok, msg = ulp_diff_ok(out, ref, max_ulp=2, frac_exact=0.97, mag=mag)
    assert ok, msg


def test_gemm_splitk_choice(pkg):
    f = pkg.native.load_library().drn_gemm_splitk_choice
    # one clip of 256 tokens: gemm_tall.hip - 256 x 64 tiles over the whole K where N / 64 workgroups fill the chip ...
    assert f(256, 12288, 4096) == 1 and f(256, 16384, 4096) == 1     # QKV / MLP-up: 192 / 256 workgroups, no slices
    assert f(256, 4096, 4096) == 4                                   # ... out-proj: 64 tiles x 4 slices of 16 K steps
    assert f(256, 4096, 16384) == 16                                 # MLP-down: 16 tiles of 256^2 x 16 slices (weight-ring kernel)
    assert f(512, 12288, 2048) == 2 and f(1024, 4096, 16384) == 4    # 2-4 clips' rows: 256^2 tiles x slices (weight-ring kernel)
    lib = pkg.native.load_library()
    lib.drn_gemm_force_tile(0)
    try:                                                             # (the 128^2 kernel's own rule)
        assert f(256, 4096, 16384) == 8 and f(256, 12288, 4096) == 2 and f(256, 16384, 4096) == 2
    finally:
        lib.drn_gemm_force_tile(-1)
    assert f(18432, 4096, 4096) == 1 and f(2048, 4096, 4096) == 1    # enough tiles already
    assert f(256, 256, 256) == 1                                     # K too short to split


@pytest.mark.parametrize("M,N,K,epi", [(512, 12288, 2048, 2), (1024, 4096, 4096, 0), (512, 12288, 4352, 1), (1024, 4096, 16384, 2),
                                       (512, 12288, 2560, 0)])
def test_gemm_splitk_weight_ring_kernel_equals_two_stage_kernel(pkg, gpu, M, N, K, epi):
    """The few-token slices on the weight-streaming kernel (A 2 stages + W 3 stages of LDS, W requested three K steps ahead,
    hand-over waits vmcnt 10 / 18 / 10 / 18) against the same slices on the 2 + 2 stage kernel (force_tile 4): the MFMA order per
    output element is the same, so the results must be bit-identical; 16, 34, 64 and 20 K steps per slice (even, and not a
    multiple of the W ring's period).  (One clip of 256 rows takes gemm_tall.hip instead: 512 / 1024 rows here.)"""
    lib = pkg.native.load_library()
    a, w = rnd((M, K), gpu, seed=160), rnd((N, K), gpu, K ** -0.5, seed=161)
    x, gate = rnd((M, N), gpu, seed=162), rnd((1, N), gpu, 0.5, seed=163)
    assert lib.drn_gemm_splitk_choice(M, N, K) > 1
    outs = {}
    for tile in (-1, 4):
        lib.drn_gemm_force_tile(tile)
        try:
            if epi == 2:
                out = x.clone()
                pkg.native.gemm(a, w, out=out, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=out)
            else:
                out = pkg.native.gemm(a, w, epilogue=epi)
            outs[tile] = out
        finally:
            lib.drn_gemm_force_tile(-1)
    assert torch.equal(outs[-1], outs[4])


@pytest.fixture(params=[0, 1], ids=["tall256x64", "tall128x128"])
def tall_shape(request, pkg, gpu):
    lib = pkg.native.load_library()
    lib.drn_gemm_tall_force_shape(request.param)
    yield request.param
    lib.drn_gemm_tall_force_shape(-1)


@pytest.mark.parametrize("N,K,epi", [(12288, 4096, 0), (16384, 4096, 1), (12288, 4096, 2), (4096, 4096, 2), (4096, 16384, 2),
                                     (12288, 192, 1), (16384, 64, 0)])
def test_gemm_tall_kernel(pkg, gpu, N, K, epi, tall_shape):
    """gemm_tall.hip (one clip of 256 rows; 256 x 64 tiles with a 4-stage LDS ring, or 128 x 128 tiles with 5 stages): unsplit it is
    bit-identical to the 128 x 128 kernel run unsplit (same K order per output element) for all three epilogues, in place for
    the gated residual; with K slices (N = 4096) within the usual bound of the fp32 product.  64, 256, 3 and 1 K steps."""
    lib = pkg.native.load_library()
    M = 256
    a, w = rnd((M, K), gpu, seed=170), rnd((N, K), gpu, K ** -0.5, seed=171)
    x, gate = rnd((M, N), gpu, seed=172), rnd((1, N), gpu, 0.5, seed=173)
    splits = lib.drn_gemm_splitk_choice(M, N, K)
    assert splits == (1 if N >= 12288 else (4 if K == 4096 else 16))

    def run(**kw):
        if epi == 2:
            out = x.clone()
            pkg.native.gemm(a, w, out=out, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=out, **kw)
            return out
        return pkg.native.gemm(a, w, epilogue=epi, **kw)

    got = run()
    lib.drn_gemm_force_tile(0)
    try:
        plain = run(splitk=1)
    finally:
        lib.drn_gemm_force_tile(-1)
    if splits == 1:
        assert torch.equal(got, plain)
    else:                                            # the slices do not depend on the tile shape
        lib.drn_gemm_tall_force_shape(1 - tall_shape)
        assert torch.equal(got, run())
        lib.drn_gemm_tall_force_shape(tall_shape)
    lin = (a.float() @ w.float().t()).to(BF)
    mag = None
    if epi == 0:
        ref = lin
    elif epi == 1:
        ref = F.gelu(lin.cpu()).to(gpu)
    else:
        ref = x + gate * lin
        mag = torch.maximum(x.abs(), (gate * lin).abs())
    ok, msg = ulp_diff_ok(got, ref, max_ulp=2, frac_exact=0.97, mag=mag)
    assert ok, msg


def test_gemm_splitk_256_batch_invariant_and_close_to_128_path(pkg, gpu):
    """Two clips of 256 tokens stacked along the rows == each clip alone, bit for bit (slice count and kernel come from one
    clip's rows: gemm_tall.hip, unsplit here); and that path agrees with the 128 x 128 split-K path to fp32-summation noise
    (different slice boundaries: not bit-identical)."""
    lib = pkg.native.load_library()
    N, K = 12288, 4096
    a, w = rnd((512, K), gpu, seed=150), rnd((N, K), gpu, K ** -0.5, seed=151)
    x, gate = rnd((512, N), gpu, seed=152), rnd((2, N), gpu, 0.5, seed=153)
    both = x.clone()
    pkg.native.gemm(a, w, out=both, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=both, rows_per_batch=256)
    for b in range(2):
        one = x[b * 256:(b + 1) * 256].clone()
        pkg.native.gemm(a[b * 256:(b + 1) * 256], w, out=one, epilogue=pkg.native.EPI_GATE_RES, gate=gate[b:b + 1], residual=one)
        assert torch.equal(one, both[b * 256:(b + 1) * 256])
    lib.drn_gemm_force_tile(0)
    try:
        old = x.clone()
        pkg.native.gemm(a, w, out=old, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=old, rows_per_batch=256)
    finally:
        lib.drn_gemm_force_tile(-1)
    assert (old != both).float().mean() < 0.02 and (old.float() - both.float()).abs().max() <= 2 * 2.0 ** -7 * both.float().abs().max()


def test_gemm144_identity_and_choice(pkg, gpu):
    lib = pkg.native.load_library()
    M = K = 2304 // 2
    K = 1152 - 1152 % 64
    N = 512
    a = torch.eye(M, K, dtype=BF, device=gpu)
    w = (torch.arange(N * K, device=gpu).reshape(N, K) % 251).to(BF)
    lib.drn_gemm_force_tile(2)
    try:
        out = pkg.native.gemm(a, w)
    finally:
        lib.drn_gemm_force_tile(-1)
    ref = torch.zeros(M, N, dtype=BF, device=gpu)
    ref[:K] = w.t()[:K]
    assert torch.equal(out, ref)
    # the wave-quantisation model: token bands of 8-way sequence parallelism take the 144-row kernel, full clips the 256^2 one
    assert lib.drn_gemm_tile_choice(2304, 4096) == 2 and lib.drn_gemm_tile_choice(2304, 16384) == 2
    assert lib.drn_gemm_tile_choice(18432, 16384) == 1
    assert lib.drn_gemm_tile_choice(256, 4096) == 0 and lib.drn_gemm_tile_choice(2304, 128) == 0


@pytest.mark.parametrize("rpb", [4608 + 100, 2048])
def test_gemm_tail_split_auto(pkg, gpu, rpb):
    """Automatic dispatch at a shape with a fractional last round (18 x 16 tiles of 256^2 = 1 round + 32): 16 tile rows run
    as 256^2 workgroups, the last 512 (+100 ragged) rows as a second launch; per-batch gates must follow the row offset."""
    M, N, K = 4608 + 100, 4096, 128
    a, w = rnd((M, K), gpu, seed=80), rnd((N, K), gpu, K ** -0.5, seed=81)
    nb = -(-M // rpb)
    x, gate = rnd((M, N), gpu, seed=82), rnd((nb, N), gpu, 0.5, seed=83)
    lin = (a.float() @ w.float().t()).to(BF)
    g_rows = gate[torch.arange(M, device=gpu) // rpb]
    ref = x + g_rows * lin
    out = x.clone()
    pkg.native.gemm(a, w, out=out, epilogue=pkg.native.EPI_GATE_RES, gate=gate, residual=out, rows_per_batch=rpb)
    ok, msg = ulp_diff_ok(out, ref, max_ulp=2, frac_exact=0.97, mag=torch.maximum(x.abs(), (g_rows * lin).abs()))
    assert ok, msg
    ok, msg = ulp_diff_ok(pkg.native.gemm(a, w), lin, max_ulp=1)
    assert ok, msg


def test_gemm256_identity_asymmetric(pkg, gpu):
    M = K = 1024
    N = 256
    a = torch.eye(M, K, dtype=BF, device=gpu)
    w = (torch.arange(N * K, device=gpu).reshape(N, K) % 251).to(BF)
    assert torch.equal(pkg.native.gemm(a, w), w.t().contiguous())


# ------------------------------------------------------------------------------------------------ split-KV attention
@pytest.mark.parametrize("heads,Sq,Sk,ns", [(2, 256, 2048, 2), (4, 300, 4100, 4), (32, 256, 4096, 8)])
def test_attention_splitkv_matches_single_pass(pkg, gpu, heads, Sq, Sk, ns, att_body):
    q = rnd((1, Sq, heads * 128), gpu, seed=60)
    k = rnd((1, Sk, heads * 128), gpu, seed=61)
    v = rnd((1, Sk, heads * 128), gpu, seed=62)
    k[0, Sk - 5] = (q[0, 3].float() * 30).to(BF)          # a late spike: the chunks end with very different maxima
    one = pkg.native.attention(q, k, v, heads=heads, kv_splits=1)
    split = pkg.native.attention(q, k, v, heads=heads, kv_splits=ns)
    ref = _attn_ref(q, k, v, heads)
    _attn_check(one, ref, f"single pass Sk{Sk}")
    _attn_check(split, ref, f"split-KV x{ns} Sk{Sk}")
    assert (split.float() - one.float()).abs().max().item() < 0.02


def test_attention_planned_tail_matches_single_pass(pkg, gpu, att_body):
    """Automatic plan at a band shape: 8 q-blocks unsplit + the 9th in key chunks (native.attention_plan)."""
    heads, Sq, Sk = 32, 2304, 4096
    assert len(pkg.native.attention_plan(1, heads, Sq, Sk)) == 2
    q = rnd((1, Sq, heads * 128), gpu, seed=70)
    k = rnd((1, Sk, heads * 128), gpu, seed=71)
    v = rnd((1, Sk, heads * 128), gpu, seed=72)
    auto = pkg.native.attention(q, k, v, heads=heads)
    one = pkg.native.attention(q, k, v, heads=heads, kv_splits=1)
    assert torch.equal(auto[:, :2048], one[:, :2048])                  # the unsplit part is the same launch arithmetic
    assert (auto.float() - one.float()).abs().max().item() < 0.02
    _attn_check(auto, _attn_ref(q, k, v, heads), "planned tail")


def test_permute_021_bit_exact(pkg, gpu):
    x = torch.randn(37, 8, 1536, device=gpu).to(torch.bfloat16)
    y = pkg.native.permute_021(x)
    assert torch.equal(y, x.permute(1, 0, 2).contiguous())
    z = pkg.native.permute_021(y)
    assert torch.equal(z, x)
