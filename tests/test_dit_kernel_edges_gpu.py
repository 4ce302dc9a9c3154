"""The DiT kernels of libdrn.so at the geometry the engine calls them with: clip batches, per-clip modulation rows, row-strided
views into packed buffers, offsets, tile edges - against the fp64 / oracle references of tests/dit_refs.py, at the GRID_* cases for
which tests/test_dit_refs_cpu.py has shown a correct stand-in to pass and wrong ones to fail.

Every case: outputs (in-place operands too) live in sentinel-filled guard windows inside one allocation and the guard must be
intact; the padding of strided inputs holds the NaN sentinel and the result must be finite; the launch is made twice into fresh
windows and both results must be bit-equal; every force knob is restored in a `finally`.  Bounds are the ones
tests/test_kernels_gpu.py states.  `-s` prints one `dit-kernel-edge` line of figures per case."""
import pytest
import torch

import dit_refs as R
from conftest import rel_l2
from oracle import dit_oracle as O
from test_gemm_plan_cpu import describe

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _report(family, tag, out, ref, mag=None, atol_rel=2e-3):
    """atol_rel: the absolute allowance of the assertion that follows (ulp_diff_ok's default; 0 for _attn_check)."""
    print(f"dit-kernel-edge {family} {tag}: {R.figures(out, ref, mag, atol_rel)}")


def _window_of(t, ld, gpu, pad_rows=2):
    """A 2-D CPU tensor placed in a guarded GPU window with row stride ld: its padding holds the NaN sentinel."""
    buf, v = R.guarded(t.shape[0], t.shape[1], ld, pad_rows, gpu)
    v.copy_(t)
    return buf, v


def _finite(t):
    return bool(torch.isfinite(t.float()).all())


@pytest.fixture(params=["32x32x16", "16x16x32"])
def att_body(request, pkg):
    """Every attention case runs on both kernel bodies (csrc/attention.hip, csrc/attention16.hip)."""
    lib = pkg.native.load_library()
    lib.drn_attention_force_shape16(1 if request.param == "16x16x32" else 0)
    try:
        yield request.param
    finally:
        lib.drn_attention_force_shape16(-1)


# ------------------------------------------------------------------------------------------------ GEMM
def _gemm_launch(pkg, gpu, c, a, w, gate, res, rows=None):
    """One launch of case c (rows: a row range = one clip alone) into fresh windows.  Returns (C window, [(buffer, window), ...])."""
    N_ = pkg.native
    lib = N_.load_library()
    r0, r1 = rows if rows else (0, c.M)
    M = r1 - r0
    lda, ldc, ldr = (c.K + 64, c.N + 64, c.N + 128) if c.strided else (c.K, c.N, c.N)
    abuf, av = _window_of(a[r0:r1], lda, gpu)
    cbuf, cv = R.guarded(M, c.N, ldc, 2, gpu)
    guards = [(cbuf, cv)]
    # (clips stacked along the rows: the launch plan comes from ONE clip's rows whatever the epilogue)
    kw = dict(rows_per_batch=c.rpb) if (rows is None and c.path != "tile" and c.path != "splitk") else {}
    if c.epi == R.EPI_GATE_RES:
        if c.alias:
            cv.copy_(res[r0:r1])
            rv = cv
        else:
            rbuf, rv = _window_of(res[r0:r1], ldr, gpu)
        g = gate if rows is None else gate[r0 // c.rpb:r0 // c.rpb + 1]
        kw = dict(gate=g.to(gpu), residual=rv, rows_per_batch=c.rpb if rows is None else None)
    wd = w.to(gpu)
    if c.path == "tile":
        lib.drn_gemm_force_tile(c.tile)
    elif c.path.startswith("tall"):
        lib.drn_gemm_tall_force_shape(int(c.path[4]))
    try:
        if c.path == "tile" or c.path == "splitk":
            N_.gemm(av, wd, out=cv, epilogue=c.epi, splitk=c.splits, **kw)
        else:                                             # automatic: the wrapper takes the launch plan from ONE clip's rows
            if c.path.startswith("tall"):
                assert lib.drn_gemm_splitk_choice(c.rpb, c.N, c.K) == c.splits, "the case must take gemm_tall.hip as planned"
            N_.gemm(av, wd, out=cv, epilogue=c.epi, **kw)
        torch.cuda.synchronize()
    finally:
        lib.drn_gemm_force_tile(-1)
        lib.drn_gemm_tall_force_shape(-1)
    if c.epi == R.EPI_GATE_RES and not c.alias:
        assert torch.equal(rv.cpu(), res[r0:r1]), "the residual is an input: not written"
    return cv, guards


@pytest.mark.parametrize("c", R.GRID_GEMM, ids=R.gemm_id)
def test_gemm_edges(pkg, gpu, c):
    a, w, gate, res = R.gemm_inputs(c)
    ref, mag = R.gemm_ref(a, w, c.epi, gate, res, c.rpb)
    out, guards = _gemm_launch(pkg, gpu, c, a, w, gate, res)
    again, guards2 = _gemm_launch(pkg, gpu, c, a, w, gate, res)
    for buf, v in guards + guards2:
        R.assert_guard_intact(buf, v)
    assert _finite(out), "the NaN padding of a strided operand reached the result"
    assert torch.equal(out, again), "two launches of the same case differ"
    o = out.cpu()
    _report("gemm", R.gemm_id(c), o, ref, mag)
    ok, msg = R.ulp_diff_ok(o, ref, mag=mag, **R.GEMM_BOUND[c.epi])
    assert ok, msg
    if c.path == "batched":
        if c.rpb == 9472:
            lib = pkg.native.load_library()
            assert lib.drn_gemm_tile_choice(c.rpb, c.N) == 1, "one clip must take the 256^2 kernel (tail split)"
            ld = (c.K + 64, c.K, c.N + 64, c.N + 128) if c.strided else None
            assert describe(lib, c.M, c.N, c.K, ld=ld, epi=c.epi, rpb=c.rpb) == \
                [(k, b * c.rpb + r0, n, n) for b in range(c.M // c.rpb) for k, r0, n in ((1, 0, 8192), (0, 8192, 1280))], "tail split"
        for b in range(c.M // c.rpb):
            one, g1 = _gemm_launch(pkg, gpu, c, a, w, gate, res, rows=(b * c.rpb, (b + 1) * c.rpb))
            R.assert_guard_intact(*g1[0])
            assert torch.equal(one, out[b * c.rpb:(b + 1) * c.rpb]), f"clip {b} of the batch differs from the clip alone"


# ------------------------------------------------------------------------------------------------ attention
def _poison_splitkv_workspace(N_, gpu, B, H, Sq, ns):
    """native.attention keeps ONE split-KV workspace, keyed by the byte count the sizer returns for the REQUESTED chunk count, and
    reuses it as the last launch left it.  Put a workspace of exactly that size there, every fp32 word a NaN (two bf16 sentinels):
    a combine step that merged a chunk no kernel wrote in THIS launch (77 keys, 4 requested, 2 written) reads NaN, not the partials
    of an earlier identical launch, and the result fails the finite check."""
    nbytes = N_.load_library().drn_attention_splitkv_workspace_bytes(B, H, Sq, ns)
    ws = torch.full((nbytes // 2,), R.SENTINEL, dtype=torch.int16, device=gpu).view(torch.uint8)
    assert ws.numel() == nbytes and bool(torch.isnan(ws.view(torch.float32)).all())
    N_._SPLIT_WS.clear()
    N_._SPLIT_WS[(ws.device, nbytes)] = ws
    return ws


def _attn_launch(pkg, gpu, c, packed, clip=None):
    """drn_attention_bf16 / _splitkv_bf16 on views of the packed buffer (clip: that clip alone, B = 1) into a fresh guarded window
    with ldo = H 128 + 64 and 128 elements between clips."""
    N_ = pkg.native
    HD = c.H * 128
    buf = packed if clip is None else packed[clip:clip + 1]
    q, k, v = R.attn_views(buf, c)
    B = q.shape[0]
    obuf, ov = R.guarded(c.Sq, HD, HD + 64, 2, gpu, batches=B, batch_gap=128)
    o3 = ov if B > 1 else ov.unsqueeze(0)
    ws = _poison_splitkv_workspace(N_, q.device, B, c.H, c.Sq, c.ns) if c.ns > 1 else None
    N_.attention(q, k, v, out=o3, heads=c.H, scale=c.scale, kv_splits=c.ns)
    torch.cuda.synchronize()
    if ws is not None:
        assert list(N_._SPLIT_WS.values())[0] is ws, "the launch must have used the poisoned workspace"
        _, n_eff = R.attn_splits(c.Sk, c.ns)
        words = ws.view(torch.float32)
        live = n_eff * (ws.numel() // 4 // c.ns)
        assert not bool(torch.isnan(words[:live]).any()) and bool(torch.isnan(words[live:]).all()), \
            "the effective chunks' partials are written densely from the start; nothing past them"
    R.assert_guard_intact(obuf, ov)
    return o3


@pytest.mark.parametrize("c", R.GRID_ATTN, ids=R.attn_id)
def test_attention_edges(pkg, gpu, c, att_body):
    cpu = R.attn_packed(c)
    packed = cpu.to(gpu)
    out = _attn_launch(pkg, gpu, c, packed)
    again = _attn_launch(pkg, gpu, c, packed)
    assert torch.equal(packed.view(torch.int16), cpu.to(gpu).view(torch.int16)), "the inputs are not written"
    assert _finite(out), "a sentinel row / column of the packed buffer reached the result"
    assert torch.equal(out, again), "two launches of the same case differ"
    if c.B > 1:
        for b in range(c.B):
            one = _attn_launch(pkg, gpu, c, packed, clip=b)
            assert torch.equal(one[0], out[b]), f"clip {b} of the batch differs from the B = 1 launch of that clip"
    q, k, v = R.attn_views(cpu, c)
    if c.Sk == 1:
        assert torch.equal(out.cpu(), v.expand(-1, c.Sq, -1)), "one key: the output must be V[0] bit for bit"
    ref, _ = R.attention_ref(q, k, v, c.H, c.scale)
    R._attn_check(out.cpu(), ref, f"{R.attn_id(c)} {att_body}")
    _report("attention", f"{R.attn_id(c)} {att_body}", out.cpu(), ref, R._attn_ref.mag, atol_rel=0.0)


def test_attention_splitkv_workspace_sized_for_the_request(pkg, gpu):
    """77 keys in 4 requested chunks run as 2: the launcher's workspace layout must fit the bytes the sizer returns for the REQUEST
    (the caller sizes before it knows the effective count), and for the effective count too."""
    lib = pkg.native.load_library()
    assert R.attn_splits(77, 4) == (64, 2)
    need = 2 * 2 * 129 * 2 * (128 + 2) * 4                # effective chunks x B x Sq x H x (128 + m, l) fp32
    assert lib.drn_attention_splitkv_workspace_bytes(2, 2, 129, 4) >= need
    assert lib.drn_attention_splitkv_workspace_bytes(2, 2, 129, 2) == need
    print(f"dit-kernel-edge attention splitkv-workspace B2-H2-Sq129-Sk77: {need} bytes for the 2 effective chunks, "
          f"{lib.drn_attention_splitkv_workspace_bytes(2, 2, 129, 4)} for the 4 requested")


# ------------------------------------------------------------------------------------------------ q/k RMSNorm + RoPE
def _rope_launch(pkg, gpu, c, qkv, wq, wk, cos, sin):
    D = c.heads * 128
    if c.layout == "packed":
        buf, win = _window_of(qkv, 3 * D + 64, gpu)
        q, k, wins = win[:, :D], win[:, D:2 * D], [(buf, win)]
    else:
        qb, q = _window_of(qkv[:, :D], D + 64, gpu)
        kb, k = _window_of(qkv[:, D:2 * D], D + 128, gpu)
        wins = [(qb, q), (kb, k)]
    cs = (cos.to(gpu), sin.to(gpu)) if c.rope else (None, None)
    pkg.native.qk_norm_rope(q if "q" in c.which else None, k if "k" in c.which else None, wq.to(gpu), wk.to(gpu), *cs, c.heads,
                            tokens_per_batch=c.tpb, pos_offset=c.pos)
    torch.cuda.synchronize()
    for b, v in wins:
        R.assert_guard_intact(b, v)
    return q, k, wins


@pytest.mark.parametrize("c", R.GRID_ROPE, ids=R.rope_id)
def test_qk_norm_rope_edges(pkg, gpu, c):
    qkv, wq, wk, cos, sin = R.rope_inputs(c)
    D = c.heads * 128
    q, k, wins = _rope_launch(pkg, gpu, c, qkv, wq, wk, cos, sin)
    q2, k2, _ = _rope_launch(pkg, gpu, c, qkv, wq, wk, cos, sin)
    assert torch.equal(q, q2) and torch.equal(k, k2), "two launches of the same case differ"
    cs = (cos, sin) if c.rope else (None, None)
    for idx, wn, tag, got in ((0, wq, "q", q), (1, wk, "k", k)):
        x = qkv[:, idx * D:(idx + 1) * D]
        if tag not in c.which:
            assert torch.equal(got.cpu(), x), f"{tag} was not passed: it must be untouched"
            continue
        assert _finite(got)
        ref = R.qk_norm_rope_ref(x, wn, *cs, c.heads, c.tpb, c.pos)
        _report("qk_norm_rope", f"{R.rope_id(c)} {tag}", got.cpu(), ref)
        ok, msg = R.ulp_diff_ok(got.cpu(), ref, **R.ROPE_BOUND)
        assert ok, (tag, msg)
    if c.layout == "packed":
        assert torch.equal(wins[0][1][:, 2 * D:].cpu(), qkv[:, 2 * D:]), "the v columns must be bit-intact"


# ------------------------------------------------------------------------------------------------ LayerNorm + modulate, broadcast add
def _ln_launch(pkg, gpu, c, which, x, shift, scale, add):
    lib = pkg.native.load_library()
    xb, xv = _window_of(x, c.D, gpu)
    hb, hv = R.guarded(c.rows, c.D, c.D, 2, gpu)
    lib.drn_ln_force_kernel(which)
    try:
        pkg.native.ln_modulate(xv, shift.to(gpu), scale.to(gpu), out=hv, add_vec=add.to(gpu) if add is not None else None,
                               rows_per_batch=R.ln_rpb(c))
        torch.cuda.synchronize()
    finally:
        lib.drn_ln_force_kernel(-1)
    R.assert_guard_intact(xb, xv)
    R.assert_guard_intact(hb, hv)
    return xv, hv


@pytest.mark.parametrize("c", R.GRID_LN, ids=R.ln_id)
def test_ln_modulate_edges(pkg, gpu, c):
    x, shift, scale, add = R.ln_inputs(c)
    xref, href = R.ln_modulate_ref(x, shift, scale, add, R.ln_rpb(c))
    outs = {}
    for which in (0, 1):
        xs, h = _ln_launch(pkg, gpu, c, which, x, shift, scale, add)
        xs2, h2 = _ln_launch(pkg, gpu, c, which, x, shift, scale, add)
        assert torch.equal(h, h2) and torch.equal(xs, xs2), "two launches of the same case differ"
        outs[which] = (xs, h)
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[1][0]), "the two LayerNorm kernels must agree bit for bit"
    xs, h = outs[1]
    assert torch.equal(xs.cpu(), xref), "x after the broadcast add (bit-exact; untouched without add_vec)"
    _report("ln_modulate", R.ln_id(c), h.cpu(), href)
    ok, msg = R.ulp_diff_ok(h.cpu(), href, **R.LN_BOUND)
    assert ok, msg
    if add is not None:                                   # the stand-alone broadcast add: the same x
        bb, bv = _window_of(x, c.D, gpu)
        pkg.native.bcast_add(bv, add.to(gpu), rows_per_batch=R.ln_rpb(c))
        torch.cuda.synchronize()
        R.assert_guard_intact(bb, bv)
        assert torch.equal(bv.cpu(), xref)


@pytest.mark.parametrize("with_add", [False, True])
def test_splitk_gate_res_ln_modulate_two_clips(pkg, gpu, with_add):
    """drn_gemm_bf16_splitk_partials + drn_splitk_gate_res_ln_modulate with two clips of 256 rows (per-clip gate, shift, scale,
    add_vec) against drn_gemm_bf16_splitk(GATE_RES) + drn_ln_modulate: X and H bit for bit, in guarded windows, twice."""
    N_ = pkg.native
    lib = N_.load_library()
    rows, D, K, rpb = 512, 4096, 4096, 256
    a, w = R.rnd((rows, K), seed=6000).to(gpu), R.rnd((D, K), K ** -0.5, seed=6001).to(gpu)
    x0 = R.rnd((rows, D), seed=6002)
    gate, shift, scale = (R.rnd((2, D), s, seed=6003 + i).to(gpu) for i, s in enumerate((0.5, 0.7, 0.7)))
    add = R.rnd((2, D), 0.5, seed=6006).to(gpu) if with_add else None
    splits = lib.drn_gemm_splitk_choice(rpb, D, K)
    assert splits > 1, "the shape must take the split-K path"
    xb_ref, x_ref = _window_of(x0, D, gpu)
    N_.gemm(a, w, out=x_ref, epilogue=N_.EPI_GATE_RES, gate=gate, residual=x_ref, rows_per_batch=rpb)
    hb_ref, h_ref = R.guarded(rows, D, D, 2, gpu)
    N_.ln_modulate(x_ref, shift, scale, out=h_ref, add_vec=add, rows_per_batch=rpb)
    st = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in (0, 1):
        ws = torch.empty(lib.drn_gemm_splitk_workspace_bytes(rows, D, splits), dtype=torch.uint8, device=gpu)
        N_._check(lib.drn_gemm_bf16_splitk_partials(a.data_ptr(), w.data_ptr(), rows, D, K, K, K, rpb, splits, ws.data_ptr(), st), "partials")
        xb, x = _window_of(x0, D, gpu)
        hb, h = R.guarded(rows, D, D, 2, gpu)
        N_._check(lib.drn_splitk_gate_res_ln_modulate(ws.data_ptr(), splits, x.data_ptr(), gate.data_ptr(),
                                                      add.data_ptr() if add is not None else None, shift.data_ptr(), scale.data_ptr(),
                                                      h.data_ptr(), rows, D, rpb, 1e-6, st), "fused")
        torch.cuda.synchronize()
        for b, v in ((xb, x), (hb, h), (xb_ref, x_ref), (hb_ref, h_ref)):
            R.assert_guard_intact(b, v)
        runs.append((x, h))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0], x_ref) and torch.equal(runs[0][1], h_ref)
    assert not torch.equal(h_ref[:rpb], h_ref[rpb:])
    print(f"dit-kernel-edge splitk_gate_res_ln_modulate clips2-rows{rows}-D{D}-K{K}-s{splits}-{'add' if with_add else 'noadd'}: "
          f"X and H bit-exact against the two-launch form")


# ------------------------------------------------------------------------------------------------ GEMV, RMSNorm
@pytest.mark.parametrize("c", R.GRID_GEMV, ids=R.gemv_id)
def test_gemv_edges(pkg, gpu, c):
    x, w, add, mul = R.gemv_inputs(c)
    ref = R.gemv_ref(x, w, add, mul, c.act)
    d = [t.to(gpu) if t is not None else None for t in (x, w, add, mul)]
    outs = []
    for _ in (0, 1):
        buf, win = R.guarded(c.G * c.B, c.N, c.N, 2, gpu)
        pkg.native.gemv(d[0], d[1], out=win.view(c.G, c.B, c.N), add=d[2], mul=d[3], act=c.act)
        torch.cuda.synchronize()
        R.assert_guard_intact(buf, win)
        outs.append(win.view(c.G, c.B, c.N))
    assert torch.equal(outs[0], outs[1]) and _finite(outs[0])
    _report("gemv", R.gemv_id(c), outs[0].cpu(), ref)
    ok, msg = R.ulp_diff_ok(outs[0].cpu(), ref, **R.gemv_bound(c))
    assert ok, msg


@pytest.mark.parametrize("rows,D,seed", R.GRID_RMSNORM)
def test_rmsnorm_edges(pkg, gpu, rows, D, seed):
    lib = pkg.native.load_library()
    x, w = R.rnd((rows, D), seed=seed), R.rnd((D,), seed=seed + 1)
    ref = O.rms_norm(x, w)
    xd, wd = x.to(gpu), w.to(gpu)
    outs = []
    for _ in (0, 1):
        buf, win = R.guarded(rows, D, D, 2, gpu)
        pkg.native._check(lib.drn_rmsnorm(xd.data_ptr(), wd.data_ptr(), win.data_ptr(), rows, D, 1e-6,
                                          torch.cuda.current_stream().cuda_stream), "drn_rmsnorm")
        torch.cuda.synchronize()
        R.assert_guard_intact(buf, win)
        outs.append(win)
    assert torch.equal(outs[0], outs[1])
    _report("rmsnorm", f"{rows}x{D}", outs[0].cpu(), ref)
    ok, msg = R.ulp_diff_ok(outs[0].cpu(), ref, **R.RMSNORM_BOUND)
    assert ok, msg


# ------------------------------------------------------------------------------------------------ index / sampler / post-process
def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("B,Cc,T,H,W", R.GRID_PATCHIFY)
def test_patchify_concat_batched(pkg, gpu, B, Cc, T, H, W):
    lib = pkg.native.load_library()
    x, cond = R.rnd((B, 16, T, H, W), seed=7000), R.rnd((B, Cc, T, H, W), seed=7001)
    C = 16 + Cc + 1
    ldo = (C * 4 + 63) // 64 * 64
    rows = B * T * (H // 2) * (W // 2)
    ref = O.patchify(torch.cat([x, cond, torch.ones(B, 1, T, H, W, dtype=BF)], 1), 1, 2).reshape(-1, C * 4)
    xd, cd = x.to(gpu), cond.to(gpu)
    outs = []
    for _ in (0, 1):
        buf, win = R.guarded(rows, ldo, ldo, 2, gpu)
        pkg.native._check(lib.drn_patchify_concat(xd.data_ptr(), cd.data_ptr(), win.data_ptr(), B, 16, Cc, 1, T, H, W, 1, 2, ldo,
                                                  _stream()), "drn_patchify_concat")
        torch.cuda.synchronize()
        R.assert_guard_intact(buf, win)
        outs.append(win)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0][:, :C * 4].cpu(), ref) and bool((outs[0][:, C * 4:] == 0).all())
    print(f"dit-kernel-edge patchify B{B} Cc{Cc} {T}x{H}x{W}: bit-exact")


@pytest.mark.parametrize("B,Tp,Hp,Wp", R.GRID_UNPATCHIFY)
def test_unpatchify_batched(pkg, gpu, B, Tp, Hp, Wp):
    lib = pkg.native.load_library()
    y = R.rnd((B * Tp * Hp * Wp, 64), seed=7010)
    ref = O.unpatchify(y.reshape(B * Tp, Hp * Wp, 64), B, Tp, Hp, Wp, 1, 2, 16)
    yb, yv = _window_of(y, 128, gpu)                      # ldy 128 > 64 live columns: the pad holds the sentinel
    n = ref.numel()
    outs = []
    for _ in (0, 1):
        buf, win = R.guarded(1, n, n + 8 - n % 8, 1, gpu)
        pkg.native._check(lib.drn_unpatchify(yv.data_ptr(), 128, win.data_ptr(), B, 16, Tp, Hp, Wp, 1, 2, _stream()), "drn_unpatchify")
        torch.cuda.synchronize()
        R.assert_guard_intact(buf, win)
        outs.append(win)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0].cpu().view(ref.shape), ref)
    print(f"dit-kernel-edge unpatchify B{B} {Tp}x{Hp}x{Wp}: bit-exact")


@pytest.mark.parametrize("n", R.GRID_SAMPLER_N)
def test_sampler_kernels_odd_counts(pkg, gpu, n):
    lib = pkg.native.load_library()
    x, mo = R.rnd((n,), 40.0, seed=7020), R.rnd((n,), seed=7021)
    xd, md = x.to(gpu), mo.to(gpu)
    sig = O.edm_sigmas(6)
    s, sn = sig[2], sig[3]
    c_in = (1 / torch.sqrt(s ** 2 + 0.5 ** 2)).item()
    c_skip = (0.5 ** 2 / (s ** 2 + 0.5 ** 2)).item()
    c_out = ((s * 0.5) / torch.sqrt(s ** 2 + 0.5 ** 2)).item()

    def run(call):
        outs = []
        for _ in (0, 1):
            buf, win = R.guarded(1, n, n + 8 - n % 8, 1, gpu)
            pkg.native._check(call(win.data_ptr()), "sampler kernel")
            torch.cuda.synchronize()
            R.assert_guard_intact(buf, win)
            outs.append(win.view(-1))
        assert torch.equal(outs[0], outs[1])
        return outs[0].cpu()

    assert torch.equal(run(lambda o: lib.drn_edm_scale_input(xd.data_ptr(), o, n, c_in, _stream())), O.edm_scale_input(x, s))
    assert torch.equal(run(lambda o: lib.drn_edm_step(md.data_ptr(), xd.data_ptr(), o, n, c_skip, c_out, s.item(), (sn - s).item(),
                                                      _stream())), O.edm_step(mo, s, sn, x))
    for g in (2.0, 0.7):
        assert torch.equal(run(lambda o: lib.drn_cfg_combine(md.data_ptr(), xd.data_ptr(), o, n, g, _stream())), mo + g * (mo - x))
    print(f"dit-kernel-edge sampler n{n}: bit-exact")


@pytest.mark.parametrize("B,T,H,W", R.GRID_POSTPROCESS)
@pytest.mark.parametrize("normalize", [False, True])
def test_postprocess_u8_batched_odd_width(pkg, gpu, B, T, H, W, normalize):
    lib = pkg.native.load_library()
    v = R.rnd((B, 3, T, H, W), 0.8, seed=7030)
    v[B - 1, :, 0, 0, :3] = 0                             # zero-norm pixels in the LAST clip
    v[B - 1, :, 0, 1, :5] *= 0.3                          # norms inside the blend band
    ref = O.postprocess(v, normalize)
    vd = v.to(gpu)
    n = ref.numel()
    outs = []
    for _ in (0, 1):
        buf, win = R.guarded(1, n, n + 16 - n % 16, 1, gpu, dtype=torch.uint8)
        pkg.native._check(lib.drn_postprocess_u8(vd.data_ptr(), win.data_ptr(), B, T, H, W, 1 if normalize else 0, _stream()),
                          "drn_postprocess_u8")
        torch.cuda.synchronize()
        R.assert_guard_intact(buf, win)
        outs.append(win)
    assert torch.equal(outs[0], outs[1])
    got = outs[0].cpu().view(ref.shape)
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} differ"
    print(f"dit-kernel-edge postprocess B{B} {T}x{H}x{W} normalize={normalize}: bit-exact")


def test_force_knobs_are_back_at_their_defaults(pkg, gpu):
    """None of the cases above may leave a process-wide override behind for later modules.  pytest runs a module's tests in file
    order, so this one, the last of the file, sees the state the module leaves.  The GEMM knobs are read back directly.
    drn_attention_force_shape16 has no getter: a body left forced to 32x32x16 (the non-default one) shows in
    drn_attention_mx_available(), which follows the selected body; one left forced to the default body is indistinguishable from
    no override.  drn_ln_force_kernel has no getter and, as both LayerNorm kernels agree bit for bit, no observable effect: its
    restoration rests on the try / finally of _ln_launch, the only place that sets it (as that of the attention body rests on
    the att_body fixture's)."""
    import os
    lib = pkg.native.load_library()
    assert lib.drn_gemm_tall_force_shape(-1) == -1
    assert lib.drn_gemm_force_res_prefetch(-1) == 1
    assert lib.drn_gemm_tile_choice(18432, 16384) == 1 and lib.drn_gemm_tile_choice(2304, 4096) == 2      # no forced tile
    assert lib.drn_gemm_splitk_choice(256, 4096, 16384) == 16                                            # (8 under force_tile 0)
    env16 = os.environ.get("DRN_ATT16", "1")[:1] != "0"                                                  # attention_shape16()
    assert bool(lib.drn_attention_mx_available()) == env16, "an attention test left the body forced"
