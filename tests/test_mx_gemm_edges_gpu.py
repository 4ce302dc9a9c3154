"""The MXFP8 GEMMs of libdrn.so - drn_gemm_mxfp8 (256 x 256 tiles), drn_gemm_mxfp8_splitk / _splitk_partials (the few-token ring
kernels, both tile shapes) and drn_gemm_mxfp8_gelu_mx - bit for bit at tile, K-ring and clip edges, on the exact data of
tests/mx_gemm_refs.py: small integers under power-of-two block scales, so that every summation order is exact in fp32 and the
expected output has no tolerance (tests/test_mx_gemm_refs_cpu.py proves that per case, and that a dropped K step, a stage mix-up,
a neighbour's scale or gate row, an omitted rounding ... would show).  Only the GELU polynomial keeps a bound: the one the bf16
kernels' GELU epilogue has.

Every case: the outputs live in NaN-sentinel (uint8: 0xA5) guard windows inside one allocation, so a cell that is not written
fails and a store outside the window is found by the guard, never by a fault; the launch is made twice into fresh windows and both
results must be bit-equal; the split-K workspace holds NaNs before every launch.  The `hooks` fixture restores both tuning hooks.
`-s` prints one `mx-gemm-edge` line per case."""
import os

import pytest
import torch
import torch.nn.functional as F

import dit_refs as R
import mx_emul as MX
import mx_gemm_refs as X

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F8 = torch.float8_e4m3fn


@pytest.fixture()
def hooks(pkg):
    """The small-M path on and the default tile shape, whatever an earlier test or the environment left; both restored after."""
    lib = pkg.native.load_library()
    was = lib.drn_gemm_mxfp8_force_small_m(1)
    shape = lib.drn_gemm_mxfp8_tall_force_shape(-1)
    try:
        yield lib
    finally:
        lib.drn_gemm_mxfp8_force_small_m(was)
        lib.drn_gemm_mxfp8_tall_force_shape(shape)


def _mx_operands(pkg, gpu, ops):
    Mx = pkg.native.MxTensor
    return Mx(ops.aq.to(gpu), ops.sa.to(gpu)), Mx(ops.wq.to(gpu), ops.sw.to(gpu))


def _poison_workspace(pkg, gpu, M, N, splits):
    """native.gemm_mxfp8 keeps ONE growing split-K workspace and reuses it as the last launch left it: fill it with NaNs, so that
    a slice tile no workgroup wrote in THIS launch reaches the output as NaN, not as an earlier launch's partials."""
    N_ = pkg.native
    nbytes = N_.load_library().drn_gemm_splitk_workspace_bytes(M, N, splits)
    ws = N_._split_workspace((gpu, "gemm"), nbytes, grow=True)
    ws.view(torch.int16).fill_(R.SENTINEL)
    assert bool(torch.isnan(ws[:nbytes].view(torch.float32)).all())


def _launch(pkg, gpu, lib, c, a, w, gate=None, res=None):
    """One launch of the geometry of case c (an MxCase) on the device operands a, w into fresh windows.  Returns (the output window,
    [(buffer, window), ...] of everything guarded)."""
    N_ = pkg.native
    M = a.shape[0]
    ldc, ldr = X.leading_dims(c)
    cbuf, cv = R.guarded(M, c.N, ldc, 2, gpu)
    guards = [(cbuf, cv)]
    kw = {}
    rv = None
    if c.epi == R.EPI_GATE_RES:
        if c.alias:
            cv.copy_(res)
            rv = cv
        else:
            rbuf, rv = R.guarded(M, c.N, ldr, 2, gpu)
            rv.copy_(res)
            guards.append((rbuf, rv))
        kw = dict(gate=gate.to(gpu), residual=rv)
    if c.kernel == "ring":
        lib.drn_gemm_mxfp8_tall_force_shape(c.shape)
        if c.splits > 1:
            _poison_workspace(pkg, gpu, M, c.N, c.splits)
    N_.gemm_mxfp8(a, w, out=cv, epilogue=c.epi, rows_per_batch=c.rpb, splitk=0 if c.kernel == "k256" else c.splits, **kw)
    torch.cuda.synchronize()
    if rv is not None and not c.alias:
        assert torch.equal(rv.cpu(), res), "the residual is an input: not written"
    return cv, guards


def _twice(pkg, gpu, lib, c, a, w, gate=None, res=None):
    """Two launches into fresh windows: guards intact, no sentinel left, nothing non-finite, both bit-equal.  Returns the CPU copy."""
    out, g1 = _launch(pkg, gpu, lib, c, a, w, gate, res)
    again, g2 = _launch(pkg, gpu, lib, c, a, w, gate, res)
    for buf, v in g1 + g2:
        R.assert_guard_intact(buf, v)
    o, o2 = out.cpu(), again.cpu()
    left = R.is_sentinel(o)
    assert not bool(left.any()), f"{int(left.sum())} cells were never written; first (m, n): {left.nonzero()[:8].tolist()}"
    assert bool(torch.isfinite(o.float()).all()), "a NaN of a guard window or of the workspace reached the result"
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), "two launches of the same case differ"
    return o


def _assert_bit_equal(out, want, tag):
    if not torch.equal(out, want):
        bad = (out != want).nonzero()
        pytest.fail(f"{tag}: {bad.shape[0]} of {out.numel()} outputs differ; first (m, n): {bad[:8].tolist()}")


# ------------------------------------------------------------------------------------------------ the three epilogues, both kernels
@pytest.mark.parametrize("c", X.GRID_K256 + X.GRID_RING, ids=X.case_id)
def test_mx_gemm_edges(pkg, gpu, hooks, c):
    ops = X.operands(c)
    gate, res = X.gate_res(c) if c.epi == R.EPI_GATE_RES else (None, None)
    want = X.expected(c, ops, gate, res)
    a, w = _mx_operands(pkg, gpu, ops)
    out = _twice(pkg, gpu, hooks, c, a, w, gate, res)
    if c.epi == R.EPI_GELU:
        print(f"mx-gemm-edge {X.case_id(c)}: {R.figures(out, want)}")
        ok, msg = X.gelu_check(out, ops.exact.to(BF))
        assert ok, msg
    else:
        _assert_bit_equal(out, want, X.case_id(c))
        print(f"mx-gemm-edge {X.case_id(c)}: bit-equal")


# ------------------------------------------------------------------------------------------------ fp32 slices
@pytest.mark.parametrize("c", X.GRID_SLICES, ids=X.slice_id)
def test_mx_gemm_slices(pkg, gpu, hooks, c):
    """drn_gemm_mxfp8_splitk_partials: slice s is the exact product of its own K range, in fp32, every cell written."""
    ops = X.operands(c)
    want = X.expected_slices(c, ops)
    a, w = _mx_operands(pkg, gpu, ops)
    hooks.drn_gemm_mxfp8_tall_force_shape(c.shape)
    assert c.splits * c.M * c.N * 4 == hooks.drn_gemm_splitk_workspace_bytes(c.M, c.N, c.splits)
    outs = []
    for _ in range(2):
        buf, win = R.guarded(c.splits * c.M, 2 * c.N, 2 * c.N, 2, gpu)           # fp32 [splits, M, N] as pairs of bf16 sentinels
        assert win.data_ptr() % 16 == 0
        rc = hooks.drn_gemm_mxfp8_splitk_partials(a.q.data_ptr(), a.scales.data_ptr(), w.q.data_ptr(), w.scales.data_ptr(), c.M, c.N,
                                                  c.K, c.rpb or 0, c.splits, win.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        R.assert_guard_intact(buf, win)
        outs.append(win.cpu().view(torch.float32).view(c.splits, c.M, c.N))
        left = torch.isnan(outs[-1])
        assert not bool(left.any()), f"{int(left.sum())} cells of the slices were never written; first {left.nonzero()[:4].tolist()}"
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches of the same case differ"
    for s in range(c.splits):
        _assert_bit_equal(outs[0][s], want[s], f"{X.slice_id(c)} slice {s}")
    print(f"mx-gemm-edge slices {X.slice_id(c)}: bit-equal")


# ------------------------------------------------------------------------------------------------ GELU to MX
def _launch_out_mx(pkg, gpu, c, a, w):
    (qb, qv), (sb, sv) = X.out_mx_windows(c.M, c.N, gpu)
    got = pkg.native.gemm_mxfp8(a, w, epilogue=R.EPI_GELU, rows_per_batch=c.rpb, out_mx=pkg.native.MxTensor(qv.view(F8), sv))
    torch.cuda.synchronize()
    assert got.q.data_ptr() == qv.data_ptr() and got.scales.data_ptr() == sv.data_ptr()
    R.assert_guard_intact(qb, qv)
    R.assert_guard_intact(sb, sv)
    return qv.cpu(), sv.cpu()


@pytest.mark.parametrize("c", X.GRID_OUT_MX, ids=X.out_mx_id)
def test_mx_gemm_gelu_mx_edges(pkg, gpu, hooks, c):
    """gemm_mxfp8(out_mx=): the bytes are mx_emul.quantize of the bf16 GELU output the same entry point's bf16 path writes for the
    same operands (the contract of this epilogue, include/drn.h), and that bf16 output keeps the GELU bound on the exact lin."""
    N_ = pkg.native
    hooks.drn_gemm_mxfp8_force_small_m(c.small_m)
    if c.kernel == "ring":
        hooks.drn_gemm_mxfp8_tall_force_shape(c.shape)
    plan = N_.mx_gemm_plan(c.M, c.N, c.K, c.rpb)
    assert plan == (1 if c.kernel == "ring" else 0), "the case must take the kernel it is listed under"
    ops = X.operands(c)
    a, w = _mx_operands(pkg, gpu, ops)
    g = X.as_gelu_case(c)._replace(rpb=c.rpb)
    bf = _twice(pkg, gpu, hooks, g, a, w)
    lin = ops.exact.to(BF)
    ok, msg = X.gelu_check(bf, lin)
    assert ok, msg
    q, s = _launch_out_mx(pkg, gpu, c, a, w)
    q2, s2 = _launch_out_mx(pkg, gpu, c, a, w)
    assert torch.equal(q, q2) and torch.equal(s, s2), "two launches of the same case differ"
    assert not bool(R.is_sentinel(s).any()), "a scale byte was never written"
    ref_q, ref_s = MX.quantize(bf)
    if not torch.equal(s, ref_s):
        bad = (s != ref_s).nonzero()
        pytest.fail(f"{bad.shape[0]} of {s.numel()} scale bytes differ; first (m, block): {bad[:8].tolist()}")
    _assert_bit_equal(q, ref_q.view(torch.uint8), X.out_mx_id(c) + " element bytes")
    print(f"mx-gemm-edge gelu-mx {X.out_mx_id(c)}: bytes bit-equal to quantize(bf16 path); bf16 path {R.figures(bf, F.gelu(lin))}")


# ------------------------------------------------------------------------------------------------ random data, no tolerance
def _rnd_operands(pkg, gpu, M, N, K, seed):
    """mx_quant of randn, as the _gemm_check of tests/test_mxfp8_gpu.py forms its operands."""
    N_ = pkg.native
    return N_.mx_quant(R.rnd((M, K), 1.0, seed).to(gpu)), N_.mx_quant(R.rnd((N, K), K ** -0.5, seed + 1).to(gpu))


def _rows(pkg, a, m):
    return pkg.native.MxTensor(a.q[:m], a.scales[:m])


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("K", [128, 384, 512])
def test_ragged_launch_equals_the_rows_of_the_full_one(pkg, gpu, hooks, K, epi):
    """The rows of a ragged launch of the 256 x 256 kernel (M = 257, M = 1) are bit-equal to the same rows of the M = 512 launch:
    the masked rows of a last tile change nothing in the live ones (clips of 129 rows: the gate row of a row is the same)."""
    N, rpb = 256, 129
    a, w = _rnd_operands(pkg, gpu, 512, N, K, 40 + K + epi)
    gate, res = R.rnd((4, N), 0.5, seed=K + 2), R.rnd((512, N), seed=K + 3)
    full = _twice(pkg, gpu, hooks, X.MxCase("k256", -1, 512, N, K, epi, True, False, rpb, 1, 0), a, w, gate, res)
    for M in (257, 1):
        c = X.MxCase("k256", -1, M, N, K, epi, M == 257, False, rpb, 1, 0)
        part = _twice(pkg, gpu, hooks, c, _rows(pkg, a, M), w, gate[:-(-M // rpb)], res[:M])
        _assert_bit_equal(part, full[:M], f"M={M} K={K} epi={epi} against the rows of M=512")
    print(f"mx-gemm-edge ragged-rows K={K} epi={epi}: M=257 and M=1 bit-equal to the rows of M=512")


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("K", [128, 384, 640])
@pytest.mark.parametrize("M", [256, 512])
def test_kernels_agree_on_random_data(pkg, gpu, hooks, M, K, epi):
    """Where both kernels are legal the 256 x 256 kernel and the two ring shapes at splits = 1 issue the same MFMA sequence per
    output element (one 16 x 16 x 128 scaled MFMA per K step, in K order): the same bits."""
    N = 512
    a, w = _rnd_operands(pkg, gpu, M, N, K, 70 + M + K + epi)
    gate, res = R.rnd((1, N), 0.5, seed=M + K), R.rnd((M, N), seed=M + K + 1)
    outs = [_twice(pkg, gpu, hooks, X.MxCase(kernel, shape, M, N, K, epi, True, False, None, 1, 0), a, w, gate, res)
            for kernel, shape in (("ring", 0), ("ring", 1), ("k256", -1))]
    _assert_bit_equal(outs[1], outs[0], f"ring shape 1 against shape 0, M={M} K={K} epi={epi}")
    d = (outs[2].float() - outs[0].float()).abs() / (torch.maximum(outs[2].float().abs(), outs[0].float().abs()) * 2.0 ** -7).clamp_min(1e-30)
    print(f"mx-gemm-edge kernels-agree M={M} K={K} epi={epi}: ring shapes bit-equal; 256 x 256 kernel against the ring: "
          f"{int((outs[2] != outs[0]).sum())} of {outs[0].numel()} differ, largest {d.max().item():.2f} bf16 ulp")
    _assert_bit_equal(outs[2], outs[0], f"256 x 256 kernel against the ring, M={M} K={K} epi={epi}")


# ------------------------------------------------------------------------------------------------ last: the hooks
def test_hooks_are_back_at_their_defaults(pkg, gpu):
    lib = pkg.native.load_library()
    want = 0 if os.environ.get("DRN_MX_SMALL_M", "")[:1] == "0" else 1
    assert lib.drn_gemm_mxfp8_force_small_m(-1) == want
    assert lib.drn_gemm_mxfp8_tall_force_shape(-1) == -1
