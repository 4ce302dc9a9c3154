"""The 384 x 256 GEMM tile at one wave per SIMD (csrc/gemm384.hip, drn_gemm_force_tile(5)) at the smallest shapes at which it can
go wrong: one and two tiles each way, 2 / 3 / 5 K steps (prologue straight into the tail, odd step count, steady state), and one
case with more tiles than CUs (the XCD remap and a second round).  Every case: bit-equal to the 256 x 256 kernel (same MFMA K
order), within the existing GEMM bounds of the fp64 product (dit_refs.GEMM_BOUND = the bounds of tests/test_kernels_gpu.py),
NaN-poisoned surroundings of C untouched."""
import functools

import pytest
import torch

import dit_refs as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TILE384 = 5
BIG = (384 * 8, 256 * 40, 128)                             # 320 tiles on 256 CUs


@functools.lru_cache(maxsize=None)
def _inputs(M, N, K, nb):
    seed = 7000 + M + 3 * N + 7 * K
    a, w = R.rnd((M, K), seed=seed), R.rnd((N, K), K ** -0.5, seed=seed + 1)
    gate, res = R.rnd((nb, N), 0.5, seed=seed + 2), R.rnd((M, N), seed=seed + 3)
    return a, w, gate, res


@functools.lru_cache(maxsize=None)
def _ref(M, N, K, nb, epi):
    """fp64 product rounded as the reference rounds (dit_refs.gemm_ref); computed once per case, shared, never modified."""
    a, w, gate, res = _inputs(M, N, K, nb)
    return R.gemm_ref(a, w, epi, gate, res, M // nb)


def _launch(pkg, gpu, tile, a, w, epi, gate=None, res=None, rpb=None, alias=False):
    """One launch into a fresh guarded C window: two sentinel rows above and below, 64 sentinel columns beside every row.
    Returns (C window, [(buffer, window), ...])."""
    N_ = pkg.native
    lib = N_.load_library()
    M, N = a.shape[0], w.shape[0]
    cbuf, cv = R.guarded(M, N, N + 64, 2, gpu)
    guards = [(cbuf, cv)]
    kw = {}
    if epi == R.EPI_GATE_RES:
        if alias:
            cv.copy_(res)
            rv = cv
        else:
            rbuf, rv = R.guarded(M, N, N + 128, 2, gpu)
            rv.copy_(res)
            guards.append((rbuf, rv))
        kw = dict(gate=gate.to(gpu), residual=rv, rows_per_batch=rpb)
    lib.drn_gemm_force_tile(tile)
    try:
        N_.gemm(a.to(gpu), w.to(gpu), out=cv, epilogue=epi, splitk=1, **kw)
        torch.cuda.synchronize()
    finally:
        lib.drn_gemm_force_tile(-1)
    if epi == R.EPI_GATE_RES and not alias:
        assert torch.equal(rv.cpu(), res), "the residual is an input: not written"
    return cv, guards


def _check(pkg, gpu, M, N, K, epi, nb=1, alias=False):
    a, w, gate, res = _inputs(M, N, K, nb)
    ref, mag = _ref(M, N, K, nb, epi)
    rpb = M // nb if nb > 1 else None
    out, guards = _launch(pkg, gpu, TILE384, a, w, epi, gate, res, rpb, alias)
    old, guards_old = _launch(pkg, gpu, 1, a, w, epi, gate, res, rpb, alias)
    for buf, v in guards + guards_old:
        R.assert_guard_intact(buf, v)
    o = out.cpu()
    print(f"gemm384 M{M} N{N} K{K} epi{epi} clips{nb}{' alias' if alias else ''}: {R.figures(o, ref, mag)}  "
          f"differs from the 256^2 kernel in {(out != old).sum().item()} elements")
    assert torch.equal(out, old), "the 384 x 256 kernel and the 256 x 256 kernel differ (same MFMA K order: same bits expected)"
    ok, msg = R.ulp_diff_ok(o, ref, mag=mag, **R.GEMM_BOUND[epi])
    assert ok, msg
    return out


@pytest.mark.parametrize("K", [128, 192, 320])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [384, 768])
@pytest.mark.parametrize("epi", [R.EPI_NONE, R.EPI_GELU, R.EPI_GATE_RES])
def test_gemm384_small(pkg, gpu, epi, M, N, K):
    _check(pkg, gpu, M, N, K, epi)


@pytest.mark.parametrize("epi", [R.EPI_NONE, R.EPI_GELU, R.EPI_GATE_RES])
def test_gemm384_more_tiles_than_cus(pkg, gpu, epi):
    _check(pkg, gpu, *BIG, epi)


@pytest.mark.parametrize("K", [128, 320])
def test_gemm384_gated_residual_in_place(pkg, gpu, K):
    """The residual aliasing C gives the bits of the residual in its own window."""
    apart = _check(pkg, gpu, 768, 512, K, R.EPI_GATE_RES, alias=False)
    in_place = _check(pkg, gpu, 768, 512, K, R.EPI_GATE_RES, alias=True)
    assert torch.equal(apart, in_place)


@pytest.mark.parametrize("alias", [False, True])
def test_gemm384_two_clips(pkg, gpu, alias):
    """Two clips of 384 rows with different gate rows, stacked: each clip bit-equal to the same clip run alone."""
    M, N, K = 768, 512, 192
    a, w, gate, res = _inputs(M, N, K, 2)
    assert not torch.equal(gate[0], gate[1])
    both = _check(pkg, gpu, M, N, K, R.EPI_GATE_RES, nb=2, alias=alias)
    for b in range(2):
        rows = slice(384 * b, 384 * (b + 1))
        one, guards = _launch(pkg, gpu, TILE384, a[rows], w, R.EPI_GATE_RES, gate[b:b + 1], res[rows], None, alias)
        for buf, v in guards:
            R.assert_guard_intact(buf, v)
        assert torch.equal(one, both[rows]), f"clip {b} of the batch differs from the clip alone"


def test_gemm384_refusals(pkg, gpu):
    """What the kernel cannot take returns DRN_EINVAL and launches nothing: the output keeps its sentinel."""
    N_ = pkg.native
    lib = N_.load_library()
    N, K = 256, 128
    w = R.rnd((N, K), seed=7901).to(gpu)

    def refused(call, cv):
        lib.drn_gemm_force_tile(TILE384)
        try:
            with pytest.raises(RuntimeError, match="unsupported"):
                call()
            torch.cuda.synchronize()
        finally:
            lib.drn_gemm_force_tile(-1)
        assert bool(R.is_sentinel(cv).all()), "a refused launch wrote its output"

    # M = 256: not a whole tile
    a = R.rnd((256, K), seed=7902).to(gpu)
    cbuf, cv = R.guarded(256, N, N, 2, gpu)
    refused(lambda: N_.gemm(a, w, out=cv, splitk=1), cv)
    # a blocked layout (A in two planes of 64 columns)
    a = R.rnd((384, K), seed=7903).to(gpu)
    a_pl = a.view(384, 2, K // 2).permute(1, 0, 2).contiguous()
    cbuf, cv = R.guarded(384, N, N, 2, gpu)
    refused(lambda: N_.gemm_blocked(a_pl, w, cv, 384, a_planes=True), cv)
    # gated residual with clips of 256 rows: a tile would straddle two clips
    a = R.rnd((768, K), seed=7904).to(gpu)
    gate, res = R.rnd((3, N), seed=7905).to(gpu), R.rnd((768, N), seed=7906).to(gpu)
    cbuf, cv = R.guarded(768, N, N, 2, gpu)
    refused(lambda: N_.gemm(a, w, out=cv, epilogue=R.EPI_GATE_RES, gate=gate, residual=res, rows_per_batch=256, splitk=1), cv)
    # and the same launch with whole-tile clips is taken
    N_.load_library().drn_gemm_force_tile(TILE384)
    try:
        N_.gemm(a, w, out=cv, epilogue=R.EPI_GATE_RES, gate=gate[:2], residual=res, rows_per_batch=384, splitk=1)
        torch.cuda.synchronize()
    finally:
        lib.drn_gemm_force_tile(-1)
    assert not bool(R.is_sentinel(cv).any())


def test_gemm384_rerun_equality(pkg, gpu):
    """The largest case 20 times on the same inputs, every result bit-equal to the first: a screen for a fragment read that races
    its DMA (the wait counts are derived in gemm384.hip, not found by this)."""
    N_ = pkg.native
    lib = N_.load_library()
    M, N, K = BIG
    a, w, gate, res = _inputs(M, N, K, 1)
    a, w = a.to(gpu), w.to(gpu)
    lib.drn_gemm_force_tile(TILE384)
    try:
        first = N_.gemm(a, w, splitk=1)
        for i in range(19):
            again = N_.gemm(a, w, splitk=1)
            assert torch.equal(again, first), f"launch {i + 2} differs from the first"
    finally:
        lib.drn_gemm_force_tile(-1)
