"""The GEMM executor launches what the planner says: a product through the automatic dispatch against the same product assembled by
hand from the launches drn_gemm_plan_describe reports, each a forced-tile call on its own rows with its clip's gate row.  Equal bit
for bit - the kernels are deterministic and the assembly changes no arithmetic - and nothing outside the windows is written.

The shape is the smallest whose clip splits (tests/test_sp_slab_refs_cpu.py): 4817 rows x 8192 columns = 4096 rows on the 256-row
kernel, then 721 on the 144-row one; K = 128, gated residual, padded row strides.  Plain: two clips, every clip its own two launches
and its own gate row.  C in planes of 1024 columns: one clip (two gated clips in planes take ONE launch - asserted below), the tail
launch advances inside every plane."""
import ctypes

import pytest
import torch

import dit_refs as R
from test_gemm_plan_cpu import describe

pytestmark = pytest.mark.gpu
MB, N, K = 4817, 8192, 128
SPLIT = [(1, 0, 4096, 4096), (2, 4096, 721, 721)]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _product(lib, a, w, c, gate, r, rows, rpb, cbc):
    """drn_gemm_bf16 / _blocked on `rows` rows: a [rows, K], c [rows, N] or planes [P, rows, cbc], r [rows, N], strided views."""
    if cbc:
        rc = lib.drn_gemm_bf16_blocked(_ptr(a), _ptr(w), _ptr(c), rows, N, K, a.stride(0), K, c.stride(1), R.EPI_GATE_RES, _ptr(gate),
                                       _ptr(r), r.stride(0), rpb, 0, 0, cbc, c.stride(0), None)
    else:
        rc = lib.drn_gemm_bf16(_ptr(a), _ptr(w), _ptr(c), rows, N, K, a.stride(0), K, c.stride(0), R.EPI_GATE_RES, _ptr(gate), _ptr(r),
                               r.stride(0), rpb, None)
    assert rc == 0


@pytest.mark.parametrize("clips,cbc", [(2, 0), (1, 1024)], ids=["plain-2clips", "cplanes-1clip"])
def test_executor_launches_the_plan(pkg, gpu, clips, cbc):
    lib = pkg.native.load_library()
    M = clips * MB
    lda, ldc, ldr = K + 64, (cbc or N) + 64, N + 128
    plan = describe(lib, M, N, K, ld=(lda, K, ldc, ldr), epi=R.EPI_GATE_RES, rpb=MB, cbc=cbc)
    assert plan == [(k, b * MB + r0, n, rpb) for b in range(clips) for k, r0, n, rpb in SPLIT]
    assert describe(lib, 2 * MB, N, K, ld=(lda, K, 1088, ldr), epi=R.EPI_GATE_RES, rpb=MB, cbc=1024) == [(1, 0, 2 * MB, MB)]
    a = R.rnd((M, K), seed=9100)
    w = R.rnd((N, K), K ** -0.5, seed=9101).to(gpu)
    gate = R.rnd((clips, N), 0.5, seed=9102).to(gpu)
    abuf, av = R.guarded(M, K, lda, 2, gpu)
    av.copy_(a)
    rbuf, rv = R.guarded(M, N, ldr, 2, gpu)
    rv.copy_(R.rnd((M, N), seed=9103))
    res = rv.clone()

    def window():
        if cbc:
            return R.place_planes(N // cbc, M, cbc, ldc, 128, gpu)
        return R.guarded(M, N, ldc, 2, gpu)

    def rows_of(v, r0, r1):
        return v[:, r0:r1] if cbc else v[r0:r1]

    cbuf, cv = window()
    _product(lib, av, w, cv, gate, rv, M, MB, cbc)
    hbuf, hv = window()
    try:
        for kernel, r0, rows, rpb in plan:
            lib.drn_gemm_force_tile(kernel)
            assert describe(lib, rows, N, K, ld=(lda, K, ldc, ldr), epi=R.EPI_GATE_RES, rpb=rpb, cbc=cbc) == [(kernel, 0, rows, rows)]
            _product(lib, av[r0:r0 + rows], w, rows_of(hv, r0, r0 + rows), gate[r0 // MB:r0 // MB + 1], rv[r0:r0 + rows], rows, rpb, cbc)
    finally:
        lib.drn_gemm_force_tile(-1)
    torch.cuda.synchronize()
    assert torch.equal(cv, hv), "the dispatch and the plan's launches made by hand differ"
    assert bool(torch.isfinite(cv.float()).all()) and torch.equal(rv, res)
    for buf, v in ((cbuf, cv), (hbuf, hv), (abuf, av), (rbuf, rv)):
        R.assert_guard_intact(buf, v)
