"""drn_gemm_mxfp8_blocked (include/drn.h): the MXFP8 GEMM with A | SA and / or C stored in column planes - the rank-major slabs of
the sequence-parallel head <-> token all-to-all.  Same kernel arithmetic as drn_gemm_mxfp8, so every comparison with the plain
layout is bit for bit; shapes are the smallest at which the plane addressing can go wrong (whole tile, ragged second tile, ragged
third tile; two planes each side; guard rows behind every plane)."""
import pytest
import torch

import mx_emul as MX
from conftest import rel_l2

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
N_, K_ = 512, 256
A_COLS, C_COLS = 128, 256                 # 2 planes each
GUARD = 5                                 # rows behind row M of every plane
SENTINEL = -7777.0
POISON_Q, POISON_S = 0x7F, 0xFF           # e4m3 NaN, E8M0 NaN: a guard row that reaches the MFMA poisons the result


def rnd(shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF)


def a_to_planes(Nn, aq, cols, guard=GUARD):
    """MxTensor [M, K] -> MxTensor of planes [P, M, cols] / [P, M, cols / 32], views of allocations with `guard` poison rows behind
    row M of every plane."""
    M, K = aq.q.shape
    P = K // cols
    q = torch.full((P, M + guard, cols), POISON_Q, dtype=torch.uint8, device=aq.q.device)
    s = torch.full((P, M + guard, cols // 32), POISON_S, dtype=torch.uint8, device=aq.q.device)
    q[:, :M] = aq.q.view(torch.uint8).view(M, P, cols).permute(1, 0, 2)
    s[:, :M] = aq.scales.view(M, P, cols // 32).permute(1, 0, 2)
    return Nn.MxTensor(q.view(torch.float8_e4m3fn)[:, :M], s[:, :M])


def c_planes(M, N, cols, device, guard=GUARD):
    """(whole allocation [P, M + guard, cols] filled with the sentinel, the [P, M, cols] view the GEMM writes)."""
    full = torch.full((N // cols, M + guard, cols), SENTINEL, dtype=BF, device=device)
    return full, full[:, :M]


def from_planes(planes):
    P, M, cols = planes.shape
    return planes.permute(1, 0, 2).reshape(M, P * cols)


def _operands(Nn, gpu, M, seed):
    aq = Nn.mx_quant(rnd((M, K_), 1.0, seed).to(gpu))
    wq = Nn.mx_quant(rnd((N_, K_), K_ ** -0.5, seed + 1).to(gpu))
    gate = rnd((1, N_), 0.5, seed + 2).to(gpu)
    resid = rnd((M, N_), 1.0, seed + 3).to(gpu)
    return aq, wq, gate, resid


def _run_blocked(Nn, aq, wq, M, epi, gate, resid, layout):
    """One blocked launch, run twice into the same output: -> (logical [M, N] result, guard rows of C or None)."""
    a = a_to_planes(Nn, aq, A_COLS) if "a" in layout else aq
    kw = dict(epilogue=epi, a_planes="a" in layout, c_planes="c" in layout)
    if epi == Nn.EPI_GATE_RES:
        kw.update(gate=gate, residual=resid)
    if "c" in layout:
        full, out = c_planes(M, N_, C_COLS, aq.q.device)
    else:
        full, out = None, torch.full((M, N_), SENTINEL, dtype=BF, device=aq.q.device)
    Nn.gemm_mxfp8_blocked(a, wq, out, M, **kw)
    first = (from_planes(out) if full is not None else out).clone()
    Nn.gemm_mxfp8_blocked(a, wq, out, M, **kw)
    torch.cuda.synchronize()
    got = from_planes(out) if full is not None else out
    assert torch.equal(first, got), "a repeated launch into the same output changed bits"
    return got, (full[:, M:] if full is not None else None)


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("layout", ["a", "c", "ac"])
@pytest.mark.parametrize("M", [256, 300, 513])
def test_blocked_equals_plain_bit_for_bit(pkg, gpu, M, layout, epi):
    Nn = pkg.native
    aq, wq, gate, resid = _operands(Nn, gpu, M, seed=M + epi)
    kw = dict(gate=gate, residual=resid) if epi == Nn.EPI_GATE_RES else {}
    ref = Nn.gemm_mxfp8(aq, wq, epilogue=epi, splitk=0, **kw)                    # drn_gemm_mxfp8, plain layout
    got, guard = _run_blocked(Nn, aq, wq, M, epi, gate, resid, layout)
    assert torch.isfinite(got.float()).all(), "a poisoned guard row of an A plane was read (load not clamped per plane)"
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {got.numel()} outputs differ from the plain layout"
    if guard is not None:
        assert bool((guard == SENTINEL).all()), "a store past row M landed behind a C plane"


def test_blocked_against_fp64_reference(pkg, gpu):
    """The bound tests/test_mxfp8_gpu.py holds the plain kernel to (rel-L2 < 3e-3), here against the fp64 product of the
    dequantised operands."""
    Nn = pkg.native
    M = 300
    aq, wq, gate, resid = _operands(Nn, gpu, M, seed=9)
    got, _ = _run_blocked(Nn, aq, wq, M, Nn.EPI_NONE, gate, resid, "ac")
    ref = MX.dequantize(aq.q, aq.scales).double() @ MX.dequantize(wq.q, wq.scales).double().t()
    e = rel_l2(got, ref)
    print(f"blocked mxfp8 gemm M={M} N={N_} K={K_}: rel-L2 vs fp64 {e:.2e}")
    assert e < 3e-3, e


def test_blocked_lane_map_exact_integers(pkg, gpu):
    """The construction of test_gemm_lane_map_exact_integers with A in 4 planes of 128 columns and C in 2 planes: small integers,
    block scales 2^-1 .. 2^1 that differ from plane to plane at the same (row, block-in-plane) position, an asymmetric W.  Every
    partial sum is exact in fp32, so the output equals the rounded integer product exactly; an A scale fetched from the wrong
    plane changes it (checked on the reference itself)."""
    Nn = pkg.native
    M, N, K, cols = 48, 512, 512, 128
    g = torch.Generator(device="cpu").manual_seed(5)
    ai = torch.randint(-8, 9, (M, K), generator=g).float()
    wi = torch.randint(-8, 9, (N, K), generator=g).float()
    wi[:, :K // 2] += torch.arange(N).view(N, 1).remainder(5)
    wi = wi.clamp(-15, 15)
    blk = torch.arange(K // 32)
    plane, j = blk // (cols // 32), blk % (cols // 32)
    sa = (126 + (plane.view(1, -1) + j.view(1, -1) + torch.arange(M).view(M, 1)) % 3).to(torch.uint8)
    sw = torch.randint(126, 129, (N, K // 32), generator=g).to(torch.uint8)
    a8, w8 = ai.to(torch.float8_e4m3fn), wi.to(torch.float8_e4m3fn)
    wd = MX.dequantize(w8, sw).double()
    ref = (MX.dequantize(a8, sa).double() @ wd.t()).to(BF)
    sa_wrong = sa.view(M, K // cols, cols // 32).roll(1, 1).reshape(M, K // 32)          # every plane with its neighbour's scales
    assert not torch.equal((MX.dequantize(a8, sa_wrong).double() @ wd.t()).to(BF), ref)
    a = a_to_planes(Nn, Nn.MxTensor(a8.to(gpu), sa.to(gpu)), cols)
    w = Nn.MxTensor(w8.to(gpu), sw.to(gpu))
    full, out = c_planes(M, N, 256, gpu)
    for _ in range(2):
        Nn.gemm_mxfp8_blocked(a, w, out, M, a_planes=True, c_planes=True)
    torch.cuda.synchronize()
    got = from_planes(out).cpu()
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        pytest.fail(f"{bad.shape[0]} of {M * N} outputs differ; first (m, n): {bad[:8].tolist()}")
    assert bool((full[:, M:] == SENTINEL).all())


def test_blocked_rejections_write_nothing(pkg, gpu):
    Nn = pkg.native
    lib = Nn.load_library()
    M = 256
    aq, wq, _, _ = _operands(Nn, gpu, M, seed=1)
    out = torch.full((M + 1, N_), SENTINEL, dtype=BF, device=gpu)

    def call(A=None, SA=None, C=None, abc=0, abs_=0, cbc=0, cbs=0, ldc=N_):
        return lib.drn_gemm_mxfp8_blocked(A or aq.q.data_ptr(), SA or aq.scales.data_ptr(), wq.q.data_ptr(), wq.scales.data_ptr(),
                                          C or out.data_ptr(), M, N_, K_, ldc, 0, None, None, 0, M, abc, abs_, cbc, cbs, None)

    assert call(abc=64, abs_=M * 64) == -1                         # A planes narrower than a K step
    assert call(abc=96, abs_=M * 96) == -1                         # not a multiple of 128
    assert call(abc=128, abs_=M * 128 - 128) == -1                 # planes overlap
    assert call(cbc=128, cbs=M * 128, ldc=128) == -1               # C planes narrower than a tile
    assert call(cbc=256, cbs=M * 256 - 4, ldc=256) == -1           # planes overlap
    assert call(A=aq.q.data_ptr() + 8) == -1                       # misaligned A
    assert call(SA=aq.scales.data_ptr() + 2) == -1                 # misaligned scales
    assert call(C=out.data_ptr() + 2) == -1                        # misaligned C
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to C"
    assert call(abc=128, abs_=M * 128, cbc=256, cbs=M * 256, ldc=256) == 0       # (the same call inside the contract runs)
    torch.cuda.synchronize()
