"""Exact-data operands, expected outputs, case grids and a plain-torch stand-in (with mutants) for the MXFP8 GEMM tests
(tests/test_mx_gemm_edges_gpu.py on the GPU, tests/test_mx_gemm_refs_cpu.py for the proof that the grid bites).  Nothing here
touches the GPU.

The data extends test_mxfp8_gpu.test_gemm_lane_map_exact_integers: every element is a small integer (exact in e4m3), every block
scale a power of two, so every term a[m, k] w[n, k] is a multiple of one grid step 2^-(2 + shift) and every partial sum, in ANY
order, stays below 2^24 grid steps (asserted per case by the CPU module): exact in fp32.  The product is therefore fixed to the
bit whatever order v_mfma_scale_f32_16x16x128_f8f6f4 sums its 128 terms in, and the expected outputs below follow from the fp64
product and the rounding points include/drn.h documents (bf16 of the accumulator; bf16 of gate * lin; bf16 of the residual sum)
with no tolerance - the GELU polynomial alone keeps the bound the bf16 kernels' GELU epilogue has (dit_refs.GEMM_BOUND).
The GRID_* lists are iterated by both modules: what is proven on the CPU is exactly what runs on the GPU."""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

import mx_emul as MX
from dit_refs import BF, EPI_GATE_RES, EPI_GELU, EPI_NONE, GEMM_BOUND, guarded, rnd, ulp_diff_ok

F8 = torch.float8_e4m3fn
K_STEP = 128                                   # one K step of every MX GEMM kernel (csrc/gemm_mx.hip, gemm_mx_tall.hip)
RING_STAGES = {0: 3, 1: 4}                     # gemm_mx_tall.hip: shape 0 = 256 x 64 tiles, 3 stages; shape 1 = 128 x 128, 4 stages


# ------------------------------------------------------------------------------------------------ cases
# kernel "k256": drn_gemm_mxfp8 (gemm_mxfp8(splitk=0), 256 x 256 tiles), shape -1.  kernel "ring": drn_gemm_mxfp8_splitk
# (gemm_mxfp8(splitk=splits)) under drn_gemm_mxfp8_tall_force_shape(shape).  strided: ldc = N + 64, ldr = N + 128, the residual in
# a window of its own; else contiguous.  alias: the residual IS the output window.  rpb: rows per clip (None = one clip).
# seed: of the operands - a function of (M, N, K) alone, so the cases of one product share ONE reference.
MxCase = namedtuple("MxCase", "kernel shape M N K epi strided alias rpb splits seed")
# fp32 slices of drn_gemm_mxfp8_splitk_partials
SliceCase = namedtuple("SliceCase", "shape M N K rpb splits seed")
# drn_gemm_mxfp8_gelu_mx (gemm_mxfp8(out_mx=)): the automatic plan decides; small_m = the drn_gemm_mxfp8_force_small_m setting
OutMxCase = namedtuple("OutMxCase", "kernel shape M N K rpb small_m seed")


def seed_of(M, N, K):
    return 7000 + 13 * M + N + 5 * K


def _case(kernel, shape, M, N, K, epi, strided, alias=False, rpb=None, splits=1):
    return MxCase(kernel, shape, M, N, K, epi, strided, alias, rpb, splits, seed_of(M, N, K))


def _k256_grid():
    cases = []
    ks = (128, 256, 384, 512)                  # 1, 2, 3 (odd: the two-stage loop ends on stage 0) and 4 K steps
    for i, M in enumerate((1, 255, 256, 257, 511, 512, 513)):
        for j, N in enumerate((256, 512)):
            for epi in (EPI_NONE, EPI_GELU, EPI_GATE_RES):
                # gated residual: two clips, the boundary inside a row tile (ragged at odd M); M = 1 is one clip
                rpb = (M + 1) // 2 if epi == EPI_GATE_RES else None
                cases.append(_case("k256", -1, M, N, ks[(i + j + epi) % 4], epi, (i + j + epi) % 2 == 0, rpb=rpb))
    # 32 K steps once, every epilogue
    for epi in (EPI_NONE, EPI_GELU, EPI_GATE_RES):
        cases.append(_case("k256", -1, 257, 256, 4096, epi, True, rpb=129 if epi == EPI_GATE_RES else None))
    # in place at a ragged M (strided and contiguous); three clips at M = 513; one clip
    cases.append(_case("k256", -1, 257, 256, 384, EPI_GATE_RES, True, alias=True, rpb=129))
    cases.append(_case("k256", -1, 511, 512, 256, EPI_GATE_RES, False, alias=True, rpb=256))
    cases.append(_case("k256", -1, 513, 512, 256, EPI_GATE_RES, True, rpb=171))
    cases.append(_case("k256", -1, 513, 256, 128, EPI_GATE_RES, False, alias=True, rpb=171))
    cases.append(_case("k256", -1, 255, 256, 128, EPI_GATE_RES, True))
    # the tile map (mx_tile_of): 10 x 3 = 30 workgroups - not a multiple of 8 - in a full L2 band of 8 tile rows and a band of 2
    # that ends ragged (2305 = 9 * 256 + 1); plain, and gated with three ragged clips
    cases.append(_case("k256", -1, 2305, 768, 128, EPI_NONE, True))
    cases.append(_case("k256", -1, 2305, 768, 128, EPI_GATE_RES, False, rpb=769))
    return cases


RING_KS = ((128, 1), (256, 1), (256, 2), (384, 1), (384, 3), (512, 1), (512, 2), (640, 1), (1280, 2))     # (K, splits)
RING_MS = ((256, None), (512, None), (512, 256), (256, 128))                                              # (M, rpb)


def _ring_grid():
    """Both tile shapes x every (K, splits) - 1 .. 5 K steps per slice: fewer than, equal to and more than the stages of either
    ring - x every (M, rpb) x both N x every epilogue; the strides and the in-place residual rotate over them.  (256, 128):
    shape_ok admits it (rows_per_batch only has to divide M); the boundary lies inside shape 0's 256-row tile and on shape 1's
    tile edge."""
    cases = []
    for shape in (0, 1):
        for ik, (K, splits) in enumerate(RING_KS):
            for im, (M, rpb) in enumerate(RING_MS):
                for j, N in enumerate((256, 512)):
                    for epi in (EPI_NONE, EPI_GELU, EPI_GATE_RES):
                        alias = epi == EPI_GATE_RES and (ik + im + j + shape) % 3 == 0
                        cases.append(_case("ring", shape, M, N, K, epi, (ik + 2 * im + j + epi + shape) % 3 != 0, alias, rpb, splits))
    return cases


def _slice_grid():
    cases = []
    for shape in (0, 1):
        for K, splits in RING_KS:
            if splits == 1:
                continue
            for M, rpb in RING_MS:
                for N in (256, 512):
                    cases.append(SliceCase(shape, M, N, K, rpb, splits, seed_of(M, N, K)))
    return cases


def _out_mx_grid():
    cases = []
    for M, small_m in ((1, 1), (255, 1), (257, 1), (513, 1), (256, 0)):
        for K in (128, 384):
            for N in (256, 512):
                cases.append(OutMxCase("k256", -1, M, N, K, None, small_m, seed_of(M, N, K)))
    for shape in (0, 1):
        for M, rpb in ((256, None), (512, 256)):
            for K in (128, 384, 640):
                for N in (256, 512):
                    cases.append(OutMxCase("ring", shape, M, N, K, rpb, 1, seed_of(M, N, K)))
    return cases


GRID_K256 = _k256_grid()
GRID_RING = _ring_grid()
GRID_SLICES = _slice_grid()
GRID_OUT_MX = _out_mx_grid()


def case_id(c):
    head = "k256" if c.kernel == "k256" else f"ring{c.shape}"
    return (f"{head}-M{c.M}-N{c.N}-K{c.K}-epi{c.epi}" + (f"-rpb{c.rpb}" if c.rpb else "") + (f"-s{c.splits}" if c.splits > 1 else "") +
            ("-alias" if c.alias else "") + ("" if c.strided else "-contig"))


def slice_id(c):
    return f"ring{c.shape}-M{c.M}-N{c.N}-K{c.K}" + (f"-rpb{c.rpb}" if c.rpb else "") + f"-s{c.splits}"


def out_mx_id(c):
    head = "k256" if c.kernel == "k256" else f"ring{c.shape}"
    return f"{head}-M{c.M}-N{c.N}-K{c.K}" + (f"-rpb{c.rpb}" if c.rpb else "") + ("" if c.small_m else "-smallm_off")


def as_gelu_case(c):
    """The bf16 GELU launch an OutMxCase is compared with (the same entry point's bf16 path), as an MxCase."""
    return MxCase(c.kernel, c.shape, c.M, c.N, c.K, EPI_GELU, False, False, None, 1, c.seed)


def tile_rows(c):
    return 128 if (c.kernel == "ring" and c.shape == 1) else 256


def leading_dims(c):
    """(ldc, ldr) of the output and residual windows."""
    return (c.N + 64, c.N + 128) if c.strided else (c.N, c.N)


# ------------------------------------------------------------------------------------------------ data
def shift_of(K):
    """Power-of-two shift of the W scales that brings the product's standard deviation near 1 (0.55 .. 1.05 at K = 128 .. 4096), so
    the GELU and the gate work in their interesting range: about log2(62 sqrt(K)).  Exactness is untouched."""
    return round(math.log2(62.0 * math.sqrt(K)))


Operands = namedtuple("Operands", "aq sa wq sw da dw exact shift")


@functools.lru_cache(maxsize=12)
def _operands(M, N, K, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ai = torch.randint(-8, 9, (M, K), generator=g).float()
    wi = torch.randint(-8, 9, (N, K), generator=g).float()
    wi[:, :K // 2] += torch.arange(N).view(N, 1).remainder(5)        # asymmetric: W != W^T structure, row-dependent
    wi = wi.clamp(-15, 15)
    shift = shift_of(K)
    sa = torch.randint(126, 129, (M, K // 32), generator=g).to(torch.uint8)
    sw = (torch.randint(126, 129, (N, K // 32), generator=g) - shift).to(torch.uint8)
    aq, wq = ai.to(F8), wi.to(F8)
    assert torch.equal(aq.float(), ai) and torch.equal(wq.float(), wi), "the integers are exact in e4m3"
    da, dw = MX.dequantize(aq, sa).double(), MX.dequantize(wq, sw).double()
    return Operands(aq, sa, wq, sw, da, dw, da @ dw.t(), shift)


def operands(c):
    """(aq [M, K] e4m3, sa [M, K / 32] uint8, wq [N, K], sw [N, K / 32], their fp64 dequantisations, the fp64 product, shift) of
    case c, built once per (M, N, K, seed) and shared by every case of that product: treat as read-only."""
    return _operands(c.M, c.N, c.K, c.seed)


def clips_of(c):
    return -(-c.M // c.rpb) if c.rpb else 1


def gate_res(c):
    """gate [clips, N], residual [M, N] bf16 (CPU, contiguous; the GPU test places the residual in a window).  The gate has the
    larger spread (2 against 0.5): gate * lin is then of the residual's size, so an omitted intermediate rounding - one ulp of
    gate * lin - survives the final rounding of the sum in more than a tenth of the elements (with a gate of 0.5 against a
    residual of 1, as the bf16 grid has them, it shows in 8 to 9 %: below what the CPU proof asks of every case)."""
    return rnd((clips_of(c), c.N), 2.0, seed=c.seed + 2), rnd((c.M, c.N), 0.5, seed=c.seed + 3)


def exactness_budget(ops):
    """max over (m, n) of sum_k |a| |w| in units of the case's grid step 2^-(2 + shift): below 2^24 every partial sum of every
    summation order is an integer number of grid steps that fp32 holds exactly."""
    return ((ops.da.abs() @ ops.dw.abs().t()).max() * 2.0 ** (2 + ops.shift)).item()


# ------------------------------------------------------------------------------------------------ expected outputs
def epilogue_expected(exact, epi, gate=None, res=None, rpb=None):
    """The kernels' written rounding points (rbf, pack_bf2 and the epilogue of csrc/gemm_mx.hip) in fp32 torch ops on the CPU."""
    lin = exact.to(BF)                       # exact is exact in fp32: one rounding
    if epi == EPI_NONE:
        return lin
    if epi == EPI_GELU:
        return F.gelu(lin)                   # torch CPU bf16 erf-GELU: the reference dit_refs.gemm_ref uses
    M = exact.shape[0]
    gate_row = gate[torch.arange(M) // (rpb if rpb else M)]
    return (res.float() + (gate_row.float() * lin.float()).to(BF).float()).to(BF)


def expected(c, ops=None, gate=None, res=None):
    ops = operands(c) if ops is None else ops
    if c.epi == EPI_GATE_RES and gate is None:
        gate, res = gate_res(c)
    return epilogue_expected(ops.exact, c.epi, gate, res, c.rpb)


def expected_slices(c, ops=None):
    """fp32 [splits, M, N]: slice s is the exact product of its own K range."""
    ops = operands(c) if ops is None else ops
    Ks = c.K // c.splits
    return torch.stack([(ops.da[:, s * Ks:(s + 1) * Ks] @ ops.dw[:, s * Ks:(s + 1) * Ks].t()).float() for s in range(c.splits)])


# ------------------------------------------------------------------------------------------------ stand-in and mutants
ACC_MUTANTS = ("drop_last_kstep", "stage_mixup", "a_scale_prev_block", "scale_row_p1")
EPI_MUTANTS = ("ragged_last_row", "gate_tile_first_row", "rpb_ignored", "res_ldc", "no_rbf_gate_lin", "no_rbf_acc", "swap_row_tiles")
MUTANTS = ACC_MUTANTS + EPI_MUTANTS


@functools.lru_cache(maxsize=64)
def _standin_slices(M, N, K, seed, splits, mutant):
    """fp32 accumulators [splits, M, N] the way the kernels form them: one fp32 product per K step of 128, added step by step
    inside each K slice.  Mutants: "drop_last_kstep" = the last K step never added; "stage_mixup" = K step 1 computed from step
    0's data (a ring stage read one step late); "a_scale_prev_block" = the last 32-block's A scale taken from the block before
    it; "scale_row_p1" = the A scales of row m taken from row m + 1."""
    ops = _operands(M, N, K, seed)
    e = ops.sa.to(torch.int32) - 127
    if mutant == "a_scale_prev_block":
        e = e.clone()
        e[:, -1] = e[:, -2]
    elif mutant == "scale_row_p1":
        e = torch.cat([e[1:], e[-1:]], 0)
    else:
        assert mutant in (None, "drop_last_kstep", "stage_mixup"), mutant
    a32 = torch.ldexp(ops.aq.float().view(M, K // 32, 32), e.unsqueeze(-1).float()).view(M, K)
    w32 = MX.dequantize(ops.wq, ops.sw)
    nk = K // K_STEP
    steps = [a32[:, k * K_STEP:(k + 1) * K_STEP] @ w32[:, k * K_STEP:(k + 1) * K_STEP].t() for k in range(nk)]
    if mutant == "stage_mixup":
        steps[1] = steps[0]
    if mutant == "drop_last_kstep":
        steps[-1] = torch.zeros_like(steps[-1])
    per = nk // splits
    out = []
    for s in range(splits):
        acc = torch.zeros(M, N)
        for t in steps[s * per:(s + 1) * per]:
            acc = acc + t
        out.append(acc)
    return torch.stack(out)


def standin_slices(c, mutant=None):
    return _standin_slices(c.M, c.N, c.K, c.seed, c.splits, mutant)


def standin(c, gate=None, res=None, mutant=None):
    """The whole launch of case c in plain fp32 torch: the slices summed in order (the reduce launch), then the epilogue with its
    rounding points.  `res` may be a strided window (the "res_ldc" mutant then reads it with the OUTPUT's row stride).
    Mutants past the accumulator: "ragged_last_row" = the last row of a ragged tile holds the row before it; "gate_tile_first_row"
    = every row of a row tile takes the gate of the tile's first row; "rpb_ignored" = gate row 0 everywhere; "res_ldc";
    "no_rbf_gate_lin" = gate * lin not rounded to bf16; "no_rbf_acc" = the accumulator not rounded to bf16 before the GELU or the
    gate; "swap_row_tiles" = the first two row tiles stored in each other's place."""
    assert mutant is None or mutant in MUTANTS, mutant
    parts = standin_slices(c, mutant if mutant in ACC_MUTANTS else None)
    acc = parts[0]
    for s in range(1, c.splits):
        acc = acc + parts[s]
    M, T = c.M, tile_rows(c)
    lin = acc if mutant == "no_rbf_acc" else acc.to(BF)
    if c.epi == EPI_NONE:
        out = lin.to(BF)
    elif c.epi == EPI_GELU:
        out = F.gelu(lin).to(BF)
    else:
        rows = torch.arange(M)
        if mutant == "gate_tile_first_row":
            rows = rows // T * T
        b = rows // (c.rpb if c.rpb else M)
        if mutant == "rpb_ignored":
            b = b * 0
        if mutant == "res_ldc":
            res = res.as_strided(res.shape, (leading_dims(c)[0], 1), res.storage_offset())
        g = gate[b].float() * lin.float()
        if mutant != "no_rbf_gate_lin":
            g = g.to(BF).float()
        out = (res.float() + g).to(BF)
    if mutant == "ragged_last_row":
        out = out.clone()
        out[M - 1] = out[M - 2]
    elif mutant == "swap_row_tiles":
        n = min(T, M - T)
        out = torch.cat([out[T:T + n], out[n:T], out[:n], out[T + n:]], 0)
    return out


def mutant_rows(c, mutant, ops=None):
    """bool [M]: the rows mutation `mutant` touches at case c, or None where it does not apply (K = 128 for a dropped step, one
    clip for the gate mutants, another epilogue for the rounding mutants, ...)."""
    ops = operands(c) if ops is None else ops
    M, T = c.M, tile_rows(c)
    rows = torch.arange(M)
    every = torch.ones(M, dtype=torch.bool)
    gated = c.epi == EPI_GATE_RES
    if mutant in ("drop_last_kstep", "stage_mixup"):
        hit = every if c.K >= 2 * K_STEP else None
    elif mutant == "a_scale_prev_block":
        hit = ops.sa[:, -1] != ops.sa[:, -2]
    elif mutant == "scale_row_p1":
        hit = torch.cat([(ops.sa[1:] != ops.sa[:-1]).any(1), torch.zeros(1, dtype=torch.bool)]) if M > 1 else None
    elif mutant == "ragged_last_row":
        hit = rows == M - 1 if (M % T and M > 1) else None
    elif mutant == "gate_tile_first_row":
        hit = (rows // c.rpb != rows // T * T // c.rpb) if (gated and c.rpb) else None
    elif mutant == "rpb_ignored":
        hit = rows >= c.rpb if (gated and c.rpb) else None
    elif mutant == "res_ldc":
        hit = rows >= 1 if (gated and c.strided and not c.alias and M > 1) else None
    elif mutant == "no_rbf_gate_lin":
        hit = every if gated else None
    elif mutant == "no_rbf_acc":
        hit = every if c.epi != EPI_NONE else None
    elif mutant == "swap_row_tiles":
        n = min(T, M - T)
        hit = ((rows < n) | ((rows >= T) & (rows < T + n))) if M > T else None
    else:
        raise AssertionError(mutant)
    return hit if (hit is not None and bool(hit.any())) else None


MIN_SHARE = 0.10          # of the affected elements in every affected row tile: a condition on the data, not a measurement


def mutant_shares(c, out, want, hit):
    """Share of differing elements among the affected rows, per affected row tile."""
    T = tile_rows(c)
    diff = (out != want) | (out.isnan() != want.isnan())          # (NaN != NaN is True already; kept explicit)
    shares = []
    for t0 in range(0, c.M, T):
        h = hit[t0:t0 + T]
        if bool(h.any()):
            shares.append(diff[t0:t0 + T][h].float().mean().item())
    return shares


def gelu_check(out, lin):
    """The GPU module's GELU assertion: the bound the project states for the bf16 kernels' GELU epilogue.  lin is exact here, so
    the fast-GELU polynomial is the only source of difference."""
    return ulp_diff_ok(out, F.gelu(lin), **GEMM_BOUND[EPI_GELU])


# ------------------------------------------------------------------------------------------------ guard windows
def store_past(buffer, view, mutant):
    """A store outside a 2-D guarded window: "row_past_M" = one row past the last; "cols_past_N" = 8 columns past N (on the last row
    where the window is contiguous - the q / scales windows of the GELU-to-MX output - since past any other row lies the next)."""
    off = view.storage_offset() - buffer.storage_offset()
    rows, cols = view.shape
    ld = view.stride(0)
    flat = buffer.view(-1)
    if mutant == "row_past_M":
        flat[off + rows * ld:][:cols] = 1
    elif mutant == "cols_past_N":
        r = rows - 1 if ld == cols else rows // 2
        flat[off + r * ld + cols:][:8] = 1
    else:
        raise AssertionError(mutant)


def out_mx_windows(M, N, device):
    """The guarded uint8 windows of a GELU-to-MX output: q [M, N] and scales [M, N / 32], contiguous as the entry point needs."""
    qb, qv = guarded(M, N, N, 2, device, dtype=torch.uint8)
    sb, sv = guarded(M, N // 32, N // 32, 4, device, dtype=torch.uint8)
    return (qb, qv), (sb, sv)
