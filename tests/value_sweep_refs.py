"""Inputs, fp64 references and comparators of the value sweeps (tests/test_value_sweep_gpu.py on the GPU, tests/test_value_sweep_refs_cpu.py
for the proof that the bounds pass the kernels' arithmetic and fail subtly wrong forms of it).  Nothing here touches the GPU; the
comparators work on whatever device their arguments live on.

The idea: GELU, SiLU and the gated residual are functions of single values, and bf16 has 65 280 finite ones.  A product with a 0/1
weight matrix (one 1.0 per weight row) is exact in fp32 in every summation order, so it carries A[m, k(n)] into C[m, n] unchanged and
what comes out is the epilogue's arithmetic alone: it is held to a relative bound with NO absolute allowance (dit_refs.ulp_diff_ok
adds 2e-3 rms, which hides GELU's whole negative shoulder), and to bit equality where the arithmetic is fixed.

Every per-value reference is a table over the 65 536 bf16 bit patterns (non-finite patterns hold 0 and are never looked up),
gathered by the bits of the value an element carries."""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from dit_refs import BF, _fma32

N_FINITE = 65280
TINY = 2.0 ** -100                 # below this magnitude of the fp64 result only sign and smallness are asked
GELU_TAIL = -4.5                   # gelu_erf_fast's comment: for x < -4.5 neither the kernel's nor the reference's form is accurate
SHARE_MARGIN = 0.01                # the margin tests/test_vae_kernels_gpu.py gives torch on the GroupNorm offset frames


# ------------------------------------------------------------------------------------------------ bits and values
def bf16_of_bits(bits):
    """int tensor of bf16 bit patterns (0 .. 65535) -> bf16."""
    b = bits.to(torch.int32)
    return ((b ^ 0x8000) - 0x8000).to(torch.int16).view(BF)


def bits_of_bf16(t):
    """bf16 -> int64 bit patterns 0 .. 65535 (index into the tables)."""
    return t.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def _all_bits():
    return torch.arange(65536, dtype=torch.int64)


def is_finite_bits(bits):
    return ((bits >> 7) & 0xFF) != 0xFF


def is_denormal_bits(bits):
    return (((bits >> 7) & 0xFF) == 0) & ((bits & 0x7F) != 0)


def is_zero_bits(bits):
    return (bits & 0x7FFF) == 0


@functools.lru_cache(maxsize=1)
def sweep_values():
    """The 65 280 finite bf16 bit patterns (both zeros and the 254 denormals included) in a fixed shuffled order, int64: every
    tile, wave and lane sees every magnitude.  Read-only."""
    b = _all_bits()
    finite = b[is_finite_bits(b)]
    assert finite.numel() == N_FINITE
    g = torch.Generator(device="cpu").manual_seed(20261020)
    return finite[torch.randperm(N_FINITE, generator=g)]


def rbf64(x):
    """fp64 -> the nearest bf16 value (ties to even) in ONE rounding, returned as fp64 (torch's own fp64 -> bf16 goes through fp32:
    two roundings).  Results below bf16's normal range are rounded on the denormal grid 2^-133."""
    _, ex = torch.frexp(x)
    q = torch.ldexp(torch.ones_like(x), (ex - 1).clamp_min(-126) - 7)
    return torch.round(x / q) * q


def ulp_of(ref64):
    """One bf16 ulp of an fp64 value: 2^(floor(log2 |value|) - 7)."""
    _, ex = torch.frexp(ref64)
    return torch.ldexp(torch.ones_like(ref64), ex - 1 - 7)


# ------------------------------------------------------------------------------------------------ per-value tables
Tables = namedtuple("Tables", "x gelu64 gelu_bf gelu_t32 gelu_tbf gelu_tail_tol silu64 silu_bf silu_tbf")


@functools.lru_cache(maxsize=1)
def _tables_cpu():
    bits = _all_bits()
    xb = bf16_of_bits(bits)
    xb = torch.where(is_finite_bits(bits), xb, torch.zeros_like(xb))
    x = xb.double()
    gelu64 = 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    t32 = F.gelu(xb.float())                                         # torch's fp32 formula x 0.5 (1 + erf(x / sqrt 2))
    tail = x < GELU_TAIL
    tol = (t32.double() - gelu64).abs()[tail].max().item()           # its largest absolute error where 1 + erf cancels
    silu64 = x / (1.0 + torch.exp(-x))
    return Tables(x, gelu64, rbf64(gelu64).to(BF), t32, t32.to(BF), tol, silu64, rbf64(silu64).to(BF), F.silu(xb.float()).to(BF))


_TABLES = {}


def tables(device="cpu"):
    """The per-value tables on `device` (built once on the CPU).  gelu64 = 0.5 x erfc(-x / sqrt 2) in fp64, gelu_bf = that rounded
    once to bf16, gelu_t32 / gelu_tbf = torch's fp32 F.gelu and its bf16 rounding, gelu_tail_tol = max |gelu_t32 - gelu64| over
    x < -4.5; silu64 = x / (1 + exp(-x)) in fp64, silu_bf, silu_tbf (torch fp32 F.silu rounded to bf16) likewise."""
    key = str(torch.device(device))
    if key not in _TABLES:
        t = _tables_cpu()
        _TABLES[key] = Tables(*[v.to(device) if torch.is_tensor(v) else v for v in t])
    return _TABLES[key]


# ------------------------------------------------------------------------------------------------ fp32 emulations of the kernels' forms
GELU_Q = (-3.593512520e-04, 6.193101872e-03, -4.942968488e-02, -4.625552893e-01, -1.149885178e+00, -1.000069737e+00)
GELU_MUTANTS = ("phi_tail_zero", "no_abs", "tanh")


def gelu_emul(x, mutant=None):
    """gelu_erf_fast of csrc/drn_common.h on bf16 x: the degree-5 polynomial q(|x|) as an fp32 fma chain, an exact exp2 rounded to
    fp32, max(x, 0) and the last fma(-|x|, e, relu); rounded to bf16.  Mutants: "phi_tail_zero" = Phi(-a) = 0 for a > 3.5 (the whole
    negative shoulder lost), "no_abs" = the last fma without its |x| modifier, "tanh" = the tanh approximation."""
    assert mutant is None or mutant in GELU_MUTANTS, mutant
    xf = x.float()
    if mutant == "tanh":
        return F.gelu(xf, approximate="tanh").to(BF)
    a = xf.abs()
    c = [torch.tensor(v, dtype=torch.float32) for v in GELU_Q]
    q = _fma32(c[0].expand_as(a), a, c[1].expand_as(a))
    for k in c[2:]:
        q = _fma32(q, a, k.expand_as(a))
    e = torch.exp2(q.double()).float()
    if mutant == "phi_tail_zero":
        e = torch.where(a > 3.5, torch.zeros_like(e), e)
    relu = xf.clamp_min(0.0)
    return _fma32(-(xf if mutant == "no_abs" else a), e, relu).to(BF)


SILU_FORMS = ("gemv", "gn")


def silu_emul(x, form, mutant=None):
    """The two SiLU forms in fp32 on bf16 x, rounded to bf16: "gemv" = x / (1 + expf(-x)) (csrc/gemv.hip), "gn" = o * rcp(1 +
    exp2(-o log2 e)) (gn_apply_kernel of csrc/vae_kernels.hip; exp2 and the reciprocal exact, rounded to fp32).  Mutant "exp_pos":
    exp(x) in place of exp(-x)."""
    assert form in SILU_FORMS and mutant in (None, "exp_pos"), (form, mutant)
    xf = x.float()
    s = 1.0 if mutant == "exp_pos" else -1.0
    if form == "gemv":
        return (xf / (1.0 + torch.exp((s * xf).double()).float())).to(BF)
    t = torch.tensor(s * 1.44269504088896340736, dtype=torch.float32) * xf
    d = 1.0 + torch.exp2(t.double()).float()
    return (xf * (1.0 / d.double()).float()).to(BF)


GATE_MUTANTS = ("one_fma",)


def gate_res_chain(lin, gate_rows, res, mutant=None):
    """The documented rounding x + rbf(g * v): torch's bf16 chain `res + gate * lin` (two roundings; what dit_refs.gemm_ref does).
    lin, res [M, N] bf16, gate_rows [M, N] bf16 (the clip's gate row per output row).  Mutant "one_fma" = fma(g, v, x), ONE
    rounding.  (Another clip's gate is a mutation of gate_rows, which the caller builds: tests/test_value_sweep_refs_cpu.py.)"""
    assert mutant is None or mutant in GATE_MUTANTS, mutant
    if mutant == "one_fma":
        return _fma32(gate_rows.float(), lin.float(), res.float()).to(BF)
    return res + gate_rows * lin


# ------------------------------------------------------------------------------------------------ comparators
Figures = namedtuple("Figures", "worst_ulp share torch_share excluded failures")


def line(site, f):
    """The `value-sweep` line of one case."""
    return (f"value-sweep {site}: worst {f.worst_ulp:.3f} ulp  bit-equal {f.share:.5f}  torch {f.torch_share:.5f}  "
            f"excluded {f.excluded}")


def _first(mask, xb):
    idx = mask.reshape(-1).nonzero().flatten()[:4]
    return [hex(int(v)) for v in xb.reshape(-1)[idx].tolist()]


def _finite_part(out64, inc, fails, what):
    """No included output is inf or NaN (a NaN is also what a cell that was never written holds); returns out64 made finite."""
    nf = inc & ~torch.isfinite(out64)
    if bool(nf.any()):
        fails.append(f"{what}: {int(nf.sum())} non-finite outputs")
    return torch.nan_to_num(out64, nan=1e300, posinf=1e300, neginf=-1e300)


def _ulp_part(out64, ref64, xb, mask, fails, what):
    """|out - ref| <= 1 ulp of ref on `mask`; returns the worst distance in ulps."""
    if not bool(mask.any()):
        return 0.0
    d = ((out64 - ref64).abs() / ulp_of(torch.where(mask, ref64, torch.ones_like(ref64))))[mask]
    bad = d > 1.0
    if bool(bad.any()):
        fails.append(f"{what}: {int(bad.sum())} outputs further than 1 ulp from the fp64 value, worst {d.max().item():.2f} ulp; "
                     f"first input bits {_first(mask & ((out64 - ref64).abs() > ulp_of(torch.where(mask, ref64, torch.ones_like(ref64)))), xb)}")
    return d.max().item()


def _tiny_part(out64, ref64, xb, mask, fails, what):
    """Where |fp64 result| < 2^-100: the output is zero, or has the result's sign and a magnitude <= 2^-100."""
    ok = (out64 == 0) | ((torch.sign(out64) == torch.sign(ref64)) & (out64.abs() <= TINY))
    bad = mask & ~ok
    if bool(bad.any()):
        fails.append(f"{what}: {int(bad.sum())} outputs neither zero nor tiny with the right sign where |fp64| < 2^-100; "
                     f"first input bits {_first(bad, xb)}")


def _share_part(out, ref_bf, torch_bf, mask, fails, what):
    n = int(mask.sum())
    if n == 0:
        return 1.0, 1.0
    share = (((out == ref_bf) & mask).sum() / n).item()
    tshare = (((torch_bf == ref_bf) & mask).sum() / n).item()
    if share < tshare - SHARE_MARGIN:
        fails.append(f"{what}: bit-equal share {share:.5f} below torch's {tshare:.5f} - {SHARE_MARGIN}")
    return share, tshare


def gelu_check(xb, out, excluded=None):
    """xb: int64 bits of the value each element carried into the GELU, out: bf16, excluded: bool (inputs the carrier flushed).
    The bounds of the sweep, none with an absolute allowance:
      x >= -4.5, |fp64| >= 2^-100   within 1 ulp of 0.5 x erfc(-x / sqrt 2)
      2^-10 <= |x| < 8, x >= -4.5   bit-equal share >= torch fp32 F.gelu rounded to bf16 on the same elements - 0.01
      x < -4.5                      out <= 0 and |out - fp64| <= the largest error of torch's fp32 formula in that region
      |fp64| < 2^-100               zero, or the right sign and <= 2^-100
    Returns Figures; .failures is empty when every bound holds."""
    T = tables(out.device)
    inc = is_finite_bits(xb) if excluded is None else is_finite_bits(xb) & ~excluded
    x, ref = T.x[xb], T.gelu64[xb]
    o = out.double()
    fails = []
    o = _finite_part(o, inc, fails, "gelu")
    head = inc & (x >= GELU_TAIL)
    worst = _ulp_part(o, ref, xb, head & (ref.abs() >= TINY), fails, "gelu x >= -4.5")
    _tiny_part(o, ref, xb, head & (ref.abs() < TINY), fails, "gelu")
    tail = inc & (x < GELU_TAIL)
    bad = tail & ((o > 0) | ((o - ref).abs() > T.gelu_tail_tol))
    if bool(bad.any()):
        fails.append(f"gelu x < -4.5: {int(bad.sum())} outputs positive or further than {T.gelu_tail_tol:.3e} from the fp64 value "
                     f"(worst {(o - ref).abs()[tail].max().item():.3e}); first input bits {_first(bad, xb)}")
    live = head & (x.abs() >= 2.0 ** -10) & (x.abs() < 8.0)              # (the tail has its own bound: no form is accurate there)
    share, tshare = _share_part(out, T.gelu_bf[xb], T.gelu_tbf[xb], live, fails, "gelu live range")
    return Figures(worst, share, tshare, int((~inc).sum()), fails)


def silu_check(xb, out, excluded=None, scale=None):
    """SiLU of the carried value (times `scale`, a tensor of powers of two, where given): within 1 ulp of the fp64 x / (1 + exp(-x))
    where |fp64| >= 2^-100 (and, scaled, below 2^126), zero or tiny with the right sign below that; bit-equal share >= torch fp32
    F.silu rounded to bf16 - 0.01."""
    T = tables(out.device)
    inc = is_finite_bits(xb) if excluded is None else is_finite_bits(xb) & ~excluded
    ref, ref_bf, t_bf = T.silu64[xb], T.silu_bf[xb], T.silu_tbf[xb]
    if scale is not None:
        ref, ref_bf, t_bf = ref * scale.double(), ref_bf * scale.to(BF), t_bf * scale.to(BF)
        inc = inc & (ref.abs() < 2.0 ** 126)
    o = out.double()
    fails = []
    o = _finite_part(o, inc, fails, "silu")
    big = inc & (ref.abs() >= TINY)
    worst = _ulp_part(o, ref, xb, big, fails, "silu")
    _tiny_part(o, ref, xb, inc & (ref.abs() < TINY), fails, "silu")
    share, tshare = _share_part(out, ref_bf, t_bf, big, fails, "silu")
    return Figures(worst, share, tshare, int((~inc).sum()), fails)


GATE_EXCLUDED_CAP = 0.02


def gate_res_excluded(lin, gate_rows, res):
    """bool [M, N]: elements whose fp32 product g v or whose sum is denormal or overflows (what the hardware does with fp32
    denormals, and where inf appears, is not part of the contract)."""
    p = gate_rows.double() * lin.double()
    lo, hi = 2.0 ** -126, 3.3895313892515355e38                       # smallest normal; bf16 max
    pb = rbf64(p)
    s = res.double() + pb
    sb = rbf64(s)
    return ((p != 0) & (p.abs() < lo)) | (pb.abs() > hi) | ((s != 0) & (s.abs() < lo)) | (sb.abs() > hi)


def gate_res_check(out, lin, gate_rows, res, excluded=None):
    """out == torch's bf16 chain res + gate * lin, bit for bit, wherever product and sum are normal or zero; the excluded elements
    are counted and may not exceed 2 % of the case.  excluded: further elements to leave out (inputs the carrier flushed)."""
    ex = gate_res_excluded(lin, gate_rows, res)
    if excluded is not None:
        ex = ex | excluded
    want = gate_res_chain(lin, gate_rows, res)
    diff = (bits_of_bf16(out) != bits_of_bf16(want)).view(out.shape) & ~ex
    fails = []
    n = out.numel()
    if bool(diff.any()):
        idx = diff.nonzero()[:4].tolist()
        fails.append(f"gated residual: {int(diff.sum())} of {n} outputs differ from res + rbf(gate * lin); first (m, n) {idx}")
    if int(ex.sum()) > GATE_EXCLUDED_CAP * n:
        fails.append(f"gated residual: {int(ex.sum())} of {n} elements excluded, more than {GATE_EXCLUDED_CAP:.0%}")
    inc = ~ex
    share = 1.0 - diff.sum().item() / max(int(inc.sum()), 1)
    d = (out.double() - want.double()).abs() / ulp_of(torch.where(want.double() != 0, want.double(), torch.ones_like(want.double())))
    d = torch.where(inc & torch.isfinite(d), d, torch.zeros_like(d))
    return Figures(d.max().item(), share, 1.0, int(ex.sum()), fails)


# ------------------------------------------------------------------------------------------------ the carrier: a 0/1 product
# site: the kernel (and, for split-K, the slice kernel in front of the shared reduce epilogue).  kernel: the id
# drn_gemm_plan_describe reports for it (csrc/gemm_plan.h).  force: drn_gemm_force_tile
# (-1 automatic).  tall: drn_gemm_tall_force_shape (-1 = not set).  rpb: rows per clip.  splitk: what native.gemm is given
# (None = automatic, 1 = unsplit, n = n slices).  Shapes: the smallest each kernel takes (csrc/gemm_plan.h: the 144-row tile from
# M = 144, drn_gemm384_ok: M % 384 == 0 and K >= 128, gemm_tall_slices: clips of 256 rows with N / 64 >= 192 unsplit); the split-K
# shapes are those of dit_refs.GRID_GEMM (128^2 slices), test_gemm_splitk_weight_ring_kernel_equals_two_stage_kernel (256-row slices)
# and GRID_GEMM's tall cases (few-token K slices).  rpb = 300 at M = 512: two ragged clips, so that one clip's rows stay 512 and the
# slices stay on the 256-row kernels (clips of 256 rows would take the few-token kernel).
SweepSite = namedtuple("SweepSite", "name kernel force tall M N K rpb splitk splits")
GEMM_SITES = (
    SweepSite("k128", 0, 0, -1, 256, 256, 256, 128, 1, 1),
    SweepSite("k256s", 1, 1, -1, 256, 256, 256, 128, 1, 1),
    SweepSite("k144", 2, 2, -1, 288, 256, 256, 144, 1, 1),
    SweepSite("k384", 5, 5, -1, 384, 256, 256, 384, 1, 1),
    SweepSite("k384-2clips", 5, 5, -1, 768, 256, 256, 384, 1, 1),     # two tiles, one clip each: the gate row follows the tile
    SweepSite("tall0", 6, -1, 0, 1024, 12288, 64, 256, None, 1),
    SweepSite("tall1", 6, -1, 1, 1024, 12288, 64, 256, None, 1),
    SweepSite("splitk-k128", 0, -1, -1, 200, 256, 512, 100, 2, 2),
    SweepSite("splitk-k256ring", 1, -1, -1, 512, 12288, 2048, 300, None, 2),
    SweepSite("splitk-k256two", 1, 4, -1, 512, 12288, 2048, 300, None, 2),
    SweepSite("splitk-tall0", 6, -1, 0, 512, 4096, 4096, 256, None, 4),
    SweepSite("splitk-tall1", 6, -1, 1, 512, 4096, 4096, 256, None, 4),
)
SITE_BY_NAME = {s.name: s for s in GEMM_SITES}


def site_clips(s):
    return -(-s.M // s.rpb)


def k_of_n(N, K):
    """k(n): the column of A that weight row n selects.  K <= N: every column is used, rotated from one K-wide column group to the
    next (values repeat across column tiles).  K > N: row n owns the K / N columns from n K / N on and selects one of them."""
    n = torch.arange(N)
    if K <= N:
        return (n + 17 * (n // K)) % K
    r = K // N
    assert K % N == 0 and r <= 64
    return n * r + (7 * n) % r


def carrier(s, launch=0):
    """(a [M, K] bf16, w [N, K] bf16 of zeros and ones, intended [M, N] int64 bits) of launch `launch` of site s: the used columns
    of A hold the sweep in order (wrapping), the unused ones finite random bf16 that meet zero weights.  Built once per shape and
    launch and shared: read-only."""
    return _carrier(s.M, s.N, s.K, launch)


@functools.lru_cache(maxsize=2)
def _carrier(M, N, K, launch):
    kn = k_of_n(N, K)
    used = torch.unique(kn)
    assert all(bool(((kn >= k0) & (kn < k0 + 64)).any()) for k0 in range(0, K, 64)), "a one in every 64-wide K step (and slice)"
    sw = sweep_values()
    slot = torch.arange(M).view(M, 1) * used.numel() + torch.arange(used.numel()).view(1, -1) + launch * M * used.numel()
    g = torch.Generator(device="cpu").manual_seed(4242 + launch)
    a_bits = sw[torch.randint(0, N_FINITE, (M, K), generator=g)]
    a_bits[:, used] = sw[slot % N_FINITE]
    w = torch.zeros((N, K), dtype=BF)
    w[torch.arange(N), kn] = 1.0
    return bf16_of_bits(a_bits), w, a_bits[:, kn]


def site_launches(s):
    """How many launches the 65 280 values need at site s."""
    return -(-N_FINITE // (s.M * min(s.N, s.K)))


@functools.lru_cache(maxsize=1)
def gate_values():
    """256 bf16 gate values: both signs, exponents 2^-20 .. 2^20 (every one of them in the first 41 entries with alternating signs,
    the two ends once more with the other sign), the rest within 2^-2 .. 2^2 so that few products leave fp32's normal range - a
    value sweep meets every exponent, so a gate 2^e alone excludes |e| / 254 of its column; mantissas cycle through the pattern
    classes (zero, all ones, one high bit, one low bit, alternating either way, low half, both ends) and pseudo-random ones."""
    classes = (0x00, 0x7F, 0x40, 0x01, 0x55, 0x2A, 0x0F, 0x41)
    bits = []
    for i in range(256):
        if i < 41:
            e, sign = i - 20, i & 1
        elif i < 43:
            e, sign = (-20, 20)[i - 41], 1
        else:
            e, sign = i % 5 - 2, (i // 5) & 1
        man = classes[i % 8] if i % 3 else (i * 37 + 11) % 128
        bits.append((sign << 15) | ((e + 127) << 7) | man)
    return bf16_of_bits(torch.tensor(bits))


def gate_rows_of(s):
    """gate [clips, N] bf16: column n of clip b holds gate value (n + 97 b) % 256 - another row for every clip."""
    gv = gate_values()
    n = torch.arange(s.N).view(1, -1)
    b = torch.arange(site_clips(s)).view(-1, 1)
    return gv[(n + 97 * b) % 256]


def residual_of(s, launch=0):
    """[M, N] bf16, seeded: an eighth exact zeros (+0), else a random sign, a magnitude 2^-20 .. 2^20 and a random mantissa."""
    g = torch.Generator(device="cpu").manual_seed(977 + 13 * s.M + s.N + launch)
    shape = (s.M, s.N)
    bits = (torch.randint(0, 2, shape, generator=g) << 15) | (torch.randint(107, 148, shape, generator=g) << 7) | \
        torch.randint(0, 128, shape, generator=g)
    bits[torch.randint(0, 8, shape, generator=g) == 0] = 0
    return bf16_of_bits(bits)


def expand_gate(gate, M, rpb):
    """gate [clips, N] -> [M, N]: the gate row of every output row."""
    return gate[torch.arange(M, device=gate.device) // rpb]


# ------------------------------------------------------------------------------------------------ MXFP8 carrier
# Every bf16 value v with 2^-8 <= |v| < 16 (12 binades x 128 mantissas x 2 signs = 3072 values) split as hi + lo: hi = the top four
# significant bits (an e4m3 element 8 .. 15 under the block scale 2^(e - 3)), lo = the next four (an element 0 .. 15 under 2^(e - 7)),
# in two neighbouring 32-wide K blocks; the weight row has 1.0 at both columns, so acc = hi + lo = v exactly.
MX_M, MX_N, MX_K, MX_RPB = 768, 256, 256, 256
MxCarrier = namedtuple("MxCarrier", "aq sa wq sw intended")


@functools.lru_cache(maxsize=1)
def mx_carrier():
    """aq [768, 256] e4m3, sa [768, 8] uint8 (E8M0), wq [256, 256] e4m3, sw [256, 8], intended [768, 256] int64 bf16 bits.  Row m
    holds four values, one per pair of K blocks p: hi at column 64 p + j(p), lo at 64 p + 32 + j(p), every other element zero;
    weight row n selects pair (n + n / 4) % 4."""
    b = _all_bits()
    ex = ((b >> 7) & 0xFF) - 127
    vals = b[(ex >= -8) & (ex <= 3)]
    g = torch.Generator(device="cpu").manual_seed(3072)
    vals = vals[torch.randperm(vals.numel(), generator=g)]
    pairs = MX_K // 64
    assert vals.numel() == MX_M * pairs == 3072
    vals = vals.view(MX_M, pairs)
    e = ((vals >> 7) & 0xFF) - 127
    sig = 128 + (vals & 0x7F)                                         # 8 significant bits
    sign = 1.0 - 2.0 * (vals >> 15).float()
    hi, lo = (sig >> 4).float() * sign, (sig & 15).float() * sign
    j = (5 * torch.arange(pairs) + 3) % 32
    a = torch.zeros((MX_M, MX_K))
    sa = torch.zeros((MX_M, MX_K // 32), dtype=torch.int64)
    for p in range(pairs):
        a[:, 64 * p + j[p]] = hi[:, p]
        a[:, 64 * p + 32 + j[p]] = lo[:, p]
        sa[:, 2 * p] = e[:, p] - 3 + 127
        sa[:, 2 * p + 1] = e[:, p] - 7 + 127
    n = torch.arange(MX_N)
    pn = (n + n // 4) % pairs
    w = torch.zeros((MX_N, MX_K))
    w[n, 64 * pn + j[pn]] = 1.0
    w[n, 64 * pn + 32 + j[pn]] = 1.0
    aq, wq = a.to(torch.float8_e4m3fn), w.to(torch.float8_e4m3fn)
    assert torch.equal(aq.float(), a) and torch.equal(wq.float(), w), "the elements are exact in e4m3"
    sw = torch.full((MX_N, MX_K // 32), 127, dtype=torch.uint8)
    return MxCarrier(aq, sa.to(torch.uint8), wq, sw, vals[:, pn])
