"""fp64 references, comparators, guard bands, case grids and plain-torch stand-ins for the DiT kernel tests
(tests/test_dit_kernel_edges_gpu.py on the GPU, tests/test_dit_refs_cpu.py for the proof that the bounds bite; the comparators
are also what tests/test_kernels_gpu.py imports).  Nothing here touches the GPU: inputs are built on the CPU from a seed,
references are computed from the bf16 inputs with the kernels' DOCUMENTED rounding points, and the stand-ins (with optional
mutations) exist to show that every bound passes a correct bf16 implementation at every GRID_* case and fails a subtly wrong one.
The GRID_* lists are iterated by both modules: what is proven on the CPU is exactly what runs on the GPU.
GRID_GEMM_BLOCKED (the slab GEMM of the sequence-parallel exchange, operands in column planes) is shared in the same way by
tests/test_sp_slab_kernels_gpu.py and tests/test_sp_slab_refs_cpu.py."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle import dit_oracle as O

BF = torch.bfloat16
F64 = torch.float64
EPI_NONE, EPI_GELU, EPI_GATE_RES = 0, 1, 2


# ------------------------------------------------------------------------------------------------ comparators
def ulp_diff_ok(out, ref, max_ulp=1, frac_exact=0.98, atol_rel=2e-3, mag=None):
    """out, ref bf16: |out-ref| <= max_ulp bf16 ulps + atol_rel * rms(ref) (cancellation near zero), most exactly equal.
    `mag`: magnitude of the terms the result was summed from (a residual add cancels: the ulp that matters is the terms')."""
    o, r = out.float(), ref.float()
    ulp = torch.maximum(r.abs(), o.abs()) * 2.0 ** -7
    if mag is not None:
        ulp = torch.maximum(ulp, mag.float() * 2.0 ** -7)
    atol = atol_rel * r.pow(2).mean().sqrt()
    bad = ((o - r).abs() > max_ulp * ulp + atol).sum().item()
    exact = (out == ref).float().mean().item()
    return bad == 0 and exact >= frac_exact, f"bad={bad} exact={exact:.5f}"


def _attn_ref(q, k, v, heads):
    B, Sq, HD = q.shape
    qh = q.float().view(B, Sq, heads, 128).transpose(1, 2)
    kh = k.float().view(B, -1, heads, 128).transpose(1, 2)
    vh = v.float().view(B, -1, heads, 128).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(128)
    p = torch.softmax(s, -1)
    o = p @ vh
    _attn_ref.mag = ((p * p) @ (vh * vh)).sqrt().transpose(1, 2).reshape(B, Sq, HD)    # |terms| the output was summed from
    return o.transpose(1, 2).reshape(B, Sq, HD)


# Measured on MI355X (round 2, printed by every test below): rel-L2 against the fp32 answer 2.4e-3 .. 2.9e-3 - bf16 output
# rounding alone is 1.7e-3 (uniform relative error of 2^-9 / sqrt 3 ... 2^-8 / sqrt 3), the rest is P rounded to bf16 for the PV
# MFMA (the reference's SDPA does the same); against the fp32 answer ROUNDED to bf16: <= 2 bf16 ulp everywhere.
ATTN_REL_L2 = 3.6e-3          # 1.25 x the largest measured value


def _attn_check(out, ref, tag, rel=ATTN_REL_L2, max_ulp=2, frac_exact=0.5):
    """out bf16 vs fp32 reference (call right after _attn_ref): rel-L2, and distance to the reference rounded to bf16 in bf16
    ulps of max(|o|, sqrt(sum_k p_k^2 v_k^2)) - the output is a sum of terms p_k v_k with P rounded to bf16 for the PV product
    (as in the reference's SDPA), so where the terms cancel the rounding error scales with the terms, not with the sum."""
    e = rel_l2(out, ref)
    r16 = ref.to(BF)
    mag = _attn_ref.mag.to(out.device)
    o, r = out.float(), r16.float()
    ulp = torch.maximum(torch.maximum(r.abs(), o.abs()), mag) * 2.0 ** -7
    worst = (o - r).abs() / ulp.clamp_min(1e-30)
    exact = (out == r16).float().mean().item()
    print(f"attention {tag}: rel-L2 {e:.3e}  max|diff| {(o - ref.float()).abs().max().item():.3e}  worst {worst.max().item():.2f} ulp  "
          f"exact {exact:.4f}")
    assert e < rel, (tag, e)
    ok, msg = ulp_diff_ok(out, r16, max_ulp=max_ulp, frac_exact=frac_exact, atol_rel=0.0, mag=mag)
    assert ok, (tag, msg)


def figures(out, ref, mag=None, atol_rel=2e-3):
    """The `dit-kernel-edge` figures of one case: worst distance in bf16 ulps (of max(|out|, |ref|, mag), after the comparator's
    absolute allowance), share of bit-equal elements, rel-L2 against `ref`.  Reporting only: the assertion is ulp_diff_ok's."""
    o, r = out.double().cpu(), ref.to(BF).double().cpu()
    ulp = torch.maximum(o.abs(), r.abs())
    if mag is not None:
        ulp = torch.maximum(ulp, mag.double().cpu())
    atol = atol_rel * r.pow(2).mean().sqrt()
    worst = (((o - r).abs() - atol).clamp_min(0) / (ulp * 2.0 ** -7).clamp_min(1e-300)).max().item() if o.numel() else 0.0
    return f"worst {worst:.2f} ulp  exact {(o == r).double().mean().item():.5f}  rel-L2 {rel_l2(out.cpu(), ref.cpu()):.3e}"


def rnd(shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF)


# ------------------------------------------------------------------------------------------------ guard bands
# A bf16 quiet NaN with a payload: no kernel produces these bits, and a kernel that READS one poisons its result.
SENTINEL = 0x7FE5
SENTINEL_U8 = 0xA5


def _fill(n, device, dtype):
    if dtype == torch.uint8:
        return torch.full((n,), SENTINEL_U8, dtype=torch.uint8, device=device)
    assert dtype == BF
    return torch.full((n,), SENTINEL, dtype=torch.int16, device=device).view(BF)


def _bits(t):
    return t if t.dtype == torch.uint8 else t.view(torch.int16)


def guarded(rows, cols, ld, pad_rows, device, batches=1, batch_gap=0, dtype=BF):
    """ONE allocation filled with the sentinel: pad_rows rows of ld elements, then `batches` windows of rows x cols with row stride
    ld, each followed by batch_gap elements, then pad_rows rows again.  Returns (buffer, view): view is the [batches,] rows x cols
    window (the batch dimension only when batches > 1).  Everything a kernel may touch lies inside the allocation; a store outside
    the window is found by assert_guard_intact, never by a fault."""
    assert ld >= cols and pad_rows >= 1 and batch_gap >= 0
    per = rows * ld + batch_gap
    buf = _fill(2 * pad_rows * ld + batches * per, device, dtype)
    if batches > 1:
        view = torch.as_strided(buf, (batches, rows, cols), (per, ld, 1), pad_rows * ld)
    else:
        view = torch.as_strided(buf, (rows, cols), (ld, 1), pad_rows * ld)
    return buf, view


def assert_guard_intact(buffer, view):
    """Every element of `buffer` outside the `view` window still holds the sentinel bits."""
    inside = torch.zeros(buffer.numel(), dtype=torch.bool, device=buffer.device)
    torch.as_strided(inside, view.shape, view.stride(), view.storage_offset() - buffer.storage_offset()).fill_(True)
    want = SENTINEL_U8 if buffer.dtype == torch.uint8 else SENTINEL
    hit = ((_bits(buffer) != want) & ~inside).nonzero().flatten()
    assert hit.numel() == 0, (f"{hit.numel()} elements outside the window were written; first flat offsets {hit[:8].tolist()} "
                              f"(window starts at {view.storage_offset() - buffer.storage_offset()}, strides {view.stride()})")


def is_sentinel(t):
    return _bits(t) == (SENTINEL_U8 if t.dtype == torch.uint8 else SENTINEL)


def store_standin(buffer, view, value, mutant=None):
    """What a kernel's store does to a guarded window; the mutants write a little more than the window."""
    view.copy_(value)
    off = view.storage_offset() - buffer.storage_offset()
    st = view.stride()
    flat = buffer.view(-1)
    if mutant == "row_past_M":                         # one row stored past the last
        last = (view.shape[0] - 1) * st[0] if view.dim() == 3 else 0
        flat[off + last + view.shape[-2] * st[-2]:][:view.shape[-1]] = 1.0
    elif mutant == "cols_past_N":                      # 8 columns stored past N, on one row
        flat[off + (view.shape[-2] // 2) * st[-2] + view.shape[-1]:][:8] = 1.0
    elif mutant == "batch_gap":                        # clip 1 stored at clip 0's end (the batch stride ignored)
        assert view.dim() == 3
        flat[off + view.shape[1] * st[1]:][:8] = 1.0
    else:
        assert mutant is None, mutant


# ------------------------------------------------------------------------------------------------ GEMM
GEMM_TILE_ROWS = {0: 128, 1: 256, 2: 144, -1: 128}     # csrc/gemm.hip BM, gemm256s.hip TB, gemm144.hip TM; automatic dispatch
#                                                         takes the 128-row kernel at N = 256 (gemm_pick_tile: N / 256 tiles per
#                                                         tile row never fill 3/4 of a round at these M)
# what ulp_diff_ok is given per epilogue: the bounds tests/test_kernels_gpu.py states (test_gemm_plain; test_gemm256_kernel)
GEMM_BOUND = {EPI_NONE: dict(max_ulp=1, frac_exact=0.98), EPI_GELU: dict(max_ulp=2, frac_exact=0.97),
              EPI_GATE_RES: dict(max_ulp=2, frac_exact=0.97)}

# path: "tile" = drn_gemm_bf16 with drn_gemm_force_tile(tile) (-1 = automatic); "splitk" = drn_gemm_bf16_splitk(splits);
# "tall0" / "tall1" = drn_gemm_tall_force_shape(0 / 1) under automatic dispatch; "batched" = automatic dispatch, clips compared
# with the clip alone.  strided: lda = K + 64, ldc = N + 64, ldr = N + 128, residual in its own window; else contiguous.
# alias: the residual IS the output window.  rpb: rows per clip (gate rows = ceil(M / rpb)).
GemmCase = namedtuple("GemmCase", "path tile M N K epi strided alias rpb splits seed")


def _gemm_grid():
    cases, seed = [], 1000
    ks = (64, 128, 192, 4096)                          # 1, 2, 3 and 64 K steps of 64
    for tile in (0, 1, 2, -1):
        h = GEMM_TILE_ROWS[tile]
        for i, M in enumerate((h - 1, h, h + 1, 2 * h - 1, 2 * h, 2 * h + 1)):
            for epi in (EPI_NONE, EPI_GELU, EPI_GATE_RES):
                seed += 1
                K = ks[(i + epi + (tile & 3)) % 4]
                # two clips, the boundary inside a tile: ragged (odd M) or even halves
                cases.append(GemmCase("tile", tile, M, 256, K, epi, True, False, (M + 1) // 2, 1, seed))
        # one aliased (in place) case per kernel, three clips, and one contiguous one
        cases.append(GemmCase("tile", tile, 2 * h + 1, 256, 128, EPI_GATE_RES, True, True, (2 * h + 3) // 3, 1, seed + 500))
        cases.append(GemmCase("tile", tile, h + 1, 512, 64, EPI_GATE_RES, False, True, h // 2 + 1, 1, seed + 501))
    # split-K on the 128 x 128 kernel's slices (two clips of 100 rows), all epilogues
    for epi in (EPI_NONE, EPI_GELU, EPI_GATE_RES):
        cases.append(GemmCase("splitk", -1, 200, 256, 512, epi, True, False, 100, 2, 1600 + epi))
    for shape in (0, 1):
        # gemm_tall.hip, K slices (drn_gemm_splitk_choice(256, 4096, 4096) == 4) and unsplit (N / 64 >= 192), two clips of 256 rows
        cases.append(GemmCase(f"tall{shape}", -1, 512, 4096, 4096, EPI_GATE_RES, True, False, 256, 4, 1610 + shape))
        cases.append(GemmCase(f"tall{shape}", -1, 512, 12288, 192, EPI_GATE_RES, True, False, 256, 1, 1620 + shape))
    cases.append(GemmCase("tall0", -1, 512, 12288, 64, EPI_GELU, True, False, 256, 1, 1630))
    # clips stacked along the rows.  4608 x 4096 per clip runs as ONE launch of the 144-row kernel over both clips
    # (drn_gemm_tile_choice(4608, 4096) == 2: no tail split); 9472 x 4096 per clip takes the 256^2 kernel with a tail split
    # (37 x 16 tiles = 2 rounds + 80: 32 tile rows, then 1280 rows on the 128^2 kernel), so every clip gets its own two launches
    cases.append(GemmCase("batched", -1, 2 * 4608, 4096, 128, EPI_GATE_RES, False, True, 4608, 1, 1640))
    cases.append(GemmCase("batched", -1, 2 * 9472, 4096, 128, EPI_GATE_RES, True, False, 9472, 1, 1641))
    return cases


GRID_GEMM = _gemm_grid()


def gemm_id(c):
    return f"{c.path}{c.tile if c.path == 'tile' else ''}-M{c.M}-N{c.N}-K{c.K}-epi{c.epi}-rpb{c.rpb}" + ("-alias" if c.alias else "") + \
           ("" if c.strided else "-contig") + (f"-s{c.splits}" if c.splits > 1 else "")


def gemm_inputs(c):
    """a [M, K], w [N, K], gate [clips, N], residual [M, N] (CPU, contiguous; the GPU test places them in strided windows)."""
    nb = -(-c.M // c.rpb)
    a, w = rnd((c.M, c.K), seed=c.seed), rnd((c.N, c.K), c.K ** -0.5, seed=c.seed + 1)
    gate, res = rnd((nb, c.N), 0.5, seed=c.seed + 2), rnd((c.M, c.N), seed=c.seed + 3)
    return a, w, gate, res


def gemm_ref(a, w, epi, gate=None, residual=None, rows_per_batch=None):
    """fp64 product rounded to bf16, then the bf16 op chain tests/test_kernels_gpu.py uses per epilogue (GELU: torch CPU bf16
    erf-GELU; gated residual: x + gate * lin in bf16 torch ops = two roundings, gate row = row // rows_per_batch).
    Returns (ref bf16, mag): mag = max(|residual|, |gate * lin|) for the gated residual, else None."""
    M = a.shape[0]
    lin = torch.cat([(a[i:i + 4096].double() @ w.double().t()).to(BF) for i in range(0, M, 4096)], 0)
    if epi == EPI_NONE:
        return lin, None
    if epi == EPI_GELU:
        return F.gelu(lin.cpu()).to(lin.device), None
    rpb = rows_per_batch if rows_per_batch else M
    g = gate[torch.arange(M, device=a.device) // rpb] * lin
    return residual + g, torch.maximum(residual.abs(), g.abs())


def gemm_standin(a, w, epi, gate=None, residual=None, rows_per_batch=None, slices=1, tile_rows=128, mutant=None, ldc=None):
    """A correct bf16 GEMM in another summation order: fp32 products of 64-wide K chunks, summed pairwise inside each of `slices`
    K slices, the slices summed in order; then the epilogue's rounding points.  Mutants (gated residual only): "gate_clip_pm1" =
    every row of a tile takes the gate of the tile's FIRST row (the previous clip's gate after a boundary inside the tile),
    "rpb_ignored" = gate row 0 everywhere, "res_ldc" = the residual read with row stride ldc instead of its own."""
    M, K = a.shape
    a32, w32 = a.float(), w.float()
    parts = [a32[:, k:k + 64] @ w32[:, k:k + 64].t() for k in range(0, K, 64)]
    slices = max(1, min(slices, len(parts)))
    per = -(-len(parts) // slices)

    def tree(xs):
        while len(xs) > 1:
            xs = [xs[i] + xs[i + 1] if i + 1 < len(xs) else xs[i] for i in range(0, len(xs), 2)]
        return xs[0]

    acc = None
    for s in range(0, len(parts), per):
        t = tree(parts[s:s + per])
        acc = t if acc is None else acc + t
    lin = acc.to(BF)
    if epi == EPI_NONE:
        return lin
    if epi == EPI_GELU:
        return F.gelu(lin)
    rpb = rows_per_batch if rows_per_batch else M
    rows = torch.arange(M)
    if mutant == "gate_clip_pm1":
        rows = rows // tile_rows * tile_rows
    elif mutant == "rpb_ignored":
        rows = rows * 0
    if mutant == "res_ldc":
        residual = residual.as_strided(residual.shape, (ldc, 1))
    else:
        assert mutant in (None, "gate_clip_pm1", "rpb_ignored"), mutant
    g = (gate[rows // rpb].float() * lin.float()).to(BF)
    return (residual.float() + g.float()).to(BF)


# ------------------------------------------------------------------------------------------------ attention
# q / k / v are column blocks of ONE packed [B, max(Sq, Sk), 3 H 128 + 64] buffer (the fused QKV GEMM's output layout with a padded
# row); rows past Sq / Sk and the 64 pad columns hold the NaN sentinel.  ns = requested key splits (1 = drn_attention_bf16).
AttnCase = namedtuple("AttnCase", "B H Sq Sk scale ns seed")
_S0 = 1.0 / math.sqrt(128)
GRID_ATTN = (
    # Sk across one 64-key tile's edges at Sq = 129, Sq across the 128-row block's edges at Sk = 65, and corners
    [AttnCase(2 + i % 2, 1 + i % 2, 129, Sk, None if i % 2 else 0.05, 1, 2000 + i) for i, Sk in enumerate((1, 8, 63, 64, 65, 129))] +
    [AttnCase(3 - i % 2, 2 - i % 2, Sq, 65, None if i % 2 else 0.11, 1, 2010 + i) for i, Sq in enumerate((1, 127, 128, 257))] +
    [AttnCase(2, 1, 1, 1, None, 1, 2020), AttnCase(3, 2, 257, 1, 0.07, 1, 2021), AttnCase(2, 2, 1, 129, 0.06, 1, 2022),
     AttnCase(3, 1, 257, 129, None, 1, 2023), AttnCase(2, 1, 127, 63, 0.12, 1, 2024), AttnCase(2, 2, 128, 64, None, 1, 2025),
     AttnCase(2, 1, 128, 8, 0.09, 1, 2026), AttnCase(3, 1, 127, 129, 0.04, 1, 2027)] +
    # split keys: 77 keys in 4 requested chunks run as 2 (no empty chunk); B > 1; 641 keys in 4 chunks of 192 (the last holds 65)
    [AttnCase(1, 2, 129, 77, None, 4, 2030), AttnCase(2, 2, 129, 77, 0.07, 4, 2031), AttnCase(3, 1, 257, 300, None, 2, 2032),
     AttnCase(2, 2, 128, 641, 0.1, 4, 2033)])


def attn_id(c):
    return f"B{c.B}-H{c.H}-Sq{c.Sq}-Sk{c.Sk}-scale{'def' if c.scale is None else c.scale}-ns{c.ns}"


def attn_packed(c):
    """The packed input buffer [B, Smax, 3 H 128 + 64] (CPU) with the sentinel wherever no operand lives."""
    HD, S = c.H * 128, max(c.Sq, c.Sk)
    buf = _fill(c.B * S * (3 * HD + 64), "cpu", BF).view(c.B, S, 3 * HD + 64)
    buf[:, :c.Sq, :HD] = rnd((c.B, c.Sq, HD), seed=c.seed)
    buf[:, :c.Sk, HD:2 * HD] = rnd((c.B, c.Sk, HD), seed=c.seed + 1)
    buf[:, :c.Sk, 2 * HD:3 * HD] = rnd((c.B, c.Sk, HD), seed=c.seed + 2)
    return buf


def attn_views(buf, c):
    HD = c.H * 128
    return buf[:, :c.Sq, :HD], buf[:, :c.Sk, HD:2 * HD], buf[:, :c.Sk, 2 * HD:3 * HD]


def attention_ref(q, k, v, heads, scale=None):
    """fp64 softmax(scale q k^T) v for q [B, Sq, H 128], k / v [B, Sk, H 128] (any strides).  Returns (o, mag), both [B, Sq, H 128]
    fp64: mag = sqrt(sum_k p_k^2 v_k^2), the magnitude of the terms (what _attn_ref leaves in _attn_ref.mag, where this also puts
    it so that _attn_check can follow directly)."""
    B, Sq, HD = q.shape
    scale = _S0 if scale is None else scale
    qh = q.double().reshape(B, Sq, heads, 128).transpose(1, 2)
    kh = k.double().reshape(B, -1, heads, 128).transpose(1, 2)
    vh = v.double().reshape(B, -1, heads, 128).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1)
    o = (p @ vh).transpose(1, 2).reshape(B, Sq, HD)
    mag = ((p * p) @ (vh * vh)).sqrt().transpose(1, 2).reshape(B, Sq, HD)
    _attn_ref.mag = mag
    return o, mag


def attn_splits(Sk, ns):
    """(keys per chunk, effective chunk count) as the launcher derives them: whole 64-key tiles, no empty chunk."""
    if ns <= 1:
        return Sk, 1
    chunk = -(-(-(-Sk // ns)) // 64) * 64
    return chunk, -(-Sk // chunk)


def attention_standin(q, k, v, heads, scale=None, ns=1, mutant=None):
    """A correct bf16 attention the way a flash kernel forms it: fp32 online softmax over 64-key tiles, P rounded to bf16 for the
    PV product, one division at the end; with ns > 1 per-chunk partials (m, l, acc) merged by a combine step.
    Mutants: "kv_clip0" = clip 0's K / V for every clip (batch stride ignored), "scale_default" = 1 / sqrt(128) whatever the
    caller passed, "drop_last_key" = the last key dropped when Sk % 64 == 1, "combine_requested" = the combine step merges the
    REQUESTED number of chunks although fewer were written (it reads stale workspace: m = 0, l = 1, acc = 1)."""
    assert mutant in (None, "kv_clip0", "scale_default", "drop_last_key", "combine_requested"), mutant
    B, Sq, HD = q.shape
    Sk = k.shape[1]
    scale = _S0 if (scale is None or mutant == "scale_default") else scale
    if mutant == "kv_clip0":
        k, v = k[:1].expand(B, -1, -1), v[:1].expand(B, -1, -1)
    if mutant == "drop_last_key" and Sk % 64 == 1 and Sk > 1:
        Sk -= 1
    qh = q.float().reshape(B, Sq, heads, 128).transpose(1, 2)
    kh = k.float().reshape(B, -1, heads, 128).transpose(1, 2)[:, :, :Sk]
    vh = v.float().reshape(B, -1, heads, 128).transpose(1, 2)[:, :, :Sk]
    sl2 = scale * 1.4426950408889634
    chunk, n_eff = attn_splits(Sk, ns)
    partials = []
    for s in range(n_eff):
        m = torch.full((B, heads, Sq, 1), -math.inf)
        l = torch.zeros((B, heads, Sq, 1))
        acc = torch.zeros((B, heads, Sq, 128))
        for t0 in range(s * chunk, min((s + 1) * chunk, Sk), 64):
            t1 = min(t0 + 64, (s + 1) * chunk, Sk)
            sc = qh @ kh[:, :, t0:t1].transpose(-1, -2)
            m_new = torch.maximum(m, sc.max(-1, keepdim=True).values)
            p = torch.exp2((sc - m_new) * sl2)
            alpha = torch.exp2((m - m_new) * sl2)
            l = l * alpha + p.sum(-1, keepdim=True)
            acc = acc * alpha + p.to(BF).float() @ vh[:, :, t0:t1]
            m = m_new
        partials.append((m, l, acc))
    if ns <= 1:
        o = partials[0][2] / partials[0][1]
    else:
        if mutant == "combine_requested":
            partials += [(torch.zeros_like(m), torch.ones_like(l), torch.ones_like(acc))] * (ns - n_eff)
        mmax = torch.stack([p_[0] for p_ in partials]).max(0).values
        den = sum(torch.exp2((m_ - mmax) * sl2) * l_ for m_, l_, _ in partials)
        o = sum(torch.exp2((m_ - mmax) * sl2) * a_ for m_, _, a_ in partials) / den
    return o.transpose(1, 2).reshape(B, Sq, HD).to(BF)


# ------------------------------------------------------------------------------------------------ q/k RMSNorm + RoPE
# clips x tpb tokens; table row = pos + tok % tpb.  which: "qk" | "q" | "k"; rope False = cos = sin = NULL.
# layout "packed": q | k | v are column blocks of one [tokens, 3 D] window with a padded row (ldq == ldk = 3 D + 64);
# "split": q and k in windows of their own with ldq = D + 64 != ldk = D + 128.
# exact: q / k hold multiples of 1/4 in [-3, 3], so the sum of 128 squares is exact in fp32 in EVERY summation order and the
# normalised value has one correct bf16 rounding.  With random data two correct fp32 kernels differ in the last bit of the mean
# square, which flips the bf16 rounding of about 4 normalised values per million; where RoPE's two terms then cancel, that one
# ulp of a term is several ulps of the result and counts as bad (measured on the CPU with the kernel's own summation order, the
# "kernel" stand-in below: 1 bad in 69 120 at clips3-tpb20-h9, 12 in 18.9 M at 4608 tokens x 32 heads).  The cases where a correct
# stand-in fails that way get exact inputs, as the rule for this grid says; the bound stays.
RopeCase = namedtuple("RopeCase", "clips tpb pos heads which rope layout seed exact", defaults=(False,))
GRID_ROPE = [
    RopeCase(2, 37, 0, 8, "qk", True, "packed", 3000), RopeCase(3, 20, 0, 9, "qk", True, "split", 3001, True),
    RopeCase(1, 50, 13, 12, "qk", True, "packed", 3002), RopeCase(2, 33, 7, 1, "qk", True, "split", 3003),
    RopeCase(3, 16, 5, 32, "qk", True, "packed", 3004), RopeCase(2, 40, 3, 9, "q", True, "split", 3005),
    RopeCase(3, 25, 11, 12, "k", True, "split", 3006), RopeCase(2, 30, 0, 8, "qk", False, "split", 3007),
    RopeCase(1, 1, 0, 1, "k", True, "split", 3008), RopeCase(2, 19, 4, 12, "q", False, "packed", 3009),
    # 4608 tokens x 4 head groups x 2 tensors = 36 864 work items > 32 768 (8192 blocks of 4 waves): the grid-stride loop
    RopeCase(2, 2304, 9, 32, "qk", True, "packed", 3010, True),
    # the same loop with RANDOM inputs, so that the summation order of the mean square counts there too: one head (7 of a wave's 8
    # head rows idle), 16 400 tokens x 2 tensors = 32 800 work items.  Of the seeds 3011 .. 3039 both stand-ins pass at 3016,
    # 3018, 3028 and 3033 (the others show 1 .. 4 of the rounding flips described above in 4.2 M elements); the first is taken
    RopeCase(2, 8200, 9, 1, "qk", True, "split", 3016),
]
ROPE_BOUND = dict(max_ulp=1, frac_exact=0.99)             # test_qk_norm_rope_matches_oracle


def rope_id(c):
    return f"clips{c.clips}-tpb{c.tpb}-pos{c.pos}-h{c.heads}-{c.which}-{'rope' if c.rope else 'norope'}-{c.layout}" + ("-exact" if c.exact else "")


def rope_inputs(c):
    """qkv [tokens, 3 D], wq, wk [128], cos, sin [pos + tokens + 1, 128] (rows past pos + tpb exist so that a wrong row index
    reads defined, different values), all bf16 on the CPU."""
    tokens, D = c.clips * c.tpb, c.heads * 128
    qkv = rnd((tokens, 3 * D), 1.5, seed=c.seed)
    if c.exact:
        g = torch.Generator().manual_seed(c.seed)
        qkv = (torch.randint(-12, 13, (tokens, 3 * D), generator=g).float() / 4).to(BF)
    wq, wk = 1 + 0.1 * rnd((128,), seed=c.seed + 1), 1 + 0.1 * rnd((128,), seed=c.seed + 2)
    g = torch.Generator().manual_seed(c.seed + 3)
    half = torch.rand((c.pos + tokens + 1, 64), generator=g) * (2 * math.pi)
    ang = torch.cat([half, half], 1).to(BF)
    cos, sin = O.rope_cos_sin(ang, BF)
    return qkv, wq, wk, cos, sin


def qk_norm_rope_ref(x, w, cos, sin, heads, tokens_per_batch=None, pos_offset=0):
    """x [tokens, heads 128] bf16 -> per-head RMSNorm then RoPE with table row pos_offset + tok % tokens_per_batch, in the
    oracle's ops (oracle.dit_oracle.rms_norm / apply_rope: the reference's rounding points).  cos = None: no RoPE."""
    tokens = x.shape[0]
    tpb = tokens_per_batch if tokens_per_batch else max(tokens, 1)
    t = O.rms_norm(x.reshape(tokens, 1, heads, 128), w)
    if cos is not None:
        rows = pos_offset + torch.arange(tokens) % tpb
        t = O.apply_rope(t, cos[rows], sin[rows])
    return t.reshape(tokens, heads * 128)


def _fma32(a, b, c):
    """fp32 fma(a, b, c): the product is exact in fp64, one rounding of the sum back to fp32."""
    return (a.double() * b.double() + c.double()).float()


def qk_norm_rope_standin(x, w, cos, sin, heads, tokens_per_batch=None, pos_offset=0, mutant=None, order="torch"):
    """The same in fp32 with the kernel's rounding points.  order "torch": the mean square as torch sums it; "kernel": as
    csrc/elementwise.hip sums it (8 lanes per head row, each an fma chain over its 8 low and 8 high elements, then a butterfly
    over the lanes) - another correct fp32 order.  Mutants: "tok_row" = table row pos + tok (no % tokens_per_batch),
    "pos_dropped" = row tok % tpb, "pos_off1" = row pos + 1 + tok % tpb."""
    assert mutant in (None, "tok_row", "pos_dropped", "pos_off1") and order in ("torch", "kernel"), (mutant, order)
    tokens = x.shape[0]
    tpb = tokens_per_batch if tokens_per_batch else max(tokens, 1)
    xf = x.float().reshape(tokens, heads, 128)
    if order == "kernel":
        lo, hi = xf[..., :64].reshape(tokens, heads, 8, 8), xf[..., 64:].reshape(tokens, heads, 8, 8)
        ssq = torch.zeros(tokens, heads, 8)
        for part in (lo, hi):
            for i in range(8):
                ssq = _fma32(part[..., i], part[..., i], ssq)
        for o in (1, 2, 4):
            ssq = ssq + ssq[..., torch.arange(8) ^ o]
        ssq = ssq[..., :1]
    else:
        ssq = xf.pow(2).sum(-1, keepdim=True)
    rinv = 1.0 / torch.sqrt(ssq / 128.0 + 1e-6)
    n = ((xf * rinv) * w.float()).to(BF).float()
    if cos is not None:
        tok = torch.arange(tokens)
        rows = {None: pos_offset + tok % tpb, "tok_row": pos_offset + tok, "pos_dropped": tok % tpb,
                "pos_off1": pos_offset + 1 + tok % tpb}[mutant]
        c, s = cos[rows].float()[:, None, :], sin[rows].float()[:, None, :]
        rot = torch.cat((-n[..., 64:], n[..., :64]), -1)
        n = ((n * c).to(BF).float() + (rot * s).to(BF).float())
    return n.to(BF).reshape(tokens, heads * 128)


# ------------------------------------------------------------------------------------------------ LayerNorm + modulate, broadcast add
# rows in all, split over 3 clips of ceil(rows / 3) rows (the last one shorter or absent); shift / scale / add_vec: [3, D]
LnCase = namedtuple("LnCase", "rows D with_add seed")
# (257 rows x 8192 is left out: over 2.1 M elements the 1-ulp bound with its 2e-3 rms allowance is marginal for ANY correct fp32
#  LayerNorm - each rounding flip of the normalised value next to a cancelling shift counts as bad, and the fp32 stand-in of
#  tests/test_dit_refs_cpu.py shows 3 such elements there; 257 rows run at D <= 1032 and D = 8192 at rows <= 5)
GRID_LN = [LnCase(rows, D, add, 4000 + 100 * add + 10 * i + j) for i, rows in enumerate((1, 3, 4, 5, 257))
           for j, D in enumerate((8, 264, 1032, 8192)) for add in (False, True)
           if not (rows == 257 and D == 8192) and (add == bool((i + j) % 2) or (rows in (1, 5, 257) and D != 264))]
LN_BOUND = dict(max_ulp=1, frac_exact=0.995)              # test_ln_modulate_matches_oracle
LN_CLIPS = 3


def ln_id(c):
    return f"rows{c.rows}-D{c.D}-{'add' if c.with_add else 'noadd'}"


def ln_rpb(c):
    return -(-c.rows // LN_CLIPS)


def ln_inputs(c):
    x = rnd((c.rows, c.D), 2.0, seed=c.seed)
    shift, scale = rnd((LN_CLIPS, c.D), 0.7, seed=c.seed + 1), rnd((LN_CLIPS, c.D), 0.7, seed=c.seed + 2)
    add = rnd((LN_CLIPS, c.D), 0.5, seed=c.seed + 3) if c.with_add else None
    return x, shift, scale, add


def ln_modulate_ref(x, shift, scale, add_vec=None, rows_per_batch=None):
    """(x after the broadcast add, h): x <- x + add_vec[row // rpb] in bf16; h = oracle.modulate(F.layer_norm(x, eps 1e-6), shift
    row, scale row) in bf16 torch ops, as the existing tests form it."""
    rows, D = x.shape
    b = torch.arange(rows) // (rows_per_batch if rows_per_batch else max(rows, 1))
    if add_vec is not None:
        x = x + add_vec[b]
    n = F.layer_norm(x.unsqueeze(0), (D,), eps=1e-6)
    return x, O.modulate(n, shift[b], scale[b]).squeeze(0)


def _ln_kernel_stats(xf):
    """Row mean and variance summed as csrc/elementwise.hip sums them: lane l of chunk i owns columns 8 (l + 64 i) .. + 7 (8 adds,
    then an fma chain for the squares), chunks grouped in four, a 64-lane butterfly per group, (g0 + g1) + (g2 + g3)."""
    rows, D = xf.shape
    nch = next(n for n in (1, 2, 4, 8, 16) if n * 512 >= D)
    lanes = torch.zeros(rows, nch * 512)
    lanes[:, :D] = xf
    live = torch.zeros(rows, nch * 512)
    live[:, :D] = 1.0
    lanes, live = lanes.reshape(rows, nch, 64, 8), live.reshape(rows, nch, 64, 8)

    def tree(part):                                    # part [rows, nch, 64]
        groups = [part[:, i:i + max(nch // 4, 1)] for i in range(0, nch, max(nch // 4, 1))] if nch >= 4 else [part]
        outs = []
        for g in groups:
            t = torch.zeros_like(g[:, 0])
            for i in range(g.shape[1]):
                t = t + g[:, i]
            for o in (32, 16, 8, 4, 2, 1):
                t = t + t[:, torch.arange(64) ^ o]
            outs.append(t[:, 0])
        return (outs[0] + outs[1]) + (outs[2] + outs[3]) if nch >= 4 else outs[0]

    s = torch.zeros(rows, nch, 64)
    for j in range(8):
        s = s + lanes[..., j]
    mean = (tree(s) / D).reshape(rows, 1)
    d = (lanes - mean[:, :, None, None]) * live
    q = torch.zeros(rows, nch, 64)
    for j in range(8):
        q = _fma32(d[..., j], d[..., j], q)
    return mean, (tree(q) / D).reshape(rows, 1)


def ln_modulate_standin(x, shift, scale, add_vec=None, rows_per_batch=None, mutant=None, order="torch"):
    """fp32 LayerNorm (two-pass variance) with the kernel's rounding points; order "torch": the sums as torch forms them,
    "kernel": the kernels' summation tree (another correct fp32 order).  Mutants: "clip_pm1" = each block of four rows takes
    the clip of its first row, "rpb_ignored" = clip 0's vectors for every row."""
    assert mutant in (None, "clip_pm1", "rpb_ignored") and order in ("torch", "kernel"), (mutant, order)
    rows, D = x.shape
    r = torch.arange(rows)
    if mutant == "clip_pm1":
        r = r // 4 * 4
    b = r // (rows_per_batch if rows_per_batch else max(rows, 1))
    if mutant == "rpb_ignored":
        b = b * 0
    if add_vec is not None:
        x = (x.float() + add_vec[b].float()).to(BF)
    xf = x.float()
    if order == "kernel":
        mean, var = _ln_kernel_stats(xf)
        n = ((xf - mean) * (1.0 / torch.sqrt(var + 1e-6))).to(BF).float()
    else:
        mean = xf.sum(-1, keepdim=True) / D
        var = (xf - mean).pow(2).sum(-1, keepdim=True) / D
        n = ((xf - mean) * torch.rsqrt(var + 1e-6)).to(BF).float()
    one_plus = (1 + scale[b].float()).to(BF).float()
    return x, ((n * one_plus).to(BF).float() + shift[b].float()).to(BF)


# ------------------------------------------------------------------------------------------------ GEMV, RMSNorm
# G weight groups [G, N, K]; x [Gx, B, K] (Gx = 1: shared); add / mul [Ga | Gm, B, N] (0 = absent, 1 = shared, G = per group)
GemvCase = namedtuple("GemvCase", "G Gx B N K Ga Gm act seed")
GRID_GEMV = [GemvCase(5, 1, 3, 384, 256, 1, 5, 1, 5000), GemvCase(4, 4, 2, 7, 8, 4, 1, 0, 5001),
             GemvCase(3, 1, 2, 1, 64, 0, 3, 1, 5002), GemvCase(2, 2, 3, 1000, 4096, 1, 0, 0, 5003),
             GemvCase(1, 1, 2, 1000, 264, 0, 0, 0, 5004), GemvCase(3, 3, 2, 1, 8, 3, 3, 0, 5005)]


def gemv_id(c):
    return f"G{c.G}-Gx{c.Gx}-B{c.B}-N{c.N}-K{c.K}-add{c.Ga}-mul{c.Gm}-act{c.act}"


def gemv_bound(c):
    """test_gemv_shared_input's default bound for the plain product, test_gemv_grouped_silu_add_mul's with add / mul / SiLU."""
    return dict(max_ulp=2, frac_exact=0.95) if (c.Ga or c.Gm or c.act) else dict(max_ulp=1, frac_exact=0.98)


def gemv_inputs(c):
    x, w = rnd((c.Gx, c.B, c.K), seed=c.seed), rnd((c.G, c.N, c.K), c.K ** -0.5, seed=c.seed + 1)
    add = rnd((c.Ga, c.B, c.N), seed=c.seed + 2) if c.Ga else None
    mul = rnd((c.Gm, c.B, c.N), seed=c.seed + 3) if c.Gm else None
    return x, w, add, mul


def gemv_ref(x, w, add=None, mul=None, act=0):
    """y[g, b] = mul * (bf16(W[g] . act(x[g | 0, b])) + add): fp64 product, bf16 torch ops after it (SiLU: torch CPU bf16)."""
    xa = F.silu(x) if act else x
    y = torch.einsum("gbk,gnk->gbn", xa.double().expand(w.shape[0], -1, -1), w.double()).to(BF)
    if add is not None:
        y = y + add
    if mul is not None:
        y = mul * y
    return y


def gemv_standin(x, w, add=None, mul=None, act=0):
    xa = (F.silu(x) if act else x).float().expand(w.shape[0], -1, -1)
    K = w.shape[2]
    y = sum(torch.einsum("gbk,gnk->gbn", xa[..., k:k + 8], w.float()[..., k:k + 8]) for k in reversed(range(0, K, 8))).to(BF)
    if add is not None:
        y = (y.float() + add.float()).to(BF)
    if mul is not None:
        y = (mul.float() * y.float()).to(BF)
    return y


GRID_RMSNORM = [(1, 8, 5100), (3, 4096, 5101), (5, 1032, 5102), (257, 128, 5103), (4, 8192, 5104)]     # rows, D, seed
RMSNORM_BOUND = dict(max_ulp=1, frac_exact=0.995)         # test_rmsnorm_matches_oracle


def rmsnorm_standin(x, w):
    xf = x.float()
    r = 1.0 / torch.sqrt(xf.pow(2).sum(-1, keepdim=True) / x.shape[-1] + 1e-6)
    return ((xf * r) * w.float()).to(BF)


# ------------------------------------------------------------------------------------------------ index / sampler / post-process
GRID_PATCHIFY = [(2, 16, 2, 8, 8), (3, 136, 1, 4, 6)]          # B, cond channels, T, H, W (patch 1 x 2 x 2)
GRID_UNPATCHIFY = [(2, 2, 5, 7), (3, 1, 3, 4)]                 # B, Tp, Hp, Wp
GRID_SAMPLER_N = [1, 7, 4097]                                  # element counts either side of every vector width
GRID_POSTPROCESS = [(2, 3, 5, 7), (3, 1, 4, 9)]                # B, T, H, W (odd W)


# ------------------------------------------------------------------------------------------------ slab GEMM (drn_gemm_bf16_blocked)
# Operands in column planes (include/drn.h): logical A[m][k] at A + (k / a_block_cols) * a_block_stride + m * lda + k % a_block_cols,
# logical C[m][n] at C + (n / c_block_cols) * c_block_stride + m * ldc + n % c_block_cols.
def planes_of(t, cols):
    """Logical [M, X] -> planes [X / cols, M, cols] (contiguous)."""
    M, X = t.shape
    assert X % cols == 0, (X, cols)
    return t.reshape(M, X // cols, cols).permute(1, 0, 2).contiguous()


def from_planes(p):
    """Planes [P, M, cols] (any strides) -> logical [M, P cols]."""
    P, M, cols = p.shape
    return p.permute(1, 0, 2).reshape(M, P * cols)


def place_planes(P, M, cols, ld, gap, device, value=None, pad_rows=2):
    """P planes of M x cols in ONE sentinel-filled allocation (guarded(..., batches=P, batch_gap=gap)): row stride ld >= cols, plane
    stride M ld + gap.  The row padding, the gaps between planes and the guard rows hold the NaN sentinel.  value: planes [P, M, cols]
    copied in.  Returns (buffer, window [P, M, cols])."""
    buf, v = guarded(M, cols, ld, pad_rows, device, batches=P, batch_gap=gap)
    if P == 1:
        v = torch.as_strided(buf, (1, M, cols), (M * ld + gap, ld, 1), pad_rows * ld)
    if value is not None:
        v.copy_(value)
    return buf, v


def gemm_cost_model(M, N):
    """(tile, cost) of csrc/gemm_plan.h's gemm_pick_tile under its defaults (tests/test_sp_slab_refs_cpu.py holds it to
    drn_gemm_tile_choice): 0 = 128 x 128, 1 = 256 x 256, 2 = 144 x 256."""
    if N < 256 or N % 256:
        return 0, 1e30
    t256, t128, t144 = -(-M // 256) * (N // 256), -(-M // 128) * (N // 128), -(-M // 144) * (N // 256)
    c128 = 0.65 * (-(-t128 // 512))
    c256 = float(-(-t256 // 256)) if M >= 256 else 1e30
    c144 = 0.64 * (-(-t144 // 256)) if (M >= 144 and t144 >= 192) else 1e30
    best = 2 if (c144 < c256 and c144 < c128) else (1 if c256 <= c128 else 0)
    return best, (c144 if best == 2 else c256 if best == 1 else c128)


def gemm_plan_rows(M, N, blocked=True):
    """(rows of the first launch, its tile) as gemm_plan_clip of csrc/gemm_plan.h plans ONE clip without the 384-row tile: the rows
    that fill whole rounds of 256 x 256 workgroups, the rest left to the launches after it when that is cheaper.  A blocked launch
    never leaves a tail to the 128 x 128 kernel."""
    tile, cost_all = gemm_cost_model(M, N)
    if tile != 1:
        return M, tile
    tm, tn = -(-M // 256), N // 256
    rounds, rem = tm * tn // 256, tm * tn % 256
    tm_main = rounds * 256 // tn
    if rounds < 1 or rem == 0 or tm_main < 1 or tm_main >= tm:
        return M, tile
    tail_tile, cost_tail = gemm_cost_model(M - tm_main * 256, N)
    if blocked and tail_tile == 0:
        cost_tail = 1e30
    return (tm_main * 256 if -(-tm_main * tn // 256) + cost_tail + 0.02 < cost_all - 0.05 else M), tile


GEMM384_MEASURED = ((18432, 4096, 16384),)             # the shapes on which the dispatcher takes the 384 x 256 tile by default


def gemm384_ok(M, N, K, ldmax, epi=EPI_NONE, rpb=0):
    """The 384 x 256 kernel's preconditions on a plain launch (drn_gemm384_ok): whole tiles, >= 2 K steps, a tile within 32-bit lane
    offsets, and with the gated residual every tile inside one clip."""
    if M < 384 or M % 384 or N % 256 or K % 64 or K < 128 or ldmax < K or (384 * ldmax + 4096) * 2 >= 1 << 31:
        return False
    return epi != EPI_GATE_RES or (rpb if 0 < rpb <= M else M) % 384 == 0


def gemm_tall_slices(M, N, K):
    """gemm_tall.hip's rule for ONE clip of M rows: 1 = the few-token kernel unsplit, n > 1 = its n K slices, 0 = another kernel."""
    if M != 256 or N % 64 or K % 64:
        return 0
    if N // 64 >= 192:
        return 1
    return next((s for s in (2, 4, 8) if 192 <= N // 64 * s <= 256 and K // 64 % s == 0 and 1024 <= K // s <= 2048), 0)


def gemm_plan_launches(M, N, K, ld=None, epi=EPI_NONE, rpb=0, blocked=False):
    """Every launch of a drn_gemm_bf16 / _blocked call under the default settings as [(kernel, first row, rows, rows_per_batch)],
    None where the call is refused; kernel 5 = 384 x 256, 6 = the few-token kernel.  ld = (lda, ldw, ldc, ldr), contiguous when None.
    An independent model of csrc/gemm_plan.h (tests/test_gemm_plan_cpu.py holds drn_gemm_plan_describe to it)."""
    lda, ldw, ldc, ldr = ld or (K, K, N, N)
    ldmax = max(lda, ldw, ldc, ldr if epi == EPI_GATE_RES else 0)
    batched = not blocked and 0 < rpb < M and M % rpb == 0
    Mb = rpb if batched else M
    if not blocked and M % 256 == 0 and lda >= K and gemm_tall_slices(Mb, N, K) == 1:
        return [(6, 0, M, rpb if rpb > 0 else M)]
    if not batched and epi == EPI_GATE_RES and rpb < M:    # ragged clips, blocked clips: one launch, the tile of the whole problem
        tile = gemm_cost_model(M, N)[0]
        return None if blocked and tile == 0 else [(tile, 0, M, rpb)]
    clip, row = [], 0
    while row < Mb:
        rows, tile = gemm_plan_rows(Mb - row, N, blocked)
        if not blocked and (Mb - row, N, K) in GEMM384_MEASURED and gemm384_ok(Mb - row, N, K, ldmax):
            rows, tile = Mb - row, 5
        if blocked and tile == 0:
            return None
        clip.append((tile, row, rows, rows))
        row += rows
    if len(clip) == 1:
        return [(clip[0][0], 0, M, Mb)]
    return [(t, b * Mb + r, n, n) for b in range(M // Mb) for t, r, n, _ in clip]


# tile: 1 / 2 = drn_gemm_force_tile, -1 = automatic dispatch.  layout: "a" = A in planes of abc columns, "c" = C in planes of cbc
# columns, "ac" = both (the other operand plain).  padded: lda / ldc = width + 64 (planes: plane gap 128 elements; the residual window
# ldr = N + 128), else contiguous.  alias: the residual IS the (plain) output window.  rpb: rows per clip.  pre: the launch takes the
# residual-prefetch variant of the 256-row kernel (and is repeated with the prefetch off).
BlockedCase = namedtuple("BlockedCase", "tile M N K epi layout abc cbc padded alias rpb pre seed")


def _widths(K):
    """The a_block_cols a K allows out of 64 (a new plane every K step), 128 and K / 2: powers of two >= 64 that divide K."""
    return [v for v in dict.fromkeys((64, 128, K // 2)) if v >= 64 and v & (v - 1) == 0 and K % v == 0]


def _gemm_blocked_grid():
    cases, seed, i = [], 7000, 0
    ks = (64, 128, 192, 4096)                          # 1, 2, 3 and 64 K steps of 64
    seen_k, seen_a, seen_c = {}, {}, {}                # how often a K, a K with A planes, an N with C planes has come up
    for tile in (1, 2):
        h = GEMM_TILE_ROWS[tile]
        for M in (h - 1, h, h + 1, 2 * h + 1):
            for epi in (EPI_NONE, EPI_GELU, EPI_GATE_RES):
                for layout in ("a", "c", "ac"):
                    seed, i = seed + 1, i + 1
                    K, N = ks[i % 4], (512, 1024)[(i // 4) % 2]
                    # K cycles; each K cycles through the A widths it allows, each N through its C widths; padding alternates per K
                    abc = _widths(K)[seen_a.get(K, 0) % len(_widths(K))]
                    cbc = (256, N // 2)[seen_c.get(N, 0) % 2]
                    padded = seen_k.get(K, 0) % 2 == 1
                    seen_k[K] = seen_k.get(K, 0) + 1
                    seen_a[K] = seen_a.get(K, 0) + ("a" in layout)
                    seen_c[N] = seen_c.get(N, 0) + ("c" in layout)
                    alias = epi == EPI_GATE_RES and layout == "a" and M % 2 == 1
                    cases.append(BlockedCase(tile, M, N, K, epi, layout, abc if "a" in layout else 0, cbc if "c" in layout else 0,
                                             padded, alias, M, False, seed))
        # gated residual, A planes, written in place (the output projection of the sharded forward); C planes with R in its own window
        cases.append(BlockedCase(tile, 2 * h + 1, 512, 192, EPI_GATE_RES, "a", 64, 0, True, True, 2 * h + 1, False, seed + 100))
        cases.append(BlockedCase(tile, 2 * h + 1, 1024, 128, EPI_GATE_RES, "c", 0, 256, True, False, 2 * h + 1, False, seed + 101))
        # two clips, the boundary inside a tile: the gate row follows the row
        for j, M in enumerate((h + 1, 2 * h + 1)):
            cases.append(BlockedCase(tile, M, 512, 128, EPI_GATE_RES, "a", 64, 0, j == 0, True, (M + 1) // 2, False, seed + 110 + j))
            cases.append(BlockedCase(tile, M, 1024, 192, EPI_GATE_RES, "ac", 64, 512, j == 1, False, (M + 1) // 2, False, seed + 120 + j))
    # M = 2 h, K = 4096 on the 256-row kernel: whole tiles inside one clip, 64 K steps = the residual-prefetch variant
    cases.append(BlockedCase(1, 512, 512, 4096, EPI_GATE_RES, "a", 64, 0, True, True, 512, True, 7300))
    cases.append(BlockedCase(1, 512, 1024, 4096, EPI_GATE_RES, "ac", 2048, 256, False, False, 512, True, 7301))
    # automatic dispatch at the band shapes of the "slabs" route: K | V (N = 2 D) and Q (N = D) projections into C planes of
    # N / world columns, world = 8, 4, 2 (one seed per (rows, N): the three plane widths share one fp64 reference)
    for r, rows in enumerate((2304, 4608, 9216)):
        for n, N in enumerate((4096, 8192)):
            for p, P in enumerate((8, 4, 2)):
                cases.append(BlockedCase(-1, rows, N, 128, EPI_NONE, "c", 0, N // P, (r + n + p) % 2 == 1, False, rows, False,
                                         7400 + 10 * r + n))
    # the output projection: A in 8 planes of 128 columns, gated residual in place
    for r, rows in enumerate((2304, 9216)):
        cases.append(BlockedCase(-1, rows, 4096, 1024, EPI_GATE_RES, "a", 128, 0, r == 0, True, rows, False, 7450 + r))
    # The tail split of gemm_plan_clip (rows that fill whole rounds of 256 x 256 workgroups, the rest in a second launch that advances
    # A by M_main * lda inside every plane).  drn_gemm_tile_choice / gemm_plan_rows over M < 20000: the band shape 9216 x 8192 above
    # is one (8192 rows on the 256-row kernel, 1024 on the 144-row one); the smallest is 4817 x 8192 (4096 rows, then a ragged 721
    # on the 144-row kernel).  The latter with A planes too, and with the gated residual in place.
    cases.append(BlockedCase(-1, 4817, 8192, 128, EPI_NONE, "ac", 64, 1024, True, False, 4817, False, 7460))
    cases.append(BlockedCase(-1, 4817, 8192, 128, EPI_GATE_RES, "a", 64, 0, False, True, 4817, False, 7461))
    return cases


GRID_GEMM_BLOCKED = _gemm_blocked_grid()


def blocked_id(c):
    return (f"{'auto' if c.tile < 0 else 'tile' + str(c.tile)}-M{c.M}-N{c.N}-K{c.K}-epi{c.epi}-{c.layout}-a{c.abc}-c{c.cbc}"
            + ("-pad" if c.padded else "-contig") + ("-alias" if c.alias else "") + (f"-rpb{c.rpb}" if c.rpb != c.M else "")
            + ("-pre" if c.pre else ""))


_BLOCKED_REF = {}


def blocked_inputs_ref(c):
    """(a, w, gate, res, ref, mag) of a case: gemm_inputs and gemm_ref, computed once per (shape, epilogue, seed) and shared."""
    key = (c.M, c.N, c.K, c.epi, c.rpb, c.seed)
    if key not in _BLOCKED_REF:
        if c.M * c.N > 1 << 22:
            _BLOCKED_REF.clear()                       # one large reference resident at a time
        a, w, gate, res = gemm_inputs(c)
        _BLOCKED_REF[key] = (a, w, gate, res) + tuple(gemm_ref(a, w, c.epi, gate, res, c.rpb))
    return _BLOCKED_REF[key]


def blocked_geometry(c):
    """dict(lda, a_stride, ldc, c_stride, ldr, gap) of a case as both the stand-in and the GPU test place it."""
    pad, gap = (64, 128) if c.padded else (0, 0)
    aw, cw = (c.abc or c.K), (c.cbc or c.N)
    lda, ldc = aw + pad, cw + pad
    return dict(lda=lda, a_stride=c.M * lda + gap if c.abc else 0, ldc=ldc, c_stride=c.M * ldc + gap if c.cbc else 0,
                ldr=ldc if c.alias else c.N + 2 * pad, gap=gap)


def blocked_windows(c, a, res, device):
    """The operand windows of a case on `device`: A (planes or plain) filled, C (planes or plain; pre-filled with the residual when
    it aliases it), R.  Returns dict(a=(buf, win), c=(buf, win), r=(buf, win) | None); win is [P, M, cols] (P = 1 when plain)."""
    g = blocked_geometry(c)
    pa, pc = (c.K // c.abc if c.abc else 1), (c.N // c.cbc if c.cbc else 1)
    out = dict(a=place_planes(pa, c.M, c.K // pa, g["lda"], g["gap"] if c.abc else 0, device, planes_of(a, c.K // pa).to(device)),
               c=place_planes(pc, c.M, c.N // pc, g["ldc"], g["gap"] if c.cbc else 0, device), r=None)
    if c.epi == EPI_GATE_RES:
        if c.alias:
            assert not c.cbc, "the residual is a plain matrix: only a plain C can alias it"
            out["c"][1][0].copy_(res)
        else:
            out["r"] = place_planes(1, c.M, c.N, g["ldr"], 0, device, res.to(device).unsqueeze(0))
    return out


BLOCKED_MUTANTS = ("a_plane_stride_ignored", "a_koff_no_wrap", "a_plane_of_tile", "c_plane_neighbour", "c_ld_plain",
                   "tail_rows_plane0", "res_read_as_planes")


def _gather(buf, idx):
    """buf.flatten()[idx]; an index outside the allocation reads the sentinel (on the GPU: whatever lies there, or a fault)."""
    flat = buf.reshape(-1)
    ok = (idx >= 0) & (idx < flat.numel())
    out = flat[idx.clamp(0, flat.numel() - 1)].clone()
    out.view(torch.int16)[~ok] = SENTINEL
    return out


def gemm_blocked_standin(c, wins, w, gate, mutant=None, slices=1):
    """gemm_standin's arithmetic reading A and R and writing C through the plane addressing of include/drn.h, element by element on
    the flat allocations of blocked_windows (CPU).  Mutants:
      a_plane_stride_ignored  A planes assumed contiguous (plane stride M lda)
      a_koff_no_wrap          k % a_block_cols lost: past the first plane the read runs on into the row's padding / the next row
      a_plane_of_tile         the plane taken from the tile's first K step only (every K step reads plane 0)
      c_plane_neighbour       column tiles past the first store into the plane of the tile before them
      c_ld_plain              rows of a C plane stored with row stride N
      tail_rows_plane0        rows past the first launch of a tail split (gemm_plan_rows) get their row offset in plane 0 only
      res_read_as_planes      R addressed like C (planes, ldc)
    A store outside the allocation is dropped (on the GPU: a fault at best); what it leaves unwritten is found like any other."""
    assert mutant is None or mutant in BLOCKED_MUTANTS, mutant
    g = blocked_geometry(c)
    M, N, K = c.M, c.N, c.K
    m = torch.arange(M).view(M, 1)
    (abuf, awin), (cbuf, cwin) = wins["a"], wins["c"]
    # ---- A
    k = torch.arange(K).view(1, K)
    if c.abc:
        plane, col = k // c.abc, k % c.abc
        stride = M * g["lda"] if mutant == "a_plane_stride_ignored" else g["a_stride"]
        if mutant == "a_koff_no_wrap":
            col = k                                    # the whole k instead of k % a_block_cols
        if mutant == "a_plane_of_tile":
            plane = plane * 0
        row = m.expand(M, K)
        if mutant == "tail_rows_plane0":
            m_main = gemm_plan_rows(M, N)[0] if c.tile < 0 else M
            row = torch.where((m >= m_main) & (plane > 0), m - m_main, m)
        ia = plane * stride + row * g["lda"] + col
    else:
        ia = m * g["lda"] + k
    a = _gather(abuf, ia + awin.storage_offset())
    # ---- R (read before C is written: it may be the same memory)
    n = torch.arange(N).view(1, N)
    res = None
    if c.epi == EPI_GATE_RES:
        rbuf, rwin = (cbuf, cwin) if c.alias else wins["r"]
        ir = m * g["ldr"] + n
        if mutant == "res_read_as_planes" and c.cbc:
            ir = (n // c.cbc) * g["c_stride"] + m * g["ldc"] + n % c.cbc
        res = _gather(rbuf, ir + rwin.storage_offset())
    out = gemm_standin(a, w, c.epi, gate, res, c.rpb, slices=slices)
    # ---- C
    flat = cbuf.reshape(-1)
    for r0 in range(0, M, 2048):                       # (row bands: the index tensors of a 9216 x 8192 output stay small)
        mm = m[r0:r0 + 2048]
        if c.cbc:
            plane = n // c.cbc
            if mutant == "c_plane_neighbour":
                plane = torch.where(n >= 256, (n // 256 * 256 - 256) // c.cbc, plane)
            ic = plane * g["c_stride"] + mm * (N if mutant == "c_ld_plain" else g["ldc"]) + n % c.cbc
        else:
            ic = mm * g["ldc"] + n
        ic = (ic + cwin.storage_offset()).reshape(-1)
        ok = (ic >= 0) & (ic < flat.numel())
        flat[ic[ok]] = out[r0:r0 + 2048].reshape(-1)[ok]
    return from_planes(cwin)
