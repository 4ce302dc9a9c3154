"""References, cases and wrong stand-ins for `window_align` (windows.align_affine / apply_affine, csrc/window_align.hip).

Everything here is numpy / torch on the CPU and independent of the code under test.
- `Reference`: the rules evaluated in float64 from sums taken with math.fsum (exact sums of exact products: a product of two
  bf16 values has 16 significant bits), and the same rules from numpy's pairwise float64 sums.
- its allowance: one fp32 ulp of the exact value plus 4 x the distance between those two evaluations - what any correct float64
  summation order may differ by, measured on the case itself and never on the code under test.
- `standin`: what the kernel does (block partition, partials summed in index order), and WRONG kernels by name;
  tests/test_window_align_cpu.py shows that the right one passes every case and that each wrong one fails a named case.
- `align_postprocess` / `walk`: the byte reference of the apply, of one window and of a windowed clip, with wrong variants.
"""
import functools
import itertools
import math

import numpy as np
import torch

import window_refs as WR

BF = torch.bfloat16
TW = WR.TW
# H x W.  37 x 53 and 64 x 96: three blocks per pass at the least (one per channel), 37 x 53 on the one-value path; 64 x 96 and
# 45 x 61 (one-value path) at O = 4 also cut a channel's run of 24 576 / 10 980 values into several 8192-value blocks, the last partial
SHAPES = [(8, 8), (5, 7), (3, 11), (8, 12), (37, 53), (64, 96), (45, 61)]
OVERLAPS = [1, 2, 4]
BATCHES = [1, 3]
OFFSETS = [0, 1]                                                     # element offset of both bases (1: 2-byte aligned only)
FLAT_VAR = 2.0 ** -20
CHUNK = 8192                                                         # csrc/window_align.hip ALIGN_CHUNK
ROWS = [(0.7, 0.1), (1.3, -0.2), (1.8, 0.05)]                        # (g_true, o_true) per pass row: different statistics per row
STANDINS = ["slope", "per_channel", "row0", "o_unclamped", "no_sqrt", "swapped", "head"]
APPLY_VARIANTS = ["fma", "after_blend", "ramp_only", "raw_carry", "normal_aligned"]


def ramp_ats(O):
    return sorted({0, 3, TW - O})


def grid():
    """(H, W, O, B, ramp_at, offset) of every kernel case."""
    return [(H, W, O, B, at, off) for (H, W), O, B in itertools.product(SHAPES, OVERLAPS, BATCHES)
            for at in ramp_ats(O) for off in OFFSETS]


# ----------------------------------------------------------------------------------------------- the rules
def solve(n, sa, sv, saa, svv, sav, variant=None):
    """float64 rules from the five sums -> (g, o, moments[6]); g and o not yet rounded to fp32."""
    f = np.float64
    with np.errstate(all="ignore"):
        n = f(n)
        ma, mv = f(sa) / n, f(sv) / n
        va, vv, cov = f(saa) / n - ma * ma, f(svv) / n - mv * mv, f(sav) / n - ma * mv
        mom = np.array([n, ma, mv, va, vv, cov], dtype=f)
        if not np.isfinite(mom).all():
            return f(1.0), f(0.0), mom
        g = f(1.0)
        if va >= FLAT_VAR and vv >= FLAT_VAR and cov > 0:
            g = cov / vv if variant == "slope" else (va / vv if variant == "no_sqrt" else np.sqrt(va / vv))
        raw = g
        g = min(max(g, f(0.5)), f(2.0))
        return g, ma - (raw if variant == "o_unclamped" else g) * mv, mom


def _flat64(t):
    return t.to(torch.float64).numpy().reshape(-1)


def _sums(a, v, how):
    if how == "fsum":
        al, vl = a.tolist(), v.tolist()
        return (math.fsum(al), math.fsum(vl), math.fsum(x * x for x in al), math.fsum(x * x for x in vl),
                math.fsum(x * y for x, y in zip(al, vl)))
    return a.sum(), v.sum(), (a * a).sum(), (v * v).sum(), (a * v).sum()


def evaluate(prev, over, how):
    """prev, over bf16 [B,3,O,H,W] (the carry and the window's overlap frames) -> float64 (affine [B,2], moments [B,6])."""
    B = prev.shape[0]
    aff, mom = np.empty((B, 2)), np.empty((B, 6))
    for b in range(B):
        a, v = _flat64(prev[b]), _flat64(over[b])
        g, o, m = solve(a.size, *_sums(a, v, how))
        aff[b], mom[b] = (g, o), m
    return aff, mom


def ulp32(x):
    with np.errstate(all="ignore"):
        return np.abs(np.spacing(np.asarray(x, dtype=np.float64).astype(np.float32))).astype(np.float64)


class Reference:
    """The two evaluations of one case and what follows from them."""

    def __init__(self, prev, over):
        self.affine, self.moments = evaluate(prev, over, "fsum")
        self.affine_pw, self.moments_pw = evaluate(prev, over, "pairwise")
        with np.errstate(all="ignore"):
            self.allow = ulp32(self.affine) + 4 * np.abs(self.affine - self.affine_pw)
            self.allow_moments = 2.0 ** -23 * np.abs(self.moments) + 4 * np.abs(self.moments - self.moments_pw)

    def affine_ok(self, got):
        """got: fp32 / float64 [B,2].  Non-finite moments: exactly (1, 0)."""
        got = np.asarray(got, dtype=np.float64)
        with np.errstate(all="ignore"):
            return bool((np.abs(got - self.affine) <= self.allow).all())

    def moments_ok(self, got):
        got = np.asarray(got, dtype=np.float64)
        fin = np.isfinite(self.moments)
        with np.errstate(all="ignore"):
            return bool(np.array_equal(np.isfinite(got), fin) and (np.abs(got - self.moments)[fin] <= self.allow_moments[fin]).all())

    def worst(self, got):
        """The largest |got - exact| in units of the allowance (printed by the tests)."""
        got = np.asarray(got, dtype=np.float64)
        with np.errstate(all="ignore"):
            return float((np.abs(got - self.affine) / self.allow).max())


# ----------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def overlap_pair(H, W, O, B):
    """(prev, over) bf16 [B,3,O,H,W] of one grid case: over = x, prev = g_true * x + o_true + noise per row; the channels of x
    differ in mean and spread (so per-channel moments are not the pooled ones), var_v >= 1e-3."""
    g = torch.Generator().manual_seed(9000 + 1000 * B + 100 * O + 7 * H + W)
    scale = torch.tensor([0.5, 0.3, 0.15]).view(1, 3, 1, 1, 1)
    shift = torch.tensor([-0.2, 0.1, 0.3]).view(1, 3, 1, 1, 1)
    x = (torch.randn((B, 3, O, H, W), generator=g) * scale + shift).to(BF)
    gt = torch.tensor([ROWS[b][0] for b in range(B)]).view(B, 1, 1, 1, 1)
    ot = torch.tensor([ROWS[b][1] for b in range(B)]).view(B, 1, 1, 1, 1)
    prev = (x.float() * gt + ot + 0.05 * torch.randn(x.shape, generator=g)).to(BF)
    return prev, x


@functools.lru_cache(maxsize=None)
def overlap_reference(H, W, O, B):
    return Reference(*overlap_pair(H, W, O, B))


def window_around(over, ramp_at, seed=0):
    """A window [B,3,TW,H,W] of seeded values that holds `over` at frames [ramp_at, ramp_at + O)."""
    B, _, O, H, W = over.shape
    g = torch.Generator().manual_seed(4242 + seed + ramp_at)
    video = (torch.randn((B, 3, TW, H, W), generator=g) * 0.8).to(BF)
    video[:, :, ramp_at:ramp_at + O] = over
    return video


RULE_HW, RULE_O, RULE_AT = (8, 12), 2, 3
RULE_CASES = ["flat_a", "flat_v", "cov_negative", "gain_4", "gain_quarter", "nan_in_a", "nan_in_v", "inf_in_a", "inf_in_v",
              "scale_65504"]


@functools.lru_cache(maxsize=None)
def rule_pair(name):
    """(prev, over, what the exact affine must be or None) of one rule case, B = 1."""
    H, W = RULE_HW
    g = torch.Generator().manual_seed(6000 + RULE_CASES.index(name))
    x = (torch.randn((1, 3, RULE_O, H, W), generator=g) * 0.4 + 0.1).to(BF)
    noise = 0.02 * torch.randn(x.shape, generator=g)
    want = None
    if name == "flat_a":
        prev, over, want = torch.full(x.shape, 0.30078125).to(BF), x, "g1"
    elif name == "flat_v":
        prev, over, want = x, torch.full(x.shape, -0.25).to(BF), "g1"
    elif name == "cov_negative":
        prev, over, want = (-x.float() + noise).to(BF), x, "g1"
    elif name == "gain_4":
        prev, over, want = (4 * x.float() + 0.2 + noise).to(BF), x, "g2"
    elif name == "gain_quarter":
        prev, over, want = (0.25 * x.float() - 0.1 + 0.1 * noise).to(BF), x, "g0.5"
    elif name == "scale_65504":
        big = (torch.randn(x.shape, generator=g) * 0.3 * 65504).to(BF)
        prev, over = (1.2 * big.float() + 500.0 + 65504 * noise).to(BF), big
    else:
        prev, over, want = (1.1 * x.float() + noise).to(BF), x.clone(), "identity"
        bad = float("nan") if name.startswith("nan") else float("inf")
        (prev if name.endswith("_a") else over)[0, 1, 1, 3, 5] = bad
    return prev, over, want


@functools.lru_cache(maxsize=None)
def rule_reference(name):
    prev, over, _ = rule_pair(name)
    return Reference(prev, over)


# ----------------------------------------------------------------------------------------------- the kernel's stand-in
def standin(prev, video, ramp_at, variant=None):
    """What drn_window_align_affine computes, in numpy: per pass and channel the run of O * H * W values is cut into CHUNK-value
    blocks, each block's five sums are taken (256 lanes of 8-value groups, lanes added pairwise as the wave's butterfly does), the
    partials are added in index order, the rules follow, and g and o are rounded to fp32 once.  variant: a wrong kernel."""
    B, O = prev.shape[0], prev.shape[2]
    out = np.empty((B, 2), dtype=np.float32)
    for b in range(B):
        at = 0 if variant == "head" else ramp_at
        a_all, v_all = prev[b], video[b, :, at:at + O]
        if variant == "swapped":
            a_all, v_all = v_all, a_all
        chans = [0] if variant == "per_channel" else [0, 1, 2]
        tot = np.zeros(5)
        for ch in chans:
            a, v = _flat64(a_all[ch]), _flat64(v_all[ch])
            for lo in range(0, a.size, CHUNK):
                aa, vv = a[lo:lo + CHUNK], v[lo:lo + CHUNK]
                pad = (-aa.size) % 256
                cols = [np.pad(c, (0, pad)).reshape(-1, 256) for c in (aa, vv, aa * aa, vv * vv, aa * vv)]
                tot += np.array([c.sum(0).reshape(4, 64).sum(1).sum() for c in cols])     # lanes, waves, block - a fixed order
        n = sum(a_all[ch].numel() for ch in chans)
        g, o, _ = solve(n, *tot, variant=variant)
        out[b] = (np.float32(g), np.float32(o))
    if variant == "row0":
        out[:] = out[0]
    return out


# ----------------------------------------------------------------------------------------------- the apply, in bytes
def apply_affine(video, affine, variant=None):
    """bf16 [B,3,T,H,W], fp32 [B,2] -> bf16(fp32(g * x) + o); "fma": one rounding of g * x + o."""
    g = torch.as_tensor(affine)[:, 0].float().view(-1, 1, 1, 1, 1)
    o = torch.as_tensor(affine)[:, 1].float().view(-1, 1, 1, 1, 1)
    if variant == "fma":
        return (video.double() * g.double() + o.double()).float().to(BF)
    return (video.float() * g + o).to(BF)


@functools.lru_cache(maxsize=None)
def fma_affine(min_hits=1):
    """An affine under which a fused apply SHOWS on window_refs.value_grid.  fp32(fp32(g * x) + o) and fp32(g * x + o) differ by an
    fp32 ulp for about every other x, but the bf16 results differ only where that ulp straddles a bf16 tie: about one x in 2^17 for
    about 33 000 values and 100 affines taken at random.  So the pair is searched (seeded, a few hundred draws): the first (g, o) for which at
    least `min_hits` of the finite bf16 values in [-4, 4] - each of them is in the value grid's window some 40 times - give
    different output BYTES fused and unfused.  -> (g, o) as Python floats of fp32 values."""
    x = WR.bf16_values()
    xv = x.view(1, 1, 1, -1, 1).expand(1, 3, 1, -1, 1)
    rng = np.random.default_rng(20)
    for _ in range(4000):
        g, o = float(np.float32(rng.uniform(0.5, 2.0))), float(np.float32(rng.uniform(-0.5, 0.5)))
        aff = torch.tensor([[g, o]])
        a, b = apply_affine(xv, aff), apply_affine(xv, aff, "fma")
        if int((a.view(torch.int16) != b.view(torch.int16)).sum()) < 3 * min_hits:
            continue
        if int((WR.O.postprocess(a, False) != WR.O.postprocess(b, False)).sum()) >= 3 * min_hits:
            return g, o
    raise AssertionError("no affine found")


def align_postprocess(video, prev, ramp_w, affine, ramp_at, write_lo, write_hi, normalize, carry_frames=0, variant=None):
    """drn_postprocess_window_align_u8 -> (uint8 [B, write_hi - write_lo, H, W, 3], the next carry [B,3,carry_frames,H,W] or None).
    affine None: drn_postprocess_window_u8 and the raw tail."""
    Tw = video.shape[2]
    v = video if affine is None else apply_affine(video, affine, "fma" if variant == "fma" else None)
    if affine is not None and variant == "ramp_only":
        n = prev.shape[2] if prev is not None else 0
        v = video.clone()
        v[:, :, ramp_at:ramp_at + n] = apply_affine(video, affine)[:, :, ramp_at:ramp_at + n]
    carry = v[:, :, Tw - carry_frames:].contiguous() if carry_frames else None
    if variant == "raw_carry" and carry_frames:
        carry = video[:, :, Tw - carry_frames:].contiguous()
    if affine is not None and variant == "after_blend":
        blended = video.clone()
        if prev is not None and prev.shape[2]:
            n = prev.shape[2]
            blended[:, :, ramp_at:ramp_at + n] = WR._blend(prev.float(), video[:, :, ramp_at:ramp_at + n].float(), ramp_w, None)
        return WR.O.postprocess(apply_affine(blended, affine)[:, :, write_lo:write_hi], normalize), carry
    return WR.blend_postprocess(v, prev, ramp_w, ramp_at, write_lo, write_hi, normalize), carry


def walk(windows, plan, O, ramp_w, flags, align, affine_of, variant=None):
    """The windowed clip of pipeline._walk on decoded windows: windows[i] bf16 [P,3,Tw,H,W] (one row per pass), flags[p] =
    normalize_normal of pass p -> uint8 [P, T, H, W, 3].  affine_of(video, prev, ramp_at) -> fp32 [1,2]."""
    P, _, Tw, H, W = windows[0].shape
    T = plan[-1].out_at + plan[-1].write_hi - plan[-1].write_lo
    out = torch.zeros((P, T, H, W, 3), dtype=torch.uint8)
    carry = [None] * P
    for i, win in enumerate(plan):
        for p in range(P):
            video, prev = windows[i][p:p + 1], carry[p]
            hand_on = O if i + 1 < len(plan) else 0
            aligned = align and prev is not None and (not flags[p] or variant == "normal_aligned")
            if aligned:
                u8, nxt = align_postprocess(video, prev, ramp_w, affine_of(video, prev, win.ramp_at), win.ramp_at, win.write_lo,
                                            win.write_hi, flags[p], hand_on, variant)
            else:
                u8 = WR.blend_postprocess(video, prev, ramp_w if prev is not None else None, win.ramp_at, win.write_lo,
                                          win.write_hi, flags[p])
                nxt = video[:, :, Tw - hand_on:].contiguous() if hand_on else None
            out[p:p + 1, win.out_at:win.out_at + u8.shape[1]] = u8
            carry[p] = nxt
    return out


# ----------------------------------------------------------------------------------------------- quality (recorded, not judged)
QUALITY = dict(T=25, Tw=9, O=1, H=16, W=24, gains=((1.0, 0.0), (0.8, 0.12), (1.25, -0.1)), noise=0.02)


def quality_figures(pkg):
    """A 25-frame piecewise-constant clip in three windows of 9; window k's stub decoder returns g_k * truth + o_k + noise ->
    the mean absolute byte error against window 0's space with window_align (off, on)."""
    q = QUALITY
    g = torch.Generator().manual_seed(31)
    levels = torch.rand((3, q["T"] // 5, 4, 4), generator=g) * 1.2 - 0.6                   # 5-frame, 4 x 6-pixel constant patches
    truth = levels.repeat_interleave(5, 1).repeat_interleave(q["H"] // 4, 2).repeat_interleave(q["W"] // 4, 3).unsqueeze(0)
    plan = pkg.windows.plan_windows(q["T"], q["Tw"], q["O"])
    assert len(plan) == len(q["gains"])
    windows = []
    for win, (gk, ok) in zip(plan, q["gains"]):
        t = truth[:, :, win.start:win.start + q["Tw"]]
        windows.append((gk * t + ok + q["noise"] * torch.randn(t.shape, generator=g)).to(BF))
    g0, o0 = q["gains"][0]
    want = WR.O.postprocess((g0 * truth + o0).to(BF), False).to(torch.int32)
    ramp = WR.ramp_table(pkg, q["O"])
    err = []
    for align in (False, True):
        got = walk(windows, plan, q["O"], ramp, [False], align, pkg.windows.align_affine)
        err.append(float((got.to(torch.int32) - want).abs().float().mean()))
    return tuple(err)
