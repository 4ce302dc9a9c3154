"""Shared references of the guided-restore tests (fit.plan_restore_guided / restore_frames_guided, drn_restore_guided_u8): the
float64 evaluation (the plan's fp32 tap tables written out here a second time as dense matrices and its fp32 range table, applied in
float64 source row by source row, no rounding), the fp32 torch specification's own error against it before its rounding (E_ref,
the unit of the bound), the bound |byte - ref64| <= 0.5 + M_BOUND * E_ref with restore_refs.M_BOUND, the case grid, the named
cases and the wrong stand-ins the bound has to catch.  Everything here runs on the CPU; every case is computed once and shared.

Inputs make the range term matter: guides are palette colours +- 3 levels of noise on piecewise-constant regions (uniformly random
guides would make almost every table read 0 and hide a kernel that ignores the guide), guide_lo is the fit's own tables applied to
guide_hi's bytes (fit.plan_guide_lo), and src is a second palette on the same regions through the same tables, plus noise.

16 x 16 -> 1 x 1 needs 16 taps per axis at the plan's reach of 2.0, which the plan refuses (8 at most); that geometry - one output
pixel: 3 bytes, all of them head or tail - is kept with the widest reach under which it passes, 0.25: 8 taps per axis, the limit."""
import dataclasses

import torch

import restore_refs as RR
from restore_refs import M_BOUND, bound_excess, dense, fit_module, geometry_id, round_u8       # noqa: F401  (shared with the tests)

# model-side (H', W') -> source-side (H, W): the issue's list
GEOMETRIES = [
    ((16, 32), (27, 40)),       # up both axes, 4 taps per axis, 120-byte rows
    ((32, 32), (37, 23)),       # up in y, down in x (6 taps), 69-byte rows
    ((16, 16), (45, 61)),       # 183-byte rows: every row at another alignment; three row tiles
    ((16, 32), (16, 45)),       # one axis at scale 1 (3 taps)
    ((16, 16), (1, 1)),         # one output pixel; 8 taps per axis (reach 0.25, above)
    ((64, 128), (135, 240)),    # several tiles on both axes
]
REACH = {((16, 16), (1, 1)): 0.25}
BATCHES = ((1, 1), (2, 1), (2, 2))                      # (B, Bg)
TIMES = ((1, 1, 1, 0), (3, 2, 5, 2), (3, 3, 3, 0))      # (Ts, Td, Tg, t0)
SIGMA = 12.0
SCENE = ((32, 64), (60, 120))                           # the piecewise-constant scene of the quality check
FLAT = ((16, 32), (27, 40))                             # the flat-frames clip: 256 frames, frame v filled with v
SWEEP = ((32, 64), (60, 120))
SWEEP_SIGMA = 64.0                                      # every entry of the table is then large enough to move a byte

GUIDE_PALETTE = torch.tensor([[30, 30, 30], [220, 40, 40], [40, 220, 40], [40, 40, 220], [220, 220, 40], [40, 220, 220],
                              [220, 40, 220]], dtype=torch.int32)
REGIONS = len(GUIDE_PALETTE)


def guided_plan(pkg, g, T, sigma=SIGMA):
    fit = fit_module(pkg)
    (hm, wm), (h, w) = g
    plan = fit.plan_fit(T, h, w, "stretch", hm, wm, windowed=True)
    return plan, fit.plan_restore_guided(plan, sigma, reach=REACH.get(g, fit.GUIDED_REACH))


# ----------------------------------------------------------------------------------------------- scenes
def regions(B, T, H, W, gen):
    """int64 [B, T, H, W]: the nearest of REGIONS seed points, which drift from frame to frame and differ from clip to clip."""
    seeds = torch.rand(B, 1, REGIONS, 2, generator=gen) + 0.07 * torch.arange(T).view(1, T, 1, 1) * torch.tensor([1.0, -0.6])
    yy = (torch.arange(H, dtype=torch.float32) + 0.5) / H
    xx = (torch.arange(W, dtype=torch.float32) + 0.5) / W
    d = (yy.view(1, 1, 1, H, 1) - seeds[..., 0].remainder(1.0).view(B, T, REGIONS, 1, 1)) ** 2 \
        + (xx.view(1, 1, 1, 1, W) - seeds[..., 1].remainder(1.0).view(B, T, REGIONS, 1, 1)) ** 2
    return d.argmin(dim=2)


def scene(pkg, plan, B, T, seed, noise=3, src_noise=0):
    """-> (guide_hi [B,T,H,W,3], guide_lo [B,T,H',W',3], truth [B,T,H,W,3] at full size, src [B,T,H',W',3]): guide_hi = the guide
    palette on the regions +- `noise`, truth = a second palette on the same regions, guide_lo and src = the fit's own tables on
    their bytes (src +- src_noise after that)."""
    fit = fit_module(pkg)
    gen = torch.Generator().manual_seed(20250307 + seed)
    reg = regions(B, T, plan.H, plan.W, gen)
    hi = GUIDE_PALETTE[reg] + torch.randint(-noise, noise + 1, reg.shape + (3,), generator=gen, dtype=torch.int32)
    hi = hi.clamp(0, 255).to(torch.uint8)
    pal = torch.randint(0, 256, (B, REGIONS, 3), generator=gen, dtype=torch.int32)
    truth = torch.stack([pal[b][reg[b]] for b in range(B)]).to(torch.uint8)
    down = dataclasses.replace(fit.plan_guide_lo(plan), T=T)
    lo, src = fit.restore_frames(hi, down), fit.restore_frames(truth, down).to(torch.int32)
    if src_noise:
        src = src + torch.randint(-src_noise, src_noise + 1, src.shape, generator=gen, dtype=torch.int32)
    return hi, lo, truth, src.clamp(0, 255).to(torch.uint8)


# ----------------------------------------------------------------------------------------------- float64 reference
def reference64(src, gplan, guide_hi, guide_lo, t0=0):
    """uint8 inputs -> float64 [B, T, H, W, 3] on the 0..255 scale, no rounding.  Dense tap matrices; walked by SOURCE row h: the
    output rows that read it (the nonzeros of the matrix's column), and per block of 32 output columns every source column
    between the first and the last that the block's rows of the matrix touch."""
    T = gplan.T
    B, Bg = src.shape[0], guide_hi.shape[0]
    my, mx = dense(gplan.y_lo_n, gplan.y_w, gplan.H_model), dense(gplan.x_lo_n, gplan.x_w, gplan.W_model)
    tab = gplan.tab.double()
    G = guide_hi[:, t0:t0 + T].long().expand(B, -1, -1, -1, -1) if Bg == 1 else guide_hi[:, t0:t0 + T].long()
    lo = guide_lo[:, t0:t0 + T].long().expand(B, -1, -1, -1, -1) if Bg == 1 else guide_lo[:, t0:t0 + T].long()
    s = src[:, :T].double()
    num = torch.zeros(B, T, gplan.H, gplan.W, 3, dtype=torch.float64)
    den = torch.zeros(B, T, gplan.H, gplan.W, dtype=torch.float64)
    for h in range(gplan.H_model):
        ys = my[:, h].nonzero().flatten()
        if not len(ys):
            continue
        y0, y1 = int(ys[0]), int(ys[-1]) + 1                       # (a band: zeros inside it weigh nothing)
        for x0 in range(0, gplan.W, 32):
            x1 = min(x0 + 32, gplan.W)
            ws = mx[x0:x1].abs().sum(dim=0).nonzero().flatten()
            w0, w1 = int(ws[0]), int(ws[-1]) + 1
            d = (G[:, :, y0:y1, x0:x1, None, :] - lo[:, :, h, None, None, w0:w1, :]).abs()         # [B, T, ny, nx, nw, 3]
            r = tab[d].prod(dim=-1) + float(gplan.eps)
            wgt = my[y0:y1, h].view(1, 1, -1, 1, 1) * mx[x0:x1, w0:w1].view(1, 1, 1, x1 - x0, w1 - w0) * r
            num[:, :, y0:y1, x0:x1] += torch.einsum("btyxw,btwc->btyxc", wgt, s[:, :, h, w0:w1])
            den[:, :, y0:y1, x0:x1] += wgt.sum(dim=-1)
    return num / den.unsqueeze(-1)


def taps64(c, guide=True, eps=None, channels=(0, 1, 2), signed=False, divide=True, t0=None, batch0=False, swap=False):
    """The operator tap by tap in float64 with a switch per way of getting it wrong (the stand-ins below)."""
    p = c["gplan"]
    T, t0 = p.T, c["t0"] if t0 is None else t0
    B, Bg = c["src"].shape[0], c["hi"].shape[0]
    pick = (lambda g: g[:1].expand(B, -1, -1, -1, -1)) if (Bg == 1 or batch0) else (lambda g: g)
    G, lo = pick(c["hi"][:, t0:t0 + T].long()), pick(c["lo"][:, t0:t0 + T].long())
    s = c["src"][:, :T].double()
    tab = p.tab.double()
    tabs = [(p.y_lo_n, p.y_w.double(), p.H_model), (p.x_lo_n, p.x_w.double(), p.W_model)]
    if swap:            # each axis with the other's table, cut or padded to its own length
        def fitted(t, n_out, n_in):
            lo_n, w = t[0], t[1]
            idx = torch.arange(n_out).clamp_max(lo_n.shape[0] - 1)
            return lo_n[idx], w[idx], n_in
        tabs = [fitted(tabs[1], p.H, p.H_model), fitted(tabs[0], p.W, p.W_model)]
    (yl, yw, hm), (xl, xw, wm) = tabs
    eps = float(p.eps) if eps is None else eps
    num = den = 0.0
    for ky in range(yw.shape[1]):
        yi = (yl[:, 0].long() + ky).clamp(0, hm - 1)
        for kx in range(xw.shape[1]):
            xi = (xl[:, 0].long() + kx).clamp(0, wm - 1)
            d = G - lo[:, :, yi][:, :, :, xi]
            d = d & 255 if signed else d.abs()
            r = tab[d][..., list(channels)].prod(dim=-1) + eps if guide else torch.ones(d.shape[:-1], dtype=torch.float64)
            w = (yw[:, ky, None] * xw[None, :, kx] * r).unsqueeze(-1)
            num = num + w * s[:, :, yi][:, :, :, xi]
            den = den + w
    return num / den if divide else num


# ----------------------------------------------------------------------------------------------- cases
_CASES = {}


def _finish(pkg, name, gplan, src, hi, lo, t0, **more):
    fit = fit_module(pkg)
    ref64 = reference64(src, gplan, hi, lo, t0)
    spec32 = fit._restore_guided_torch(src, gplan, hi, lo, t0, rounded=False)
    return dict(name=name, gplan=gplan, src=src, hi=hi, lo=lo, t0=t0, ref64=ref64, spec32=spec32, spec=round_u8(spec32),
                e_ref=float((spec32.double() - ref64).abs().max()), **more)


def case(pkg, g, B=1, Bg=1, Ts=1, Td=1, Tg=1, t0=0):
    """One grid case, computed once: inputs, plan, the float64 reference, the fp32 specification before and after its rounding,
    E_ref.  Clip b of src shows the scene of guide clip b (clip 0 where Bg = 1) from frame t0 on."""
    key = (g, B, Bg, Ts, Td, Tg, t0)
    if key not in _CASES:
        plan, gplan = guided_plan(pkg, g, Td)
        plan = dataclasses.replace(plan, T=Tg)
        hi, lo, _, _ = scene(pkg, plan, Bg, Tg, seed=sum(g[1]))
        frames = (torch.arange(Ts) + t0).clamp_max(Tg - 1)
        srcs = []
        for b in range(B):          # a palette of its own per clip, on the regions of its guide clip
            _, _, _, s = scene(pkg, plan, Bg, Tg, seed=sum(g[1]), src_noise=6 + b)
            srcs.append(s[b if Bg == B else 0].index_select(0, frames).roll(b, dims=-1))
        _CASES[key] = _finish(pkg, f"{geometry_id(g)}_B{B}g{Bg}_T{Ts}to{Td}of{Tg}at{t0}", gplan, torch.stack(srcs), hi, lo, t0)
    return _CASES[key]


def grid(geometries=None):
    for g in (GEOMETRIES if geometries is None else geometries):
        for B, Bg in BATCHES:
            for Ts, Td, Tg, t0 in TIMES:
                yield g, B, Bg, Ts, Td, Tg, t0


def sweep_case(pkg):
    """guide_hi flat 0 (frame 0) and flat 255 (frame 1) against a guide_lo that takes every byte value in every channel, one
    channel at a time (the two others match guide_hi), at sigma 64: all 256 entries of the table are read in every channel and
    none is too small to move a byte."""
    if "sweep" not in _CASES:
        plan, gplan = guided_plan(pkg, SWEEP, 2, SWEEP_SIGMA)
        (hm, wm), (h, w) = SWEEP
        i = torch.arange(hm * wm)
        lo = torch.zeros(1, 2, hm * wm, 3, dtype=torch.uint8)
        lo[0, 1] = 255
        for f in range(2):
            lo[0, f][i, i % 3] = (i // 3 % 256).to(torch.uint8)
        lo = lo.view(1, 2, hm, wm, 3)
        hi = torch.zeros(1, 2, h, w, 3, dtype=torch.uint8)
        hi[0, 1] = 255
        for f, G in ((0, 0), (1, 255)):
            for ch in range(3):
                assert len(torch.unique((lo[0, f, :, :, ch].int() - G).abs())) == 256
        _CASES["sweep"] = _finish(pkg, "sweep", gplan, RR.source(1, 2, hm, wm, seed=91), hi, lo, 0)
    return _CASES["sweep"]


def fallback_case(pkg):
    """A guide that matches no tap (guide_hi 255, guide_lo 0: every table read is 0.0): r = eps everywhere, the spatial filter
    alone."""
    if "fallback" not in _CASES:
        g = GEOMETRIES[0]
        plan, gplan = guided_plan(pkg, g, 2)
        (hm, wm), (h, w) = g
        assert float(gplan.tab[255]) == 0.0
        hi = torch.full((1, 2, h, w, 3), 255, dtype=torch.uint8)
        lo = torch.zeros(1, 2, hm, wm, 3, dtype=torch.uint8)
        _CASES["fallback"] = _finish(pkg, "fallback", gplan, RR.source(1, 2, hm, wm, seed=92), hi, lo, 0)
    return _CASES["fallback"]


def flat_case(pkg):
    """256 frames, frame v of src filled with v, under a palette guide (one frame, repeated): -> (src, gplan, hi, lo)."""
    if "flat" not in _CASES:
        plan, gplan = guided_plan(pkg, FLAT, 256)
        hi, lo, _, _ = scene(pkg, dataclasses.replace(plan, T=1), 1, 1, seed=93)
        _CASES["flat"] = (RR.flat_clip(), gplan, hi.expand(1, 256, -1, -1, -1).contiguous(), lo.expand(1, 256, -1, -1, -1).contiguous())
    return _CASES["flat"]


def quality_scene(pkg, g=SCENE, sigma=SIGMA):
    """The piecewise-constant scene of the quality check: -> (src, gplan, hi, lo, truth, the plain way back's plan)."""
    fit = fit_module(pkg)
    plan, gplan = guided_plan(pkg, g, 1, sigma)
    hi, lo, truth, src = scene(pkg, plan, 1, 1, seed=94)
    return src, gplan, hi, lo, truth, fit.plan_restore(plan)


NAMED = {"sweep": sweep_case, "fallback": fallback_case}


# ----------------------------------------------------------------------------------------------- wrong stand-ins
def wrong_stand_ins():
    """name -> (the case it must fail at: f(pkg) -> case, f(case) -> uint8 a wrong kernel would give)."""
    def padded_pitch(c):
        good = round_u8(c["ref64"])
        B, T, H, W, _ = good.shape
        pitch = (W * 3 + 3) // 4 * 4
        rows = torch.zeros(B * T * H, pitch, dtype=torch.uint8)
        rows[:, :W * 3] = good.reshape(B * T * H, W * 3)
        return rows.reshape(-1)[:good.numel()].reshape(good.shape)

    def byte_late(c):
        return round_u8(c["ref64"]).reshape(-1).roll(1).reshape(c["ref64"].shape)

    def at(g, **kw):
        return lambda pkg: case(pkg, g, **kw)
    G0, G1, G2 = GEOMETRIES[0], GEOMETRIES[1], GEOMETRIES[2]
    return {
        "guide ignored": (at(G0), lambda c: round_u8(taps64(c, guide=False))),
        "eps dropped": (fallback_case, lambda c: round_u8(taps64(c, eps=0.0))),
        "one channel's table only": (sweep_case, lambda c: round_u8(taps64(c, channels=(0,)))),
        "signed instead of absolute difference": (sweep_case, lambda c: round_u8(taps64(c, signed=True))),
        "no division": (at(G0), lambda c: round_u8(taps64(c, divide=False))),
        "t0 ignored": (at(G0, Ts=3, Td=2, Tg=5, t0=2), lambda c: round_u8(taps64(c, t0=0))),
        "batch 0's guide for every clip": (at(G0, B=2, Bg=2), lambda c: round_u8(taps64(c, batch0=True))),
        "y and x tables swapped": (at(G1), lambda c: round_u8(taps64(c, swap=True))),
        "truncation instead of round half to even": (at(G0), lambda c: c["spec32"].floor().clamp(0, 255).to(torch.uint8)),
        "row pitch padded": (at(G2), padded_pitch),
        "a byte late": (at(G0), byte_late),
    }
