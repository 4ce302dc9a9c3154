"""Fit any clip to the model's grid (the nodes' opt-in `fit` input).

The tokenizer takes T = 8k + 1 frames and H, W that are multiples of 16 (8 for the tokenizer, times the DiT's 2 x 2 patches).
`plan_fit` decides, on the host, how a (T, H, W) clip gets there: a target size, a resize with the antialiased triangle filter of
`F.interpolate(mode="bilinear", antialias=True)` written out as per-axis tap tables, a centre crop OF THE RESIZED picture (so the
crop never cuts what the resize would have kept sharp), and a time index that repeats the last frame up to the next 8k + 1.
`fit_frames` applies a plan to ComfyUI frames [B, T, H, W, 3] fp32 in [0, 1] (or uint8, a byte i standing for i / 255) and returns the model's [B, 3, T', H', W'] bf16 in
[-1, 1]: resample, crop, pad, `* 2 - 1`, round, transpose.  Its torch backend is the specification and what CPU devices run;
on a GPU one launch of drn_fit_frames or, from uint8, drn_fit_frames_u8 (one kernel template, csrc/fit.hip) does all of it.  At scale 1 on both axes (identity or pure crop) both
backends give the bits of today's ingest, `(image.permute(0, 4, 1, 2, 3) * 2 - 1).to(bf16)`, on the cropped frames.

The way back (the nodes' `fit_restore`): `plan_restore` turns the plan of a fit that kept the whole picture round, and
`restore_frames` resamples the pipeline's uint8 outputs [B, T', H', W', 3] to the source's [B, T, H, W, 3] with the same filter -
the torch backend again the specification, on a GPU one launch of drn_restore_frames_u8 (csrc/restore.hip).  The three kernels share csrc/resample_core.h.

The guided way back (the nodes' `restore_guide`): `plan_restore_guided` widens the way back's spatial tables and adds
a range table, and `restore_frames_guided` weights every tap again by how close the full-size source pixel is to the fitted source
at that tap (joint bilateral upsampling) - torch the specification, on a GPU one launch of drn_restore_guided_u8
(csrc/restore_guided.hip, on the same core).
"""
import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

GRID = 16          # H, W granularity of the model: 8 (tokenizer) x 2 (DiT patch)
MAX_TAPS = 32      # per axis; a down-scale beyond about 15x is refused (drn_fit_frames: Ky, Kx in 1..32)
MODES = ("crop", "stretch")


@dataclass
class FitPlan:
    mode: str
    T: int              # source frames: callers return the first T output frames
    H: int
    W: int
    T_out: int          # T'
    H_out: int          # H'
    W_out: int          # W'
    H_full: int         # the resized size the crop is cut from (stretch: the target itself)
    W_full: int
    y0: int
    x0: int
    t_idx: torch.Tensor     # int32 [T']: source frame of every output frame
    y_lo_n: torch.Tensor    # int32 [H', 2]: first source row and tap count of every output row
    y_w: torch.Tensor       # float32 [H', Ky]: its weights, zero-padded
    x_lo_n: torch.Tensor
    x_w: torch.Tensor
    identity: bool

    @property
    def scale1_y(self) -> bool:
        return self.H_full == self.H

    @property
    def scale1_x(self) -> bool:
        return self.W_full == self.W


def axis_taps(n_in: int, n_full: int, off: int, n_out: int, reach: float = 1.0):
    """Tap table of output samples off .. off + n_out - 1 of an axis resized from n_in to n_full samples, in the arithmetic of
    torch's antialiased bilinear resize: -> (lo_n int32 [n_out, 2], w float64 [n_out, K]).  Rows sum to 1 (normalised in
    float64), taps of weight exactly 0 are dropped, the rest of a row is zero padding.  reach: the triangle's support widened by
    this factor (1.0: torch's own, the same tables bit for bit; the guided way back takes 2.0)."""
    scale = n_in / n_full
    support = max(scale, 1.0) * reach
    i = np.arange(off, off + n_out, dtype=np.float64)
    c = scale * (i + 0.5)
    lo = np.maximum(0, (c - support + 0.5).astype(np.int64))          # the cast truncates, like torch's
    hi = np.minimum((c + support + 0.5).astype(np.int64), n_in)
    span = int((hi - lo).max())
    j = lo[:, None] + np.arange(span, dtype=np.int64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((j - c[:, None] + 0.5) / support))
    w[j >= hi[:, None]] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    nz = w != 0.0
    first = nz.argmax(axis=1)
    last = span - 1 - nz[:, ::-1].argmax(axis=1)
    n = last - first + 1
    K = int(n.max())
    cols = first[:, None] + np.arange(K)[None, :]
    out = np.where(cols <= last[:, None], np.take_along_axis(w, np.minimum(cols, span - 1), axis=1), 0.0)
    lo_n = np.stack([lo + first, n], axis=1).astype(np.int32)
    return lo_n, out


def _single(lo_n, w, n_in) -> bool:
    """An axis table that copies its n_in samples: one tap of weight 1.0 per output sample, in place."""
    return w.shape[1] == 1 and len(lo_n) == n_in and bool((lo_n[:, 0] == np.arange(n_in)).all()) and bool((w == 1.0).all())


def _target(side: int, given: int, name: str) -> int:
    if given:
        if given < 0 or given % GRID:
            raise ValueError(f"fit_{name} must be a positive multiple of {GRID} (or 0 = the source rounded down), got {given}")
        return int(given)
    if side < GRID:
        raise ValueError(f"a source {name} of {side} is below the model's grid of {GRID}")
    return side // GRID * GRID


def plan_fit(T: int, H: int, W: int, mode: str, height: int = 0, width: int = 0, windowed: bool = False) -> FitPlan:
    """How a clip of T frames of H x W reaches the model's grid.  mode 'stretch': the whole picture resampled to the target;
    'crop': resized to cover the target, then centre-cropped (both targets 0: a pure centre crop at scale 1).  height / width:
    the target, multiples of 16; 0 = that side of the source rounded down to one.  windowed: the clip will be rendered in
    windows of 8k + 1 frames, which take any T, so no frames are added."""
    if mode not in MODES:
        raise ValueError(f"fit mode must be one of {MODES}, got {mode!r}")
    if T < 1 or H < 1 or W < 1:
        raise ValueError(f"empty clip: T, H, W = {T}, {H}, {W}")
    H_out, W_out = _target(H, height, "height"), _target(W, width, "width")
    if mode == "stretch":
        H_full, W_full = H_out, W_out
    else:
        s = 1.0 if not height and not width else max(H_out / H, W_out / W)
        H_full = max(H_out, int(math.floor(H * s + 0.5)))
        W_full = max(W_out, int(math.floor(W * s + 0.5)))
    y0, x0 = (H_full - H_out) // 2, (W_full - W_out) // 2
    y_lo_n, y_w = axis_taps(H, H_full, y0, H_out)
    x_lo_n, x_w = axis_taps(W, W_full, x0, W_out)
    for name, w in (("height", y_w), ("width", x_w)):
        if w.shape[1] > MAX_TAPS:
            raise ValueError(f"the {name} down-scale needs {w.shape[1]} taps per output sample; at most {MAX_TAPS} are supported")
    T_out = T if (T - 1) % 8 == 0 or windowed else (T - 1) // 8 * 8 + 9
    t_idx = np.minimum(np.arange(T_out), T - 1).astype(np.int32)
    identity = T_out == T and _single(y_lo_n, y_w, H) and _single(x_lo_n, x_w, W)
    return FitPlan(mode, T, H, W, T_out, H_out, W_out, H_full, W_full, y0, x0, torch.from_numpy(t_idx),
                   torch.from_numpy(y_lo_n), torch.from_numpy(y_w.astype(np.float32)),
                   torch.from_numpy(x_lo_n), torch.from_numpy(x_w.astype(np.float32)), identity)


@dataclass
class RestorePlan:
    T: int                  # frames to return: the source clip's own length (the time padding is cut)
    H_model: int            # the size the outputs arrive in: the fit's H', W'
    W_model: int
    H: int                  # the size they leave in: the source's
    W: int
    y_lo_n: torch.Tensor    # int32 [H, 2], float32 [H, Ky]: the tables of axis_taps(H', H, 0, H)
    y_w: torch.Tensor
    x_lo_n: torch.Tensor
    x_w: torch.Tensor
    identity: bool          # both axes single taps of weight 1.0: restore_frames only cuts in time


def plan_restore(plan: FitPlan) -> RestorePlan:
    """The way back of a fit that kept the whole picture ('stretch', or a 'crop' that cut nothing): the model-size uint8 outputs
    resampled to the source's H x W with the same antialiased triangle filter, and cut to its T frames.  A crop that cut cannot
    be undone: ValueError."""
    whole = plan.mode == "stretch" or (plan.y0 == 0 and plan.x0 == 0 and plan.H_full == plan.H_out and plan.W_full == plan.W_out)
    if not whole:
        raise ValueError(f"a crop cannot be undone: this fit cut {plan.H_full} x {plan.W_full} down to {plan.H_out} x {plan.W_out}, "
                         "so the outputs cannot be restored to the source size; use fit = 'stretch' (or fit_restore off)")
    y_lo_n, y_w = axis_taps(plan.H_out, plan.H, 0, plan.H)
    x_lo_n, x_w = axis_taps(plan.W_out, plan.W, 0, plan.W)
    for name, w in (("height", y_w), ("width", x_w)):
        if w.shape[1] > MAX_TAPS:
            raise ValueError(f"restoring the {name} needs {w.shape[1]} taps per output sample; at most {MAX_TAPS} are supported")
    identity = _single(y_lo_n, y_w, plan.H_out) and _single(x_lo_n, x_w, plan.W_out)
    return RestorePlan(plan.T, plan.H_out, plan.W_out, plan.H, plan.W,
                       torch.from_numpy(y_lo_n), torch.from_numpy(y_w.astype(np.float32)),
                       torch.from_numpy(x_lo_n), torch.from_numpy(x_w.astype(np.float32)), identity)


def _taps_torch(x, dim, lo_n, w):
    """One axis of the specification: the plan's fp32 table applied tap by tap, k = 0 .. K - 1, an index_select and a
    multiply-add each.  Padded taps have weight 0 and an index held inside the axis."""
    lo = lo_n[:, 0].to(device=x.device, dtype=torch.long)
    w = w.to(x.device)
    shape = [1] * x.ndim
    shape[dim] = -1
    acc = None
    for k in range(w.shape[1]):
        term = x.index_select(dim, (lo + k).clamp_max(x.shape[dim] - 1)) * w[:, k].reshape(shape)
        acc = term if acc is None else acc + term
    return acc


def _restore_torch(u8, rplan: RestorePlan, rounded=True):
    """The specification: fp32 on the 0..255 scale, the horizontal pass, then the vertical one, round half to even, clamp."""
    x = u8[:, :rplan.T].to(torch.float32)
    x = _taps_torch(x, 3, rplan.x_lo_n, rplan.x_w)
    x = _taps_torch(x, 2, rplan.y_lo_n, rplan.y_w)
    return x.round().clamp(0.0, 255.0).to(torch.uint8) if rounded else x


def restore_frames(u8: torch.Tensor, rplan: RestorePlan, backend: str = "auto") -> torch.Tensor:
    """uint8 [B, T', H', W', 3] at the model's size -> uint8 [B, T, H, W, 3] at the source's, frames 0 .. T - 1, on the same
    device.  backend: 'auto' = the HIP kernel (drn_restore_frames_u8) on a GPU tensor and torch on a CPU tensor; 'torch' / 'hip'
    force a path ('hip' needs a GPU tensor).  An identity plan launches nothing: the input, cut in time.  Normal maps are
    resampled like any picture and not renormalised."""
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    if u8.dtype != torch.uint8 or u8.ndim != 5 or u8.shape[-1] != 3:
        raise ValueError(f"restore needs uint8 [B, T, H, W, 3] frames, got {u8.dtype} {tuple(u8.shape)}")
    if tuple(u8.shape[2:4]) != (rplan.H_model, rplan.W_model) or u8.shape[1] < rplan.T:
        raise ValueError(f"the plan was made for at least {rplan.T} frames of {(rplan.H_model, rplan.W_model)}, "
                         f"got {tuple(u8.shape[1:4])}")
    if backend == "hip" and not u8.is_cuda:
        raise ValueError(f"backend='hip' needs a GPU tensor, got one on {u8.device} (the torch path is what CPU devices run)")
    if rplan.identity:
        return u8[:, :rplan.T]
    if backend == "torch" or not u8.is_cuda:
        return _restore_torch(u8, rplan)
    from . import native
    return native.restore_frames(u8.contiguous(), rplan.T, rplan.y_lo_n, rplan.y_w, rplan.x_lo_n, rplan.x_w)


# ----------------------------------------------------------------------------------------------- the guided way back
GUIDED_MAX_TAPS = 8       # per axis (drn_restore_guided_u8: Ky, Kx in 1..8)
GUIDED_REACH = 2.0        # the spatial support: max(scale, 1) * 2, four taps per axis when up-scaling
GUIDED_EPS = 2.0 ** -10   # the floor of the range term: the denominator stays positive


@dataclass
class GuidedPlan:
    T: int                  # frames to return
    H_model: int            # the size the outputs arrive in: the fit's H', W'
    W_model: int
    H: int                  # the size they leave in: the source's
    W: int
    y_lo_n: torch.Tensor    # int32 [H, 2], float32 [H, Ky]: the tables of axis_taps(H', H, 0, H, reach)
    y_w: torch.Tensor
    x_lo_n: torch.Tensor
    x_w: torch.Tensor
    tab: torch.Tensor       # float32 [256]: exp(-d^2 / (2 sigma^2)) of a byte difference d, float64 rounded once
    eps: float
    sigma: float


def range_table(sigma: float) -> torch.Tensor:
    """The range term of one channel by byte difference d = 0 .. 255: exp(-d^2 / (2 sigma^2)) in float64, rounded to fp32 once.
    The product over the three channels is the Gaussian of the colour distance."""
    d = np.arange(256, dtype=np.float64)
    return torch.from_numpy(np.exp(-d * d / (2.0 * float(sigma) ** 2)).astype(np.float32))


def plan_restore_guided(plan: FitPlan, sigma: float, reach: float = GUIDED_REACH) -> GuidedPlan:
    """The guided way back of a fit that kept the whole picture (joint bilateral upsampling, Kopf et al. 2007): the spatial tables
    of `plan_restore` with the support widened by `reach` - the filter then gets past the one mixed pixel every low-resolution
    edge has -, the range table of `sigma` (in levels of 255) and the floor.  ValueError where `plan_restore` refuses, for more
    than 8 taps on an axis and for sigma <= 0."""
    if not sigma > 0:
        raise ValueError(f"restore_sigma must be positive, got {sigma}")
    plan_restore(plan)                  # a crop that cut cannot be undone
    y_lo_n, y_w = axis_taps(plan.H_out, plan.H, 0, plan.H, reach)
    x_lo_n, x_w = axis_taps(plan.W_out, plan.W, 0, plan.W, reach)
    for name, w in (("height", y_w), ("width", x_w)):
        if w.shape[1] > GUIDED_MAX_TAPS:
            raise ValueError(f"the guided restore of the {name} needs {w.shape[1]} taps per output sample; at most "
                             f"{GUIDED_MAX_TAPS} are supported (restore_guide = 'off' takes up to {MAX_TAPS})")
    return GuidedPlan(plan.T, plan.H_out, plan.W_out, plan.H, plan.W,
                      torch.from_numpy(y_lo_n), torch.from_numpy(y_w.astype(np.float32)),
                      torch.from_numpy(x_lo_n), torch.from_numpy(x_w.astype(np.float32)), range_table(sigma), GUIDED_EPS, float(sigma))


def plan_guide_lo(plan: FitPlan) -> RestorePlan:
    """The source as the model saw it, as a plan for `restore_frames`: the fit's own spatial tables applied to the source's bytes
    (bytes by tap tables, round half to even), frames 0 .. T - 1.  For fits that kept the whole picture, as `plan_restore`."""
    plan_restore(plan)
    return RestorePlan(plan.T, plan.H, plan.W, plan.H_out, plan.W_out, plan.y_lo_n, plan.y_w, plan.x_lo_n, plan.x_w,
                       _single(plan.y_lo_n.numpy(), plan.y_w.numpy(), plan.H) and _single(plan.x_lo_n.numpy(), plan.x_w.numpy(), plan.W))


def _restore_guided_torch(u8, gplan: GuidedPlan, guide_hi, guide_lo, t0=0, rounded=True):
    """The specification: fp32 on the 0..255 scale, tap by tap, ky outer and kx inner; per tap the range term from the table, the
    weight, a multiply-add per channel and one for the denominator; one division, round half to even, clamp."""
    T = gplan.T
    dev = u8.device
    src = u8[:, :T].to(torch.float32)
    lo = guide_lo[:, t0:t0 + T]
    G = guide_hi[:, t0:t0 + T].to(torch.int16)
    tab = gplan.tab.to(dev)
    eps = torch.tensor(gplan.eps, dtype=torch.float32, device=dev)
    ylo, xlo = (t[:, 0].to(device=dev, dtype=torch.long) for t in (gplan.y_lo_n, gplan.x_lo_n))
    yw, xw = gplan.y_w.to(dev), gplan.x_w.to(dev)
    num = den = None
    for ky in range(yw.shape[1]):
        yi = (ylo + ky).clamp_max(gplan.H_model - 1)
        for kx in range(xw.shape[1]):
            xi = (xlo + kx).clamp_max(gplan.W_model - 1)
            d = (G - lo[:, :, yi][:, :, :, xi].to(torch.int16)).abs().long()
            t = tab[d]
            r = t[..., 0] * t[..., 1] * t[..., 2] + eps
            w = ((yw[:, ky, None] * xw[None, :, kx]) * r).unsqueeze(-1)          # padded taps: weight 0
            term = w * src[:, :, yi][:, :, :, xi]
            num = term if num is None else num + term
            den = w if den is None else den + w
    x = num / den
    return x.round().clamp(0.0, 255.0).to(torch.uint8) if rounded else x


def restore_frames_guided(u8: torch.Tensor, gplan: GuidedPlan, guide_hi: torch.Tensor, guide_lo: torch.Tensor, t0: int = 0,
                          backend: str = "auto") -> torch.Tensor:
    """uint8 [B, T', H', W', 3] at the model's size -> uint8 [B, T, H, W, 3] at the source's, frames 0 .. T - 1, with the source
    as a guide: guide_hi [Bg, Tg, H, W, 3] the source picture, guide_lo [Bg, Tg, H', W', 3] the source as the model saw it
    (`plan_guide_lo`), both uint8 on u8's device, Bg 1 or B; output frame t reads guide frames t0 + t.  backend: 'auto' = the HIP
    kernel (drn_restore_guided_u8: 2.3 ms against the torch path's 150 ms at 57 x 1080 x 1920, profiles/restore_guided.txt) on a GPU tensor and torch
    on a CPU tensor; 'torch' / 'hip' force a path ('hip' needs a GPU tensor).  Normal maps are not renormalised."""
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    for name, t in (("frames", u8), ("guide_hi", guide_hi), ("guide_lo", guide_lo)):
        if t.dtype != torch.uint8 or t.ndim != 5 or t.shape[-1] != 3:
            raise ValueError(f"the guided restore needs uint8 [B, T, H, W, 3] {name}, got {t.dtype} {tuple(t.shape)}")
        if t.device != u8.device:
            raise ValueError(f"{name} is on {t.device}, the frames on {u8.device}")
    if tuple(u8.shape[2:4]) != (gplan.H_model, gplan.W_model) or u8.shape[1] < gplan.T:
        raise ValueError(f"the plan was made for at least {gplan.T} frames of {(gplan.H_model, gplan.W_model)}, "
                         f"got {tuple(u8.shape[1:4])}")
    Bg, Tg = guide_hi.shape[:2]
    if tuple(guide_hi.shape[2:4]) != (gplan.H, gplan.W) or tuple(guide_lo.shape) != (Bg, Tg, gplan.H_model, gplan.W_model, 3):
        raise ValueError(f"the plan needs guides of {(gplan.H, gplan.W)} and {(gplan.H_model, gplan.W_model)} with the same clips "
                         f"and frames, got {tuple(guide_hi.shape)} and {tuple(guide_lo.shape)}")
    if Bg not in (1, u8.shape[0]):
        raise ValueError(f"{Bg} guide clips for {u8.shape[0]} clips: one for all, or one each")
    if t0 < 0 or t0 + gplan.T > Tg:
        raise ValueError(f"frames {t0} .. {t0 + gplan.T - 1} are outside the guide's {Tg}")
    if backend == "hip" and not u8.is_cuda:
        raise ValueError(f"backend='hip' needs a GPU tensor, got one on {u8.device} (the torch path is what CPU devices run)")
    if backend == "torch" or not u8.is_cuda:
        return _restore_guided_torch(u8, gplan, guide_hi, guide_lo, t0)
    from . import native
    return native.restore_guided(u8.contiguous(), guide_lo.contiguous(), guide_hi.contiguous(), gplan.T, gplan.y_lo_n, gplan.y_w,
                                 gplan.x_lo_n, gplan.x_w, gplan.tab, gplan.eps, t0=int(t0))


@dataclass
class RestoreGuide:
    """What the pipeline's `restore_guide` holds: the plan and the two guides, on the pipeline's device."""
    plan: GuidedPlan
    hi: torch.Tensor        # uint8 [Bg, T, H, W, 3]: the source picture
    lo: torch.Tensor        # uint8 [Bg, T, H', W', 3]: the source as the model saw it


def source_guide(plan: FitPlan, image_5d: torch.Tensor, sigma: float, device) -> RestoreGuide:
    """The source clip [B, T, H, W, 3] as the guide of its fit's way back.  uint8 frames are used as they are; fp32 ones in [0, 1]
    become bytes on `device`, once; guide_lo is `restore_frames` under `plan_guide_lo`."""
    gplan = plan_restore_guided(plan, sigma)
    if image_5d.ndim != 5 or image_5d.shape[-1] != 3 or tuple(image_5d.shape[1:4]) != (plan.T, plan.H, plan.W):
        raise ValueError(f"the plan was made for {(plan.T, plan.H, plan.W)} frames, got {tuple(image_5d.shape)}")
    hi = image_5d.to(device)
    if hi.dtype != torch.uint8:
        hi = (hi.to(torch.float32) * 255.0).round().clamp(0, 255).to(torch.uint8)
    hi = hi.contiguous()
    return RestoreGuide(gplan, hi, restore_frames(hi, plan_guide_lo(plan)).contiguous())


# a source byte i enters the fit as fp32(i) / 255, correctly rounded: the true division, done once on the CPU.  (i * (1 / 255) in
# fp32 differs from it at 126 of the 256 values; the kernel builds the same table with a correctly rounded division.)
U8_UNIT = torch.arange(256, dtype=torch.float32) / 255.0


def u8_unit(u8: torch.Tensor) -> torch.Tensor:
    """uint8 frames -> the fp32 frames they stand for, `u8.float() / 255.0` as the CPU computes it, by table lookup: the same
    bits on any device (no division on the device)."""
    if u8.dtype != torch.uint8:
        raise ValueError(f"u8_unit needs uint8, got {u8.dtype}")
    return U8_UNIT.to(u8.device)[u8.long()]


def _fit_torch(image_5d, plan: FitPlan, device, round_bf16=True):
    """The specification: gather frames, antialiased resize, crop slice, * 2 - 1, bf16.  An axis at scale 1 is sliced, not
    interpolated, so a pure crop is a copy."""
    x = image_5d.to(device=device, dtype=torch.float32).permute(0, 4, 1, 2, 3)
    x = x.index_select(2, plan.t_idx.to(device=x.device, dtype=torch.long))
    B = x.shape[0]
    x = x.permute(0, 2, 1, 3, 4).reshape(B * plan.T_out, 3, plan.H, plan.W)
    if plan.scale1_y:
        x = x[:, :, plan.y0:plan.y0 + plan.H_out]
    if plan.scale1_x:
        x = x[:, :, :, plan.x0:plan.x0 + plan.W_out]
    if not (plan.scale1_y and plan.scale1_x):
        size = (plan.H_out if plan.scale1_y else plan.H_full, plan.W_out if plan.scale1_x else plan.W_full)
        x = F.interpolate(x.contiguous(), size=size, mode="bilinear", antialias=True, align_corners=False)
        if not plan.scale1_y:
            x = x[:, :, plan.y0:plan.y0 + plan.H_out]
        if not plan.scale1_x:
            x = x[:, :, :, plan.x0:plan.x0 + plan.W_out]
    x = x.reshape(B, plan.T_out, 3, plan.H_out, plan.W_out).permute(0, 2, 1, 3, 4) * 2.0 - 1.0
    return x.to(torch.bfloat16).contiguous() if round_bf16 else x.contiguous()


def fit_frames(image_5d: torch.Tensor, plan: FitPlan, device, backend: str = "auto") -> torch.Tensor:
    """[B, T, H, W, 3] fp32 in [0, 1], or uint8 (a byte i standing for i / 255, `u8_unit`), on the host or on a device ->
    [B, 3, T', H', W'] bf16 in [-1, 1] on `device`.  backend: 'auto' = the HIP kernel (drn_fit_frames, for uint8 frames
    drn_fit_frames_u8: the bytes are what is uploaded) on a GPU device and torch on a CPU device; 'torch' / 'hip' force a path
    ('hip' needs a GPU device).  The torch path on uint8 frames is `u8_unit`, then the fp32 specification."""
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    if image_5d.ndim != 5 or image_5d.shape[-1] != 3:
        raise ValueError(f"fit needs [B, T, H, W, 3] frames, got {tuple(image_5d.shape)}")
    if image_5d.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"fit needs float32 or uint8 frames, got {image_5d.dtype}")
    if tuple(image_5d.shape[1:4]) != (plan.T, plan.H, plan.W):
        raise ValueError(f"the plan was made for {(plan.T, plan.H, plan.W)} frames, got {tuple(image_5d.shape[1:4])}")
    on_gpu = torch.device(device).type == "cuda"
    if backend == "hip" and not on_gpu:
        raise ValueError(f"backend='hip' needs a GPU device, got {device!r} (the torch path is what CPU devices run)")
    u8 = image_5d.dtype == torch.uint8
    if backend == "torch" or not on_gpu:
        return _fit_torch(u8_unit(image_5d) if u8 else image_5d, plan, device)
    from . import native
    if u8:
        src = image_5d.to(device=device).contiguous()
        return native.fit_frames_u8(src, plan.t_idx, plan.y_lo_n, plan.y_w, plan.x_lo_n, plan.x_w)
    src = image_5d.to(device=device, dtype=torch.float32).contiguous()
    return native.fit_frames(src, plan.t_idx, plan.y_lo_n, plan.y_w, plan.x_lo_n, plan.x_w)
