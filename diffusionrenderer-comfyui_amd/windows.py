"""Window schedule of a long clip ("Long clips"), pure host arithmetic, and the specification of `window_align`
(align_affine / apply_affine below: torch and numpy, on whatever device the tensors live; the GPU path is csrc/window_align.hip).

The renderer is trained on 57-frame clips; a longer video is cut into windows of that one length which overlap by
`overlap` frames and are joined in PIXEL space, where the decoded frames become uint8 (drn_postprocess_window_u8).  The
tokenizer is causal - latent frame 0 of a window encodes one pixel frame, every later one eight - so two windows' latents of
the same pixel frames are different quantities and are never averaged.

Every window has the full length (one model config, one launch plan, one start-noise shape): the last one is shifted back
instead of being cut short, and its frames in front of the join are computed and thrown away - the predecessor alone supplies
them.
"""
from typing import List, NamedTuple

import numpy as np
import torch


class Window(NamedTuple):
    start: int        # global frame of the window's frame 0
    ramp_at: int      # window-local first frame of the cross-fade with the predecessor (0, and no ramp, for window 0)
    write_lo: int     # window-local half-open range of the frames this window writes ...
    write_hi: int
    out_at: int       # ... and the global frame where that range lands


def _check(window_frames, overlap):
    for name, v in (("window_frames", window_frames), ("window_overlap", overlap)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if window_frames < 9 or (window_frames - 1) % 8:
        raise ValueError(f"window_frames must be 8k + 1 and at least 9 (the tokenizer packs 1 + 8k frames), got {window_frames}")
    if not 0 <= overlap <= (window_frames - 1) // 2:
        raise ValueError(f"window_overlap must lie in [0, {(window_frames - 1) // 2}] for window_frames {window_frames} (a frame "
                         f"is covered by the ramps of at most two windows), got {overlap}")


def plan_windows(T: int, window_frames: int, overlap: int) -> List[Window]:
    """The windows of a T-frame clip, in order.  T <= window_frames: one window [0, T) (the caller's unwindowed path).

    Otherwise stride = window_frames - overlap, n = ceil((T - overlap) / stride) windows start at i * stride, the last at
    T - window_frames.  Window i > 0 meets window i - 1 over exactly the predecessor's last `overlap` frames; it writes from that
    ramp on, up to its own last `overlap` frames (the carry handed to the next window) - the last window up to its end."""
    _check(window_frames, overlap)
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 1:
        raise ValueError(f"a clip has at least one frame, got T = {T!r}")
    Wf, O = int(window_frames), int(overlap)
    T = int(T)
    if T <= Wf:
        return [Window(0, 0, 0, T, 0)]
    stride = Wf - O
    n = -(-(T - O) // stride)
    starts = [i * stride for i in range(n - 1)] + [T - Wf]
    plan = []
    for i, s in enumerate(starts):
        ramp_at = 0 if i == 0 else starts[i - 1] + Wf - O - s
        plan.append(Window(s, ramp_at, ramp_at, Wf if i == n - 1 else Wf - O, s + ramp_at))
    return plan


def check_window_align(window_align, window_frames, window_overlap, tile_height=0, tile_width=0):
    """ValueError for a `window_align` that cannot be honoured, from settings alone (so before any GPU work).  Without windows
    (window_frames = 0) there is nothing to align and nothing to refuse."""
    if not (window_align and window_frames):
        return
    if not window_overlap:
        raise ValueError("window_align needs window_overlap >= 1: the overlap is where two windows describe the same frames")
    if tile_height or tile_width:
        raise ValueError("window_align with tiles is not implemented (a gain per tile and window would make the tiles disagree): "
                         "set tile_height = tile_width = 0")


def ramp_weights(overlap: int) -> np.ndarray:
    """fp32 [overlap]: w[j] = float32((j + 1) / (overlap + 1)), the weight of the NEW window at ramp frame j (the predecessor
    has 1 - w).  Strictly inside (0, 1): neither window's frame is ever copied, the join has no seam on either side."""
    if isinstance(overlap, bool) or not isinstance(overlap, (int, np.integer)) or overlap < 0:
        raise ValueError(f"window_overlap must be a non-negative integer, got {overlap!r}")
    return np.array([(j + 1) / (overlap + 1) for j in range(int(overlap))], dtype=np.float32)


# ----------------------------------------------------------------------------------------------- windows that agree
# Two windows are independent samples: the cross-fade hides the seam, not the disagreement in level and contrast.  The one place
# where both describe the same frames is the overlap, so the new window's first two moments are matched to the carry's there
# (gain compensation of panorama stitching, mean / std colour transfer) before the cross-fade.  One (g, o) for the three channels:
# hue and neutral greys survive.
ALIGN_FLAT_VAR = 2.0 ** -20          # a flat overlap: a standard deviation under a quarter of a byte level (2 / 255 / 4 ~ 2^-9)
ALIGN_GAIN_MIN, ALIGN_GAIN_MAX = 0.5, 2.0


def align_solve(n, sum_a, sum_v, sum_aa, sum_vv, sum_av):
    """The rules, in float64, from the five sums of one pass's overlap -> ((g, o) as float64, not yet rounded to fp32, and the
    moments (n, mean_a, mean_v, var_a, var_v, cov)).  Population moments.  g = sqrt(var_a / var_v): moment matching, not the
    regression slope cov / var_v, which two noisy samples of one truth dilute below 1 (contrast would shrink window after window).
    g = 1 for a flat overlap (either variance below ALIGN_FLAT_VAR) or contents that disagree (cov <= 0); then clamped to
    [0.5, 2]; o = mean_a - g * mean_v with the clamped g.  Any non-finite moment: (1, 0)."""
    f = np.float64
    with np.errstate(all="ignore"):
        n = f(n)
        mean_a, mean_v = f(sum_a) / n, f(sum_v) / n
        var_a, var_v = f(sum_aa) / n - mean_a * mean_a, f(sum_vv) / n - mean_v * mean_v
        cov = f(sum_av) / n - mean_a * mean_v
        moments = (n, mean_a, mean_v, var_a, var_v, cov)
        if not all(np.isfinite(m) for m in moments):
            return (f(1.0), f(0.0)), moments
        g = f(1.0)
        if var_a >= ALIGN_FLAT_VAR and var_v >= ALIGN_FLAT_VAR and cov > 0:
            g = np.sqrt(var_a / var_v)
        g = min(max(g, f(ALIGN_GAIN_MIN)), f(ALIGN_GAIN_MAX))
        return (g, mean_a - g * mean_v), moments


def align_affine(video: torch.Tensor, prev_tail: torch.Tensor, ramp_at: int) -> torch.Tensor:
    """video [B,3,Tw,H,W] bf16 (the new window), prev_tail [B,3,O,H,W] bf16 (the carry, already in window 0's space) -> fp32
    [B, 2] = (g, o) per pass row, from the float64 moments over all 3 * O * H * W values of the carry and of the window's frames
    [ramp_at, ramp_at + O); each rounded to fp32 once."""
    B, O = prev_tail.shape[0], prev_tail.shape[2]
    if O < 1 or ramp_at < 0 or ramp_at + O > video.shape[2]:
        raise ValueError(f"the overlap [{ramp_at}, {ramp_at + O}) does not lie in a window of {video.shape[2]} frames")
    out = np.empty((B, 2), dtype=np.float32)
    for b in range(B):
        a = prev_tail[b].detach().cpu().to(torch.float64).numpy().reshape(-1)
        v = video[b, :, ramp_at:ramp_at + O].detach().cpu().to(torch.float64).numpy().reshape(-1)
        with np.errstate(all="ignore"):
            (g, o), _ = align_solve(a.size, a.sum(), v.sum(), (a * a).sum(), (v * v).sum(), (a * v).sum())
            out[b] = (np.float32(g), np.float32(o))
    return torch.from_numpy(out).to(video.device)


def apply_affine(video: torch.Tensor, affine: torch.Tensor) -> torch.Tensor:
    """Every value of the window -> bf16(fp32(g * x) + o) with its pass row's (g, o): two separately rounded fp32 operations,
    never an FMA.  Before the ramp blend, the normal blend and the clamp chain; the next carry is cut from the result."""
    g = affine[:, 0].to(torch.float32).view(-1, 1, 1, 1, 1)
    o = affine[:, 1].to(torch.float32).view(-1, 1, 1, 1, 1)
    return (video.to(torch.float32) * g + o).to(torch.bfloat16)
