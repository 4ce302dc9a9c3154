"""Window schedule of a long clip ("Long clips").  Pure host arithmetic: no tensors, no device work.

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


def ramp_weights(overlap: int) -> np.ndarray:
    """fp32 [overlap]: w[j] = float32((j + 1) / (overlap + 1)), the weight of the NEW window at ramp frame j (the predecessor
    has 1 - w).  Strictly inside (0, 1): neither window's frame is ever copied, the join has no seam on either side."""
    if isinstance(overlap, bool) or not isinstance(overlap, (int, np.integer)) or overlap < 0:
        raise ValueError(f"window_overlap must be a non-negative integer, got {overlap!r}")
    return np.array([(j + 1) / (overlap + 1) for j in range(int(overlap))], dtype=np.float32)
