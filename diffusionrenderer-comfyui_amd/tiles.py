"""Spatial tiles of a large picture.  The planner is pure host arithmetic; `blend_tile` joins one rendered tile
into the picture's canvas.

The renderer is trained at one picture size (576 x 1024); a larger picture is rendered as overlapping tiles of exactly
`tile_height x tile_width`, each on its own, and joined in PIXEL space where the results already lie as bytes on the device -
windows.py's scheme along H and W.  Every tile has the full size (one model config, one launch plan, one start-noise shape): the
last row and column of tiles are shifted back to end with the picture instead of being cut short, and what they computed in
front of the join is thrown away.  Tiles are independent samples, as windows are: they share the seed and the start noise and are
not conditioned on each other, so two tiles may disagree, and the cross-fade hides the seam, not the disagreement.

`blend_tile`'s torch backend is the specification and what CPU devices run; on a GPU one launch of drn_tile_blend_u8
(csrc/tile_blend.hip) does it.

That is the pipeline's `tile_join = "pixel"`.  With `tile_join = "latent"` the tiles are sampled JOINTLY instead:
one noisy latent canvas exists for the whole picture, at every Euler step each tile takes its crop of it through the DiT
(`latent_gather`) and its step result is cross-faded into the next canvas (`latent_step_join`: this file's blend rule on bf16),
so neighbouring tiles agree.  It rests on the tiles lying on the tokenizer's grid (`latent_tile`) and covering the canvas
(`covers`); the final canvas is decoded tile by tile and joined in pixel space as above.  Again the torch backends are the
specification, and on a GPU each is one launch (csrc/latent_tiles.hip).
"""
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from .windows import ramp_weights


class Span(NamedTuple):
    start: int        # global sample of the span's sample 0
    ramp_at: int      # span-local first sample this span writes; for every span but the first, the cross-fade starts here


class Tile(NamedTuple):
    y: int            # the tile's corner in the picture ...
    x: int
    h: int            # ... and its size
    w: int
    ry: int           # tile-local first row / column written (rows and columns in front are computed and discarded)
    rx: int
    Oy: int           # ramp lengths: the first Oy written rows / Ox written columns are cross-faded over the neighbour's
    Ox: int


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v)


def plan_axis(n: int, size: int, overlap: int, name: str = "size") -> List[Span]:
    """The spans of one axis of n samples, in order.  n <= size: one span (0, 0) of extent n.  Otherwise stride = size - overlap,
    count = ceil((n - overlap) / stride) spans of extent `size` start at i * stride, the last at n - size.  Span i writes its
    local range [ramp_at, size); for i > 0 that range starts where the predecessor's last `overlap` samples lie, and its first
    `overlap` samples are the ramp over them.  windows.plan_windows without the carry: a span writes up to its own end."""
    n, size, overlap = _int("n", n), _int(name, size), _int("overlap", overlap)
    if size < 16 or size % 16:
        raise ValueError(f"{name} must be a positive multiple of 16 (the model's grid), got {size}")
    if not 0 <= overlap <= size // 2:
        raise ValueError(f"overlap must lie in [0, {size // 2}] for {name} {size} (a sample is covered by at most two ramps per "
                         f"axis), got {overlap}")
    if n < 1:
        raise ValueError(f"an axis has at least one sample, got n = {n}")
    if n <= size:
        return [Span(0, 0)]
    stride = size - overlap
    count = -(-(n - overlap) // stride)
    starts = [i * stride for i in range(count - 1)] + [n - size]
    return [Span(s, 0 if i == 0 else starts[i - 1] + size - overlap - s) for i, s in enumerate(starts)]


def plan_tiles(H: int, W: int, tile_h: int, tile_w: int, overlap: int) -> Optional[List[Tile]]:
    """The tiles of an H x W picture in raster order (row-major), or None where the picture is one tile ("not tiled").  A tile_h
    or tile_w of 0, or one that is at least the picture's side, makes that axis one span of the whole side."""
    H, W = _int("H", H), _int("W", W)
    tile_h, tile_w, overlap = _int("tile_height", tile_h), _int("tile_width", tile_w), _int("tile_overlap", overlap)
    if H < 1 or W < 1:
        raise ValueError(f"a picture has at least one pixel, got (H, W) = {(H, W)}")
    if overlap < 0:
        raise ValueError(f"tile_overlap must not be negative, got {overlap}")
    axes = []
    for n, size, name in ((H, tile_h, "tile_height"), (W, tile_w, "tile_width")):
        if size == 0 or size >= n:                     # one span of the whole side: the overlap has nothing to fit into
            if size % 16:
                raise ValueError(f"{name} must be a positive multiple of 16 (the model's grid) or 0, got {size}")
            axes.append((n, [Span(0, 0)]))
            continue
        try:
            spans = plan_axis(n, size, overlap, name)
        except ValueError as e:
            raise ValueError(str(e).replace("overlap must", "tile_overlap must")) from None
        axes.append((size if len(spans) > 1 else n, spans))
    (h, ys), (w, xs) = axes
    if len(ys) * len(xs) == 1:
        return None
    return [Tile(sy.start, sx.start, h, w, sy.ramp_at, sx.ramp_at, overlap if i else 0, overlap if j else 0)
            for i, sy in enumerate(ys) for j, sx in enumerate(xs)]


def latent_tile(t: Tile, f: int) -> Tile:
    """`t` in latent units: every field divided by the tokenizer's spatial compression factor `f`.  One latent
    pixel is the same f x f pixels in every tile only where the tile's corner, written range and ramps lie on the f-grid, so a
    field off it is refused."""
    f = _int("f", f)
    if f < 1:
        raise ValueError(f"the compression factor is at least 1, got {f}")
    for name, v in zip(Tile._fields, t):
        if _int(name, v) % f:
            raise ValueError(f"{t}: {name} = {v} is off the latent grid of {f} (tile_overlap and the picture's sides must be "
                             f"multiples of {f} for a latent-space join)")
    return Tile(*(int(v) // f for v in t))


def covers(tiles: List[Tile], H: int, W: int) -> bool:
    """Whether the written rectangles of `tiles` cover every sample of an H x W canvas: what lets the latent join swap its two
    canvases after the last tile without clearing one."""
    seen = np.zeros((H, W), dtype=bool)
    for t in tiles:
        seen[t.y + t.ry:t.y + t.h, t.x + t.rx:t.x + t.w] = True
    return bool(seen.all())


def _weights(O: int, device):
    return torch.from_numpy(ramp_weights(O)).to(device) if O else None


def _check_latent(name, x, like=None):
    if x.dtype != torch.bfloat16 or x.ndim != 5:
        raise ValueError(f"{name}: bf16 [P, C, F, H, W] latents needed, got {x.dtype} {tuple(x.shape)}")
    if like is not None and (x.device != like.device or tuple(x.shape[:3]) != tuple(like.shape[:3])):
        raise ValueError(f"{name} {tuple(x.shape)} on {x.device} and the canvas {tuple(like.shape)} on {like.device} are not one "
                         "sample on one device")


def _torch_path(backend, x):
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    if backend == "hip" and not x.is_cuda:
        raise ValueError(f"backend='hip' needs a GPU tensor, got one on {x.device} (the torch path is what CPU devices run)")
    return backend == "torch" or not x.is_cuda


def latent_gather(canvas: torch.Tensor, t: Tile, c_in: float, copies: int = 1, backend: str = "auto") -> torch.Tensor:
    """The DiT's input for one tile: the crop of the latent canvas bf16 [P, C, F, Hc, Wc] at `t` (latent units), scaled by c_in
    in fp32 and rounded to bf16 - edm_scale_input of the contiguous crop -, `copies` (1, or 2 under CFG) times along the batch.
    backend as for blend_tile; the HIP path is one launch of drn_latent_tile_gather."""
    _check_latent("canvas", canvas)
    if copies not in (1, 2):
        raise ValueError(f"copies must be 1 or 2, got {copies}")
    Hc, Wc = canvas.shape[3:5]
    if t.y < 0 or t.x < 0 or t.h < 1 or t.w < 1 or t.y + t.h > Hc or t.x + t.w > Wc:
        raise ValueError(f"{t} does not lie inside a canvas of {(Hc, Wc)}")
    if _torch_path(backend, canvas):
        one = (canvas[..., t.y:t.y + t.h, t.x:t.x + t.w].float() * c_in).to(torch.bfloat16)
        return torch.cat([one] * copies, 0).contiguous()
    if not canvas.is_contiguous():
        raise ValueError("the HIP path gathers from a contiguous canvas")
    from . import native
    return native.latent_tile_gather(canvas, t.h, t.w, t.y, t.x, float(c_in), copies)


def _step_join_torch(model_out, uncond, guidance, cur, nxt, t: Tile, wy, wx, c_skip, c_out, sigma, dt):
    """The specification, on slices.  m = the CFG combine of cfg_kernel (two bf16 roundings inside, one outside) or the model's
    output; b = edm_step_kernel's update of the CURRENT canvas, rounded to bf16; then _blend_torch's rule on bf16: nxt <- b where
    wgt == 1 (nxt is not read there), else bf16(a + wgt * (b - a)) in three fp32 operations."""
    bf = torch.bfloat16
    ys, xs = slice(t.y + t.ry, t.y + t.h), slice(t.x + t.rx, t.x + t.w)
    m = model_out[..., t.ry:, t.rx:].float()
    if uncond is not None:
        d = (m - uncond[..., t.ry:, t.rx:].float()).to(bf).float()
        gd = (d * float(guidance)).to(bf).float()
        m = (m + gd).to(bf).float()
    sm = cur[..., ys, xs].float()
    denoised = sm * float(c_skip) + m * float(c_out)
    deriv = (sm - denoised) / torch.tensor(float(sigma), dtype=torch.float32, device=sm.device)     # a true division on any device
    b = (sm + deriv * float(dt)).to(bf).float()
    fy = torch.ones(t.h - t.ry, dtype=torch.float32, device=nxt.device)
    fx = torch.ones(t.w - t.rx, dtype=torch.float32, device=nxt.device)
    if wy is not None:
        fy[:t.Oy] = wy
    if wx is not None:
        fx[:t.Ox] = wx
    wgt = fy[:, None] * fx[None, :]
    a = nxt[..., ys, xs].float()
    d = b - a
    mm = wgt * d
    nxt[..., ys, xs] = torch.where(wgt == 1.0, b, a + mm).to(bf)
    return nxt


def latent_step_join(model_out: torch.Tensor, uncond: Optional[torch.Tensor], guidance: float, canvas_cur: torch.Tensor,
                     canvas_next: torch.Tensor, t: Tile, c_skip: float, c_out: float, sigma: float, dt: float,
                     backend: str = "auto") -> torch.Tensor:
    """One tile's Euler step joined into the NEXT latent canvas, IN PLACE: model_out (and uncond, or None for no CFG) bf16
    [P, C, F, h, w], the canvases bf16 [P, C, F, Hc, Wc], `t` the tile's entry of plan_tiles in latent units (latent_tile).  The
    sample is read from canvas_cur, the ramps run over what the tiles above and to the left wrote to canvas_next.  backend as for
    blend_tile; the HIP path is one launch of drn_latent_tile_step_join.  Returns canvas_next."""
    _check_latent("canvas_cur", canvas_cur)
    _check_latent("canvas_next", canvas_next, canvas_cur)
    _check_latent("model_out", model_out, canvas_cur)
    if uncond is not None:
        _check_latent("uncond", uncond, canvas_cur)
        if tuple(uncond.shape) != tuple(model_out.shape):
            raise ValueError(f"uncond {tuple(uncond.shape)} is not shaped like model_out {tuple(model_out.shape)}")
    Hc, Wc = canvas_cur.shape[3:5]
    if tuple(canvas_next.shape) != tuple(canvas_cur.shape) or canvas_next.data_ptr() == canvas_cur.data_ptr():
        raise ValueError("the join reads one canvas and writes another of the same shape")
    if tuple(model_out.shape[3:5]) != (t.h, t.w) or t.y < 0 or t.x < 0 or t.y + t.h > Hc or t.x + t.w > Wc:
        raise ValueError(f"{t} does not describe a tile of {tuple(model_out.shape[3:5])} inside a canvas of {(Hc, Wc)}")
    if not (0 <= t.ry < t.h and 0 <= t.rx < t.w and t.Oy >= 0 and t.Ox >= 0 and t.ry + t.Oy <= t.h and t.rx + t.Ox <= t.w):
        raise ValueError(f"{t}: the written range and its ramps must lie inside the tile")
    if float(sigma) == 0.0:
        raise ValueError("sigma must not be 0 (the step divides by it)")
    wy, wx = _weights(t.Oy, canvas_cur.device), _weights(t.Ox, canvas_cur.device)
    if _torch_path(backend, canvas_cur):
        return _step_join_torch(model_out, uncond, guidance, canvas_cur, canvas_next, t, wy, wx, c_skip, c_out, sigma, dt)
    if not (canvas_cur.is_contiguous() and canvas_next.is_contiguous()):
        raise ValueError("the HIP path joins contiguous canvases")
    from . import native
    return native.latent_tile_step_join(model_out.contiguous(), None if uncond is None else uncond.contiguous(), float(guidance),
                                        canvas_cur, canvas_next, wy, wx, t.y, t.x, t.ry, t.rx, float(c_skip), float(c_out),
                                        float(sigma), float(dt))


def _blend_torch(canvas, tile, t: Tile, wy, wx):
    """The specification, on slices: wgt = wy * wx (1.0 where an axis has no ramp or the sample lies behind it), canvas <- tile where
    wgt == 1 (the canvas is not read there), else round_half_even(a + wgt * (b - a)) in three fp32 operations, clamped."""
    hh, ww = t.h - t.ry, t.w - t.rx
    dst = canvas[:, :, t.y + t.ry:t.y + t.h, t.x + t.rx:t.x + t.w]
    src = tile[:, :, t.ry:, t.rx:]
    fy = torch.ones(hh, dtype=torch.float32, device=canvas.device)
    fx = torch.ones(ww, dtype=torch.float32, device=canvas.device)
    if wy is not None:
        fy[:t.Oy] = wy
    if wx is not None:
        fx[:t.Ox] = wx
    # behind both ramps every weight is 1: a copy.  The ramps are the top strip (every column) and the left strip below it
    dst[:, :, t.Oy:, t.Ox:] = src[:, :, t.Oy:, t.Ox:]
    for ys, xs in ((slice(0, t.Oy), slice(0, ww)), (slice(t.Oy, hh), slice(0, t.Ox))):
        wgt = (fy[ys, None] * fx[None, xs])[:, :, None]
        a, b = dst[:, :, ys, xs].float(), src[:, :, ys, xs].float()
        d = b - a
        m = wgt * d
        v = torch.where(wgt == 1.0, b, a + m)
        dst[:, :, ys, xs] = v.round().clamp(0.0, 255.0).to(torch.uint8)
    return canvas


def blend_tile(canvas: torch.Tensor, tile: torch.Tensor, t: Tile, backend: str = "auto") -> torch.Tensor:
    """One rendered tile into the picture's canvas, IN PLACE: canvas uint8 [B, T, H, W, 3], tile uint8 [B, T, h, w, 3] on the same
    device, `t` the tile's entry of plan_tiles.  Tiles are blended in raster order: a tile's ramps run over what the tiles above
    and to the left wrote.  backend: 'auto' = the HIP kernel (drn_tile_blend_u8) on a GPU tensor and torch on a CPU tensor;
    'torch' / 'hip' force a path ('hip' needs a GPU tensor).  Returns the canvas."""
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    for name, u8 in (("canvas", canvas), ("tile", tile)):
        if u8.dtype != torch.uint8 or u8.ndim != 5 or u8.shape[-1] != 3:
            raise ValueError(f"{name}: uint8 [B, T, H, W, 3] frames needed, got {u8.dtype} {tuple(u8.shape)}")
    if tile.device != canvas.device or tuple(tile.shape[:2]) != tuple(canvas.shape[:2]):
        raise ValueError(f"canvas {tuple(canvas.shape)} on {canvas.device} and tile {tuple(tile.shape)} on {tile.device} are not "
                         "one clip on one device")
    H, W = canvas.shape[2:4]
    if tuple(tile.shape[2:4]) != (t.h, t.w) or t.y < 0 or t.x < 0 or t.y + t.h > H or t.x + t.w > W:
        raise ValueError(f"{t} does not describe a tile of {tuple(tile.shape[2:4])} inside a canvas of {(H, W)}")
    if not (0 <= t.ry < t.h and 0 <= t.rx < t.w and t.Oy >= 0 and t.Ox >= 0 and t.ry + t.Oy <= t.h and t.rx + t.Ox <= t.w):
        raise ValueError(f"{t}: the written range and its ramps must lie inside the tile")
    if backend == "hip" and not canvas.is_cuda:
        raise ValueError(f"backend='hip' needs a GPU tensor, got one on {canvas.device} (the torch path is what CPU devices run)")
    wy, wx = _weights(t.Oy, canvas.device), _weights(t.Ox, canvas.device)
    if backend == "torch" or not canvas.is_cuda:
        return _blend_torch(canvas, tile, t, wy, wx)
    if not canvas.is_contiguous():
        raise ValueError("the HIP path blends into a contiguous canvas")
    from . import native
    return native.tile_blend_u8(canvas, tile.contiguous(), wy, wx, t.y, t.x, t.ry, t.rx)
