"""Relight edits: material edits and layer insertion on the G-buffers between the two stages of Cosmos1Relight.

The inverse stage leaves five uint8 maps [B, T, H', W', 3] on the device, in INVERSE_PASSES order (base colour, metallic,
roughness, normal, depth).  An edit changes them before the forward stage renders from them:

    material editing    per map and channel a gain and an offset on the byte scale, applied where `edit_mask` says
    object insertion    per map a `layer` - the inserted object's own G-buffer - composited under the object's matte
                        `insert_mask`; both are then lit together

The rule per map, pixel and channel, with x the byte, unit(i) = fit.u8_unit (the correctly rounded i / 255), every fp32
operation rounded on its own and rint rounding half to even:

    e = u8(rint(clamp(fp32(g * fp32(x)) + o, 0, 255)))       the affine of ensemble.apply_affine_u8, same rounding
    y = u8(rint(x + unit(m_e) * (e - x)))                    tiles' blend; m_e = 255 gives e, 0 gives x
    z = layer ? u8(rint(y + unit(m_i) * (L - y))) : y        L = the layer's byte
    normal map only, pixels with a normal layer and m_i != 0:
        z <- ensemble.reduce_members([z], "normal")          decode, l2, correctly rounded sqrt and /, max(l, 1e-6), encode

A pixel with m_e == 0 and m_i == 0 keeps its bytes in every map, and a normal is never renormalised where nothing was inserted.
Masks and layers broadcast over frames and clips where their T or B is 1.  `edit_gbuffers` below is the specification in torch
and what CPU devices run; on GPU tensors one launch of drn_gbuffer_edit_u8 (csrc/gbuffer_edit.hip) edits all maps in place.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from .fit import RestorePlan, _single, restore_frames, u8_unit

MAPS = ("basecolor", "metallic", "roughness", "normal", "depth")         # nodes.INVERSE_PASSES: the order of every list here
NORMAL = MAPS.index("normal")
GAIN_MIN, GAIN_MAX = 0.0, 8.0
OFFSET_MAX = 255.0


def _identity_rows():
    return [[1.0, 1.0, 1.0] for _ in MAPS], [[0.0, 0.0, 0.0] for _ in MAPS]


@dataclass
class GBufferEdit:
    """gain, offset: [5][3] per map and channel, offsets on the byte scale, identity (1, 0); the normal map's row must be the
    identity.  edit_mask: [1 or B, 1 or T, H, W] or None = 255 everywhere: where the affine applies.  layers: per map None or
    [1 or B, 1 or T, H, W, 3], the inserted object's G-buffer.  insert_mask: the object's matte, shaped like edit_mask; required
    exactly when a layer is set.  Masks and layers are uint8, or float32 in [0, 1] (a value v standing for the byte
    round(v * 255), as fit.source_guide makes bytes)."""
    gain: Sequence[Sequence[float]] = field(default_factory=lambda: _identity_rows()[0])
    offset: Sequence[Sequence[float]] = field(default_factory=lambda: _identity_rows()[1])
    edit_mask: Optional[torch.Tensor] = None
    layers: Sequence[Optional[torch.Tensor]] = field(default_factory=lambda: [None] * len(MAPS))
    insert_mask: Optional[torch.Tensor] = None


def check_edit(edit: GBufferEdit, shape, source_hw=None):
    """ValueError for an edit that cannot be applied to G-buffers of shape = (B, T, H', W'), from the settings and shapes alone
    (so before any pipeline or GPU call).  source_hw: the source picture's (H, W) where masks and layers may also arrive at that
    size (the node, which then brings them to the model's grid with the fit's own tables); None: the model's size only."""
    B, T, H, W = (int(n) for n in shape)
    gain, offset = np.asarray(edit.gain, dtype=np.float64), np.asarray(edit.offset, dtype=np.float64)
    if gain.shape != (len(MAPS), 3) or offset.shape != (len(MAPS), 3):
        raise ValueError(f"gain and offset are [5][3] (per map in {MAPS} and channel), got {gain.shape} and {offset.shape}")
    if not (np.isfinite(gain).all() and np.isfinite(offset).all()):
        raise ValueError("an edit's gains and offsets must be finite")
    if (gain < GAIN_MIN).any() or (gain > GAIN_MAX).any():
        raise ValueError(f"an edit's gain must lie in [{GAIN_MIN:g}, {GAIN_MAX:g}], got {gain.min():g} .. {gain.max():g}")
    if (np.abs(offset) > OFFSET_MAX).any():
        raise ValueError(f"an edit's offset must lie in [-{OFFSET_MAX:g}, {OFFSET_MAX:g}] (the byte scale), got "
                         f"{offset.min():g} .. {offset.max():g}")
    if (gain[NORMAL] != 1.0).any() or (offset[NORMAL] != 0.0).any():
        raise ValueError("the normal map takes no gain or offset: an affine of an encoded unit vector is not one (insert a normal "
                         "layer instead)")
    layers = list(edit.layers)
    if len(layers) != len(MAPS):
        raise ValueError(f"layers holds one entry per map in {MAPS} (None = nothing inserted), got {len(layers)}")
    any_layer = any(l is not None for l in layers)
    if any_layer and edit.insert_mask is None:
        raise ValueError("a layer needs insert_mask, the inserted object's matte")
    if edit.insert_mask is not None and not any_layer:
        raise ValueError("insert_mask without any layer: nothing would be inserted")
    sizes = [(H, W)] + ([tuple(int(n) for n in source_hw)] if source_hw is not None else [])
    named = [("edit_mask", edit.edit_mask, 4), ("insert_mask", edit.insert_mask, 4)]
    named += [(f"the {MAPS[k]} layer", l, 5) for k, l in enumerate(layers)]
    for name, t, ndim in named:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"{name} must be a uint8 or float32 tensor, got {getattr(t, 'dtype', type(t))}")
        want = "[B, T, H, W]" if ndim == 4 else "[B, T, H, W, 3]"
        if t.ndim != ndim or (ndim == 5 and t.shape[-1] != 3):
            raise ValueError(f"{name} must be {want}, got {tuple(t.shape)}")
        if t.shape[1] not in (1, T):
            raise ValueError(f"{name} has {t.shape[1]} frames: 1 (for every frame) or the clip's {T}")
        if t.shape[0] not in (1, B):
            raise ValueError(f"{name} has {t.shape[0]} clips: 1 (for every clip) or the batch's {B}")
        if tuple(t.shape[2:4]) not in sizes:
            raise ValueError(f"{name} is (H, W) = {tuple(t.shape[2:4])}: neither the model's {(H, W)}"
                             + (f" nor the source's {sizes[1]}" if source_hw is not None else ""))


def as_bytes(t: torch.Tensor) -> torch.Tensor:
    """uint8 as it is; float32 in [0, 1] -> round(x * 255), clamped: the bytes fit.source_guide makes."""
    if t.dtype == torch.uint8:
        return t
    return (t.to(torch.float32) * 255.0).round().clamp(0, 255).to(torch.uint8)


def _affine(x, g, o):
    return torch.round(torch.clamp(x.to(torch.float32) * g + o, 0.0, 255.0)).to(torch.uint8)


def _blend(a, b, m):
    """a + unit(m) * (b - a) on bytes; m [B', T', H, W] broadcasts over clips, frames and the three channels."""
    fa = a.to(torch.float32)
    return torch.round(fa + u8_unit(m).unsqueeze(-1) * (b.to(torch.float32) - fa)).clamp(0.0, 255.0).to(torch.uint8)


def _edit_torch(gbuffers, edit):
    from .ensemble import reduce_members
    out = []
    for k, x in enumerate(gbuffers):
        g = torch.tensor(edit.gain[k], dtype=torch.float32, device=x.device)
        o = torch.tensor(edit.offset[k], dtype=torch.float32, device=x.device)
        z = x
        if not (bool((g == 1.0).all()) and bool((o == 0.0).all())):
            e = _affine(x, g, o)
            z = e if edit.edit_mask is None else _blend(x, e, edit.edit_mask)
        L = edit.layers[k]
        if L is not None:
            z = _blend(z, L, edit.insert_mask)
            if k == NORMAL:
                unit, _ = reduce_members([z], "normal", backend="torch")
                z = torch.where((edit.insert_mask != 0).unsqueeze(-1), unit, z)
        out.append(z)
    return out


def is_identity(edit: GBufferEdit) -> bool:
    """Nothing set: every gain 1, every offset 0, no layer."""
    return bool((np.asarray(edit.gain) == 1.0).all()) and bool((np.asarray(edit.offset) == 0.0).all()) and \
        all(l is None for l in edit.layers)


def edit_gbuffers(gbuffers: Sequence[torch.Tensor], edit: GBufferEdit, backend: str = "auto") -> List[torch.Tensor]:
    """The five uint8 G-buffers [B, T, H, W, 3] in MAPS order, on one device, under `edit` (masks and layers at the G-buffers'
    size, uint8 or float32) -> the five edited maps.  backend: 'auto' = the HIP kernel (drn_gbuffer_edit_u8: ONE launch for all
    maps, IN PLACE on the tensors handed in wherever their frames are contiguous - a [:, :keep] view is) on GPU tensors and
    torch on CPU tensors; 'torch' / 'hip' force a path ('hip' needs GPU tensors).  The torch path is the specification, returns
    new tensors for the maps it changes and builds fp32 copies on the way; a map the edit does not touch is returned as it is."""
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    gbuffers = list(gbuffers)
    if len(gbuffers) != len(MAPS):
        raise ValueError(f"the G-buffers are five maps in the order {MAPS}, got {len(gbuffers)}")
    first = gbuffers[0]
    for k, g in enumerate(gbuffers):
        if not isinstance(g, torch.Tensor) or g.dtype != torch.uint8 or g.ndim != 5 or g.shape[-1] != 3:
            raise ValueError(f"the {MAPS[k]} map must be uint8 [B, T, H, W, 3], got {getattr(g, 'dtype', type(g))} "
                             f"{tuple(getattr(g, 'shape', ()))}")
        if g.shape != first.shape or g.device != first.device:
            raise ValueError(f"the {MAPS[k]} map {tuple(g.shape)} on {g.device} and the {MAPS[0]} map {tuple(first.shape)} on "
                             f"{first.device} are not one clip on one device")
    check_edit(edit, first.shape[:4])
    if backend == "hip" and not first.is_cuda:
        raise ValueError(f"backend='hip' needs GPU tensors, got them on {first.device} (the torch path is what CPU devices run)")
    dev = first.device
    edit = GBufferEdit(edit.gain, edit.offset, None if edit.edit_mask is None else as_bytes(edit.edit_mask.to(dev)),
                       [None if l is None else as_bytes(l.to(dev)) for l in edit.layers],
                       None if edit.insert_mask is None else as_bytes(edit.insert_mask.to(dev)))
    if is_identity(edit) or first.numel() == 0:
        return gbuffers
    if backend == "torch" or not first.is_cuda:
        return _edit_torch(gbuffers, edit)
    from . import native
    maps, at = [], []
    for k, g in enumerate(gbuffers):
        gain, offset = [float(v) for v in edit.gain[k]], [float(v) for v in edit.offset[k]]
        if edit.layers[k] is None and gain == [1.0] * 3 and offset == [0.0] * 3:
            continue                                        # untouched: not handed to the kernel
        if not g[0, 0].is_contiguous():
            g = g.contiguous()
        layer = edit.layers[k]
        if layer is not None and not layer[0, 0].is_contiguous():
            layer = layer.contiguous()
        maps.append((g, g, layer, gain, offset, k == NORMAL))
        at.append(k)
    masks = [None if m is None else (m if m[0, 0].is_contiguous() else m.contiguous()) for m in (edit.edit_mask, edit.insert_mask)]
    for k, dst in zip(at, native.gbuffer_edit_u8(maps, masks[0], masks[1])):
        gbuffers[k] = dst
    return gbuffers


# ----------------------------------------------------------------------------------------------- the node's inputs
def _frames_4d(m: torch.Tensor, clips) -> torch.Tensor:
    """A stack of N frames [N, ...] -> [B', T', ...]: N clips of one frame where N is 1 or the batch's B, as the nodes read a 4-D
    IMAGE; otherwise the N frames of one clip (a video's mask beside a 5-D image)."""
    return m.unsqueeze(1) if clips is None or m.shape[0] in (1, int(clips)) else m.unsqueeze(0)


def _mask_4d(m: torch.Tensor, name: str, clips=None) -> torch.Tensor:
    """A ComfyUI MASK -> [B, T, H, W]: [H, W] is one frame for all; [N, H, W] a stack of frames (_frames_4d); [B, T, H, W] as it
    is.  A mask may ride as an IMAGE of three equal channels ([N, H, W, 3] or [B, T, H, W, 3]): its first."""
    if not isinstance(m, torch.Tensor):
        raise ValueError(f"{name} must be a tensor, got {type(m)}")
    if m.ndim == 5 or (m.ndim == 4 and m.shape[-1] == 3):
        m = m[..., 0]
    if m.ndim == 2:
        return m[None, None]
    if m.ndim == 3:
        return _frames_4d(m, clips)
    if m.ndim == 4:
        return m
    raise ValueError(f"{name} must be [H, W], [N, H, W] or [B, T, H, W] (or an IMAGE of three equal channels), got {tuple(m.shape)}")


def _layer_5d(l, name, standardize, clips):
    if isinstance(l, torch.Tensor) and l.ndim == 4:
        return _frames_4d(l, clips)
    return standardize(l, name)


def build_edit(standardize, edit_mask=None, edit_base_color_tint=0xFFFFFF, edit_base_color_gain=1.0, edit_roughness_gain=1.0,
               edit_metallic_gain=1.0, edit_base_color_offset=0.0, edit_roughness_offset=0.0, edit_metallic_offset=0.0,
               insert_mask=None, insert_base_color=None, insert_metallic=None, insert_roughness=None, insert_normal=None,
               insert_depth=None, clips=None) -> Optional[GBufferEdit]:
    """Cosmos1Relight's edit inputs -> the edit, or None where every input is at its default (then nothing is built and the node
    makes exactly the calls it made before the inputs existed).  The base colour's gain per channel is tint_c / 255 * gain, the
    tint a display colour 0xRRGGBB; offsets arrive in [-1, 1] and are scaled by 255; a constant is gain 0 plus an offset.
    standardize: the nodes' standardize_to_5d, which layers go through like any IMAGE; clips: the image's B, which decides how a
    stack of N frames is read (_frames_4d)."""
    tint = int(edit_base_color_tint)
    if not 0 <= tint <= 0xFFFFFF:
        raise ValueError(f"edit_base_color_tint is a display colour 0xRRGGBB, got {edit_base_color_tint!r}")
    gain, offset = _identity_rows()
    for name, g, o in (("basecolor", edit_base_color_gain, edit_base_color_offset), ("roughness", edit_roughness_gain, edit_roughness_offset),
                       ("metallic", edit_metallic_gain, edit_metallic_offset)):
        if not (math.isfinite(float(g)) and math.isfinite(float(o))):
            raise ValueError("an edit's gains and offsets must be finite")
        if abs(float(o)) > 1.0:
            raise ValueError(f"an edit's offset input must lie in [-1, 1] (it is scaled by 255), got {o!r}")
        k = MAPS.index(name)
        gain[k] = [float(g)] * 3
        offset[k] = [float(o) * 255.0] * 3
    k = MAPS.index("basecolor")
    gain[k] = [((tint >> s) & 255) / 255.0 * float(edit_base_color_gain) for s in (16, 8, 0)]
    layers = [insert_base_color, insert_metallic, insert_roughness, insert_normal, insert_depth]          # MAPS order
    edit = GBufferEdit(gain, offset, None, [None] * len(MAPS), None)
    if is_identity(edit) and edit_mask is None and insert_mask is None and all(l is None for l in layers):
        return None
    edit.edit_mask = None if edit_mask is None else _mask_4d(edit_mask, "edit_mask", clips)
    edit.insert_mask = None if insert_mask is None else _mask_4d(insert_mask, "insert_mask", clips)
    edit.layers = [None if l is None else _layer_5d(l, f"insert_{MAPS[i]}", standardize, clips) for i, l in enumerate(layers)]
    return edit


def fit_edit(edit: GBufferEdit, plan, device) -> GBufferEdit:
    """The edit's masks and layers as bytes on `device` at the model's grid.  What arrives at the model's size is used as it is;
    what arrives at the source's goes through the fit's own spatial tables on bytes (restore_frames under the plan's y / x tables,
    as fit.plan_guide_lo builds them, without plan_restore's refusal: a cutting crop is fine here, nothing is undone).
    plan: the FitPlan of the call, or None with fit off."""
    rplan = None

    def to_grid(t, mask):
        nonlocal rplan
        if t is None:
            return None
        t = as_bytes(t.to(device))
        if plan is None or tuple(t.shape[2:4]) == (plan.H_out, plan.W_out):
            return t
        if rplan is None:
            same = _single(plan.y_lo_n.numpy(), plan.y_w.numpy(), plan.H) and _single(plan.x_lo_n.numpy(), plan.x_w.numpy(), plan.W)
            rplan = RestorePlan(0, plan.H, plan.W, plan.H_out, plan.W_out, plan.y_lo_n, plan.y_w, plan.x_lo_n, plan.x_w, same)
        rplan.T = t.shape[1]
        if mask:
            return restore_frames(t.unsqueeze(-1).expand(*t.shape, 3).contiguous(), rplan)[..., 0].contiguous()
        return restore_frames(t.contiguous(), rplan).contiguous()

    return GBufferEdit(edit.gain, edit.offset, to_grid(edit.edit_mask, True), [to_grid(l, False) for l in edit.layers],
                       to_grid(edit.insert_mask, True))
