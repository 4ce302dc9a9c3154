"""Seed ensembles: the settings check and the specification of the per-pixel reduce (reduce_members below: torch,
on whatever device the tensors live, and what CPU devices run; the GPU path is csrc/ensemble.hip, drn_ensemble_reduce_u8).

The inverse renderer is a sampler: two seeds give two base colours, roughness maps and depths for one video.  Test-time
ensembling (Marigold, GeoWizard) renders the same input under N seeds and reduces the N samples per pixel with a robust
statistic.  Here the members are the pipeline's uint8 results [..., 3], which stay on the device, and the reduce is

    median   per byte: the two middle values of the N sorted bytes, averaged half to even (odd N: the middle value)
    mean     per byte: the integer sum over N, rounded half to even
    normal   per pixel: the members decoded to vectors, summed, renormalised and encoded again - a channel-wise median or mean
             of unit vectors is not a unit vector

with, on request, the members' spread around the result: the median (mean) absolute deviation per byte, or for normals one minus
the mean resultant length |sum v_k| / N, written to all three channels.  Everything is integer arithmetic or fp32 with every
operation rounded on its own, so the kernel and this file agree bit for bit.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from .fit import u8_unit

MODES = ("median", "mean", "normal")
REDUCES = ("median", "mean")             # what `ensemble_reduce` may name; "normal" is chosen per pass by its flag
MAX_MEMBERS = 16
SEED_MASK = 2 ** 64 - 1


def check_ensemble(ensemble, ensemble_reduce="median", init_noise=None):
    """ValueError for an ensemble that cannot be rendered, from settings alone (so before any GPU work)."""
    if isinstance(ensemble, bool) or not isinstance(ensemble, int) or not 1 <= ensemble <= MAX_MEMBERS:
        raise ValueError(f"ensemble must be an integer in 1..{MAX_MEMBERS} (1 = off), got {ensemble!r}")
    if ensemble_reduce not in REDUCES:
        raise ValueError(f"ensemble_reduce must be one of {REDUCES}, got {ensemble_reduce!r}")
    if ensemble > 1 and init_noise is not None:
        raise ValueError(f"ensemble = {ensemble} with an init_noise is refused: every member would start from the same noise and "
                         "be the same sample (set ensemble = 1, or leave the start noise to the seeds)")


def member_seed(seed: int, k: int) -> int:
    """The seed of member k: seed + k, wrapped at 2^64 (member 0 renders under the call's own seed)."""
    return (int(seed) + int(k)) & SEED_MASK


def _half_even_mid(lo, hi):
    t = lo + hi
    r = t >> 1
    return r + ((t & 1) * (r & 1))


def _median(stack):
    s, _ = torch.sort(stack, dim=0)
    N = stack.shape[0]
    return _half_even_mid(s[(N - 1) // 2], s[N // 2])


def _mean(stack):
    N = stack.shape[0]
    S = stack.sum(dim=0)
    q = torch.div(S, N, rounding_mode="floor")
    rem = S - q * N
    up = (2 * rem > N) | ((2 * rem == N) & ((q & 1) == 1))
    return q + up.to(q.dtype)


def _reduce_torch(members, mode, spread):
    N = len(members)
    if mode in ("median", "mean"):
        stat = _median if mode == "median" else _mean
        stack = torch.stack([m.to(torch.int32) for m in members])
        r = stat(stack)
        sp = stat((stack - r).abs()).to(torch.uint8) if spread else None
        return r.to(torch.uint8), sp
    # normal: fp32, one rounding per operation (torch never fuses two ops)
    s = None
    for m in members:
        v = u8_unit(m) * 2.0 - 1.0
        s = v if s is None else s + v
    l2 = (s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + s[..., 2] * s[..., 2]
    # the correctly rounded fp32 root: torch's vectorised fp32 sqrt on the CPU is not (l2 = 0x40030991 comes back one ulp low), the
    # float64 root rounded to fp32 is (a root cannot lie close enough to a midpoint of fp32 for the second rounding to matter)
    l = torch.sqrt(l2.to(torch.float64)).to(torch.float32)
    d = torch.clamp(l, min=1e-6)
    n = s / d.unsqueeze(-1)
    r = torch.round(torch.clamp((n + 1.0) * 127.5, 0.0, 255.0)).to(torch.uint8)
    sp = None
    if spread:
        one = torch.round(255.0 * torch.clamp(1.0 - l / float(N), 0.0, 1.0)).to(torch.uint8)
        sp = one.unsqueeze(-1).expand(r.shape).contiguous()
    return r, sp


def reduce_members(members: Sequence[torch.Tensor], mode: str, spread: bool = False,
                   backend: str = "auto") -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """N uint8 tensors of one shape [..., 3] on one device (1 <= N <= 16; they need not be contiguous with each other) -> (the
    per-pixel reduce under `mode`, the members' spread around it or None), both uint8 of the members' shape.  N = 1: 'median'
    and 'mean' copy the member (spread 0); 'normal' still renormalises it.

    backend: 'auto' = the HIP kernel (drn_ensemble_reduce_u8, one launch, no stack of the members) on GPU tensors and torch on
    CPU tensors; 'torch' / 'hip' force a path ('hip' needs GPU tensors).  The torch path is the specification and what CPU
    devices run."""
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    members = list(members)
    if not 1 <= len(members) <= MAX_MEMBERS:
        raise ValueError(f"1..{MAX_MEMBERS} members can be reduced, got {len(members)}")
    first = members[0]
    for k, m in enumerate(members):
        if not isinstance(m, torch.Tensor) or m.dtype != torch.uint8:
            raise ValueError(f"member {k} is not a uint8 tensor")
        if m.ndim < 1 or m.shape[-1] != 3:
            raise ValueError(f"member {k} {tuple(m.shape)} is not [..., 3] pixels")
        if m.shape != first.shape or m.device != first.device:
            raise ValueError(f"member {k} {tuple(m.shape)} on {m.device} and member 0 {tuple(first.shape)} on {first.device} are "
                             "not one result on one device")
    if backend == "hip" and not first.is_cuda:
        raise ValueError(f"backend='hip' needs GPU tensors, got them on {first.device} (the torch path is what CPU devices run)")
    if backend == "torch" or not first.is_cuda or first.numel() == 0:
        return _reduce_torch(members, mode, bool(spread))
    from . import native
    return native.ensemble_reduce_u8([m.contiguous() for m in members], mode, bool(spread))


def reduce_results(member_outs: List[list], flags, reduce: str, spread: bool = False):
    """The pipeline's walk over N members' results: member_outs[k][c][p] = member k's uint8 result of batch c and pass p,
    flags[c][p] = that pass's normalize_normal flag -> (results[c][p], spreads[c][p] or None) with the mode 'normal' where the flag
    is set and `reduce` elsewhere.  A member's tensors are dropped from `member_outs` as soon as their pass is reduced."""
    results, spreads = [], []
    for c, fl in enumerate(flags):
        results.append([])
        spreads.append([])
        for p, flag in enumerate(fl):
            mem = [outs[c][p] for outs in member_outs]
            for outs in member_outs:
                outs[c][p] = None
            r, s = reduce_members(mem, "normal" if flag else reduce, spread=spread)
            del mem
            results[-1].append(r)
            spreads[-1].append(s)
    return results, spreads
