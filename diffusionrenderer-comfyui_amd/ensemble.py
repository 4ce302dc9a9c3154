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

Ensembles that agree (`ensemble_align`): relative depth and base colour come out of every seed at a gain and an
offset of their own, so a per-byte median of the raw members is a median of different quantities.  With the switch on, every
member k >= 1 of every non-normal pass is first carried into member 0's space by one pair (g, o) per clip, solved from the
members' Gram matrix over the whole clip (align_solve_members is the rule, align_members runs it; on the GPU
csrc/ensemble_align.hip, drn_ensemble_align_affine), and the reduce reads every byte through its member's pair (apply_affine_u8;
drn_ensemble_reduce_affine_u8).  All sums behind the rule are integers, so they are exact in any order.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .fit import u8_unit

MODES = ("median", "mean", "normal")
REDUCES = ("median", "mean")             # what `ensemble_reduce` may name; "normal" is chosen per pass by its flag
MAX_MEMBERS = 16
SEED_MASK = 2 ** 64 - 1


ALIGN_FLAT = 2.0 ** -6               # windows.ALIGN_FLAT_VAR on the byte scale: a standard deviation of an eighth of a level
ALIGN_GAIN_MIN, ALIGN_GAIN_MAX = 0.5, 2.0
ALIGN_MAX_CLIP = 2 ** 36             # bytes per clip: every sum stays below 2^53 and converts to float64 exactly


def check_ensemble(ensemble, ensemble_reduce="median", init_noise=None, ensemble_align=False):
    """ValueError for an ensemble that cannot be rendered, from settings alone (so before any GPU work)."""
    if not isinstance(ensemble_align, bool):
        raise ValueError(f"ensemble_align must be True or False, got {ensemble_align!r}")
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


# ----------------------------------------------------------------------------------------------- ensembles that agree
def align_solve_members(n, S, G):
    """The rule, in float64 on the byte scale, from the exact integer sums of one clip of n bytes: S[k] = sum m_k and
    G[j][k] = sum m_j m_k (the upper triangle j <= k is read) -> (affine float32 [N, 2] = (g, o) per member, each rounded to fp32
    once, (mean float64 [N], C float64 [N, N])).  Population moments; every operation rounded on its own.

    Member 0 keeps (1, 0).  For k >= 1 and N >= 3 the cross rule: num = sum_j C_0j and den = sum_j C_kj over j not in {0, k}; with
    m_k = g_k truth + o_k + noise_k a third member's noise is independent of both, so cov(m_k, m_j) = g_k g_j var(truth) whatever
    each member's own noise is, and num / den = g_0 / g_k (the instrumental-variable estimate).  Where either is below ALIGN_FLAT
    (or N = 2) the rule of windows.align_solve: g = sqrt(C_00 / C_kk), or 1 for a flat member or members that disagree
    (C_0k <= 0).  g is clamped to [0.5, 2], o = mean_0 - g mean_k with the clamped g; anything non-finite gives (1, 0)."""
    f = np.float64
    N = len(S)
    mean = np.zeros(N, dtype=f)
    C = np.zeros((N, N), dtype=f)
    out = np.zeros((N, 2), dtype=np.float32)
    out[:, 0] = 1.0
    with np.errstate(all="ignore"):
        n = f(n)
        for k in range(N):
            mean[k] = f(S[k]) / n
        for j in range(N):
            for k in range(j, N):
                e = f(G[j][k]) / n
                mm = mean[j] * mean[k]
                C[j, k] = C[k, j] = e - mm
        for k in range(1, N):
            g = None
            if N >= 3:
                num, den = f(0.0), f(0.0)
                for j in range(1, N):
                    if j != k:
                        num = num + C[0, j]
                        den = den + C[k, j]
                if np.isfinite(num) and np.isfinite(den) and num >= ALIGN_FLAT and den >= ALIGN_FLAT:
                    g = num / den
            if g is None:
                g = f(1.0)
                if C[0, 0] >= ALIGN_FLAT and C[k, k] >= ALIGN_FLAT and C[0, k] > 0:
                    g = np.sqrt(C[0, 0] / C[k, k])
            g = min(max(g, f(ALIGN_GAIN_MIN)), f(ALIGN_GAIN_MAX))
            gm = g * mean[k]
            o = mean[0] - gm
            if all(np.isfinite(v) for v in (g, o, C[0, 0], C[k, k], C[0, k])):
                out[k] = (np.float32(g), np.float32(o))
    return out, (mean, C)


def _check_members(members):
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
    return members


def _check_clips(members):
    first = members[0]
    if first.ndim < 2 or first.shape[0] < 1 or first.numel() == 0:
        raise ValueError(f"aligned members are [B, ..., 3] clips with B >= 1 and something in them, got {tuple(first.shape)}")
    if first.numel() // first.shape[0] > ALIGN_MAX_CLIP:
        raise ValueError(f"a clip of more than 2^36 bytes cannot be aligned, got {first.numel() // first.shape[0]}")


def align_members(members: Sequence[torch.Tensor], backend: str = "auto") -> torch.Tensor:
    """N uint8 tensors [B, ..., 3] of one shape on one device (clip b = member[b]) -> fp32 [N, B, 2] on that device: member k's
    (g, o) for clip b, by align_solve_members from the sums over all of the clip's bytes (one pair for the three channels).

    backend: 'auto' = the HIP kernels (drn_ensemble_align_affine: two launches, the affines never leave the device, nothing
    synchronises) on GPU tensors and torch / numpy on CPU tensors; 'torch' / 'hip' force a path ('hip' needs GPU tensors).  The
    torch path is the specification: the sums as float64 products on the members' device - integers below 2^53, so exact in any
    order -, the rule in numpy on the host (on GPU tensors this path synchronises)."""
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    members = _check_members(members)
    _check_clips(members)
    first = members[0]
    if backend == "hip" and not first.is_cuda:
        raise ValueError(f"backend='hip' needs GPU tensors, got them on {first.device} (the torch path is what CPU devices run)")
    if backend != "torch" and first.is_cuda:
        from . import native
        return native.ensemble_align_affine([m.contiguous() for m in members])
    N, B = len(members), first.shape[0]
    n = first.numel() // B
    out = np.empty((N, B, 2), dtype=np.float32)
    for b in range(B):
        X = torch.stack([m[b].reshape(-1) for m in members]).to(torch.float64)
        S = X.sum(dim=1).cpu().numpy().astype(np.int64)
        G = (X @ X.t()).cpu().numpy().astype(np.int64)
        del X
        out[:, b], _ = align_solve_members(n, S, G)
    return torch.from_numpy(out).to(first.device)


def apply_affine_u8(member: torch.Tensor, affine: torch.Tensor) -> torch.Tensor:
    """A member [B, ..., 3] uint8 read through its affines [B, 2] fp32: every byte x of clip b ->
    u8(rint(clamp(fp32(g * fp32(x)) + o, 0, 255))): two separately rounded fp32 operations (torch never fuses two ops), the clamp,
    then round half to even.  (1, 0) gives the byte back."""
    shape = (-1,) + (1,) * (member.ndim - 1)
    g = affine[:, 0].to(torch.float32).reshape(shape)
    o = affine[:, 1].to(torch.float32).reshape(shape)
    return torch.round(torch.clamp(member.to(torch.float32) * g + o, 0.0, 255.0)).to(torch.uint8)


def _check_affine(members, mode, affine):
    if mode == "normal":
        raise ValueError("normal maps are never aligned: an affine goes with 'median' or 'mean'")
    _check_clips(members)
    first = members[0]
    if not isinstance(affine, torch.Tensor) or affine.dtype != torch.float32 or \
            tuple(affine.shape) != (len(members), first.shape[0], 2) or affine.device != first.device:
        raise ValueError(f"affine must be fp32 [N, B, 2] = {(len(members), first.shape[0], 2)} on {first.device}")


def reduce_members(members: Sequence[torch.Tensor], mode: str, spread: bool = False,
                   backend: str = "auto", affine: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """N uint8 tensors of one shape [..., 3] on one device (1 <= N <= 16; they need not be contiguous with each other) -> (the
    per-pixel reduce under `mode`, the members' spread around it or None), both uint8 of the members' shape.  N = 1: 'median'
    and 'mean' copy the member (spread 0); 'normal' still renormalises it.

    backend: 'auto' = the HIP kernel (drn_ensemble_reduce_u8, one launch, no stack of the members) on GPU tensors and torch on
    CPU tensors; 'torch' / 'hip' force a path ('hip' needs GPU tensors).  The torch path is the specification and what CPU
    devices run.

    affine (ensembles that agree; 'median' and 'mean' only, members [B, ..., 3]): fp32 [N, B, 2] on the members' device, finite, as
    align_members returns it: member k's bytes of clip b are read through apply_affine_u8 in front of the reduce, and the spread
    is taken around the aligned members (drn_ensemble_reduce_affine_u8: still one launch).  None: today's reduce."""
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    members = _check_members(members)
    first = members[0]
    if affine is not None:
        _check_affine(members, mode, affine)
    if backend == "hip" and not first.is_cuda:
        raise ValueError(f"backend='hip' needs GPU tensors, got them on {first.device} (the torch path is what CPU devices run)")
    if backend == "torch" or not first.is_cuda or first.numel() == 0:
        if affine is not None:
            members = [apply_affine_u8(m, affine[k]) for k, m in enumerate(members)]
        return _reduce_torch(members, mode, bool(spread))
    from . import native
    if affine is not None:
        return native.ensemble_reduce_affine_u8([m.contiguous() for m in members], affine.contiguous(), mode, bool(spread))
    return native.ensemble_reduce_u8([m.contiguous() for m in members], mode, bool(spread))


def reduce_results(member_outs: List[list], flags, reduce: str, spread: bool = False, align: bool = False):
    """The pipeline's walk over N members' results: member_outs[k][c][p] = member k's uint8 result of batch c and pass p,
    flags[c][p] = that pass's normalize_normal flag -> (results[c][p], spreads[c][p] or None) with the mode 'normal' where the flag
    is set and `reduce` elsewhere.  A member's tensors are dropped from `member_outs` as soon as their pass is reduced.

    align (ensembles that agree): every pass whose flag is not set is first solved (align_members) and then reduced through its
    affines; a normal pass is never aligned.  The return then has a third entry, affines[c][p]: the fp32 [N, B, 2] tensor on the
    members' device, or None for a normal pass.  Off, the walk makes exactly the calls it made before the switch existed."""
    results, spreads, affines = [], [], []
    for c, fl in enumerate(flags):
        results.append([])
        spreads.append([])
        affines.append([])
        for p, flag in enumerate(fl):
            mem = [outs[c][p] for outs in member_outs]
            for outs in member_outs:
                outs[c][p] = None
            if align and not flag:
                a = align_members(mem)
                r, s = reduce_members(mem, reduce, spread=spread, affine=a)
            else:
                a = None
                r, s = reduce_members(mem, "normal" if flag else reduce, spread=spread)
            del mem
            results[-1].append(r)
            spreads[-1].append(s)
            affines[-1].append(a)
    return (results, spreads, affines) if align else (results, spreads)
