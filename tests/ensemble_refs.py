"""Seed ensembles: the reference of drn_ensemble_reduce_u8 / ensemble.reduce_members written out in numpy, independently of
ensemble.py (np.sort, integer arithmetic, np.float32 operation by operation), the case grid that the CPU and the GPU tests share,
the wrong stand-ins the grid has to tell from the reference, and the synthetic scene of the robustness figures."""
import zlib

import numpy as np

MODES = ("median", "mean", "normal")
F = np.float32

# one sweep of the kernel's capped grid (csrc/ensemble.hip: 2048 workgroups of 256 lanes): 16 bytes per lane on the aligned path
# (48 in 'normal'), one byte (one pixel) per lane on the ragged one
SWEEP_LANES = 2048 * 256


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ----------------------------------------------------------------------------------------------- the reference
def _mid_half_even(lo, hi):
    t = lo + hi
    r = t >> 1
    return r + (t & 1) * (r & 1)


def _median(stack):
    s = np.sort(stack, axis=0)
    N = stack.shape[0]
    return _mid_half_even(s[(N - 1) // 2], s[N // 2])


def _mean(stack):
    N = stack.shape[0]
    S = stack.sum(axis=0)
    q, rem = np.divmod(S, N)
    up = (2 * rem > N) | ((2 * rem == N) & (q % 2 == 1))
    return q + up


UNIT = (np.arange(256, dtype=F) / F(255.0)).astype(F)               # numpy's fp32 division is correctly rounded


def decode(m, unit=UNIT):
    return (unit[m] * F(2.0) - F(1.0)).astype(F)


def normal_sum(members, unit=UNIT):
    s = decode(members[0], unit)
    for m in members[1:]:
        s = (s + decode(m, unit)).astype(F)
    return s.reshape(-1, 3)


def normal_finish(s, N, fused_l2=False, renormalise=True):
    sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
    if fused_l2:            # l2 as two fused multiply-adds would give it: each product unrounded inside its sum
        t = (sy.astype(np.float64) * sy + (sx * sx).astype(F)).astype(F)
        l2 = (sz.astype(np.float64) * sz + t).astype(F)
    else:
        l2 = ((sx * sx + sy * sy).astype(F) + sz * sz).astype(F)
    l = np.sqrt(l2).astype(F)
    d = np.maximum(l, F(1e-6))
    n = (s / d[:, None]).astype(F) if renormalise else (s / F(N)).astype(F)
    r = np.rint(np.clip(((n + F(1.0)).astype(F) * F(127.5)).astype(F), F(0.0), F(255.0))).astype(np.uint8)
    e = (F(1.0) - (l / F(N)).astype(F)).astype(F)
    sp = np.rint((F(255.0) * np.clip(e, F(0.0), F(1.0))).astype(F)).astype(np.uint8)
    return r.reshape(-1), np.repeat(sp, 3)


def reduce_ref(members, mode, spread=False):
    """members: N flat uint8 arrays of one length (a multiple of 3 in 'normal') -> (result, spread or None), flat uint8."""
    N = len(members)
    assert 1 <= N <= 16 and mode in MODES
    if mode == "normal":
        r, sp = normal_finish(normal_sum(members), N)
        return r, (sp if spread else None)
    stat = _median if mode == "median" else _mean
    stack = np.stack([m.astype(np.int64) for m in members])
    r = stat(stack)
    sp = stat(np.abs(stack - r)).astype(np.uint8) if spread else None
    return r.astype(np.uint8), sp


# ----------------------------------------------------------------------------------------------- the case grid
def _pad3(cols):
    """[N, n] -> [N, n rounded up to a multiple of 3] (zeros)."""
    n = cols.shape[1]
    return np.ascontiguousarray(np.pad(cols, ((0, 0), (0, (-n) % 3))).astype(np.uint8))


def _value_sets(N, rng):
    """Columns of N bytes: all members equal, one outlier at every position, 0 / 255 extremes in every split, ties from a small
    alphabet, neighbours (what half-to-even sees), random."""
    cols = []
    for v in (0, 1, 2, 127, 128, 254, 255):
        cols.append([v] * N)
    for base, out in ((100, 255), (100, 0), (3, 200), (254, 1)):
        for j in range(N):
            c = [base] * N
            c[j] = out
            cols.append(c)
    for k in range(N + 1):
        cols.append([0] * k + [255] * (N - k))
        cols.append([255] * k + [0] * (N - k))
    alphabet = np.array([0, 1, 2, 3, 126, 127, 128, 129, 253, 254, 255])
    cols.extend(alphabet[rng.integers(0, len(alphabet), size=(240, N))].tolist())
    cols.extend((rng.integers(0, 254, size=(120, 1)) + rng.integers(0, 3, size=(120, N))).tolist())
    cols.extend(rng.integers(0, 256, size=(240, N)).tolist())
    return _pad3(np.array(cols, dtype=np.int64).T)


def _unit_bytes(v):
    return np.rint(np.clip((v + 1.0) * 127.5, 0, 255)).astype(np.uint8)


def _normal_sets(N, rng):
    """Pixels of N members for 'normal': members equal, opposite vectors (0 against 255 sums to exactly zero), nearly opposite
    ones (i against 255 - i), the 256 byte values on each axis, random unit vectors quantised to bytes with per-member noise."""
    px = []
    v = np.arange(256)
    mid = np.full(256, 128)
    for axis in range(3):
        one = [mid, mid, mid]
        one[axis] = v
        p = np.stack(one, 1)                                   # [256, 3]
        px.append(np.repeat(p[None], N, 0))                    # members equal
        if N >= 2:
            q = np.repeat(p[None], N, 0).copy()
            q[1::2] = 255 - q[1::2]                            # every second member turned round: nearly opposite
            px.append(q)
    if N >= 2 and N % 2 == 0:
        ext = rng.integers(0, 2, size=(64, 3)) * 255           # corners of the cube: +-1 exactly
        q = np.repeat(ext[None], N, 0)
        q[1::2] = 255 - q[1::2]                                # the sum is exactly zero: 128, 128, 128 and spread 255
        px.append(q)
    u = rng.normal(size=(600, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    noisy = u[None] + 0.15 * rng.normal(size=(N, 600, 3))
    noisy /= np.linalg.norm(noisy, axis=2, keepdims=True)
    px.append(_unit_bytes(noisy))
    px.append(rng.integers(0, 256, size=(N, 300, 3)))
    return np.ascontiguousarray(np.concatenate(px, 1).reshape(N, -1).astype(np.uint8))


def byte_pairs():
    """All 65 536 byte pairs as two members (padded to whole pixels)."""
    a = np.repeat(np.arange(256), 256)
    b = np.tile(np.arange(256), 256)
    return _pad3(np.stack([a, b]))


# pixels whose sum with the member (0, 0, 0) has an l2 that two fused multiply-adds round differently from the three products
# and two sums of the specification, far enough to move a result byte (found by search over all pixels; a random pixel does
# so with probability of about 1e-5, which only the sweep cases reach)
FMA_PIXELS = ((129, 3, 3), (3, 129, 3), (255, 69, 7), (69, 255, 7), (211, 35, 13), (35, 211, 13), (95, 118, 14), (143, 84, 20),
              (84, 143, 20), (84, 57, 21), (112, 58, 25), (58, 112, 25), (143, 31, 31), (31, 143, 31), (145, 35, 35),
              (153, 150, 36), (91, 11, 37), (11, 91, 37), (46, 1, 42), (42, 1, 46), (239, 23, 47), (151, 47, 47), (47, 151, 47),
              (238, 51, 51))

SIZES = tuple(range(3, 772, 3))
SET_N = (3, 4, 5, 8, 16)


def cases(big=True):
    """-> (name, mode, members [N, n_bytes] uint8) for: every size 3, 6, ... 771 (N cycling through 1..16, every mode), every N at
    771 bytes in every mode, all byte pairs at N = 2, the value sets and the normal sets at N = 3, 4, 5, 8, 16 (the normal sets
    also at 1 and 2), the pixels that see a fused l2, and - `big` - sizes past one sweep of the capped grid on the aligned and on
    the ragged path."""
    for i, n in enumerate(SIZES):
        N = 1 + i % 16
        for mode in MODES:
            yield f"size.{n}.n{N}.{mode}", mode, _rng(f"size.{n}.{mode}").integers(0, 256, size=(N, n), dtype=np.uint8)
    for N in range(1, 17):
        for mode in MODES:
            yield f"members.n{N}.{mode}", mode, _rng(f"members.{N}.{mode}").integers(0, 256, size=(N, 771), dtype=np.uint8)
    for mode in ("median", "mean"):
        yield f"pairs.{mode}", mode, byte_pairs()
    for N in SET_N:
        sets = _value_sets(N, _rng(f"sets.{N}"))
        for mode in ("median", "mean"):
            yield f"sets.n{N}.{mode}", mode, sets
    for N in (1, 2) + SET_N:
        yield f"normals.n{N}", "normal", _normal_sets(N, _rng(f"normals.{N}"))
    fma = np.array(FMA_PIXELS, dtype=np.uint8).reshape(-1)
    yield "normals.fma", "normal", np.stack([fma, np.zeros_like(fma)])
    if big:
        yield from big_cases()


def big_cases():
    """Past one sweep of the capped grid: 16 (48) bytes per lane where all bases are aligned, one byte (pixel) per lane otherwise
    (the GPU test runs the `.ragged` ones off the 16-byte grid; on the CPU they are sizes like any other)."""
    more = 48 * 37 + 9
    up3 = lambda n: n + (-n) % 3                                   # whole pixels in every mode: the members are [..., 3] tensors
    for mode, N, n in (("median", 3, SWEEP_LANES * 16 + more), ("normal", 2, SWEEP_LANES * 48 + more),
                       ("mean", 2, SWEEP_LANES * 16 + more)):
        yield f"sweep.{mode}", mode, _rng(f"sweep.{mode}").integers(0, 256, size=(N, up3(n)), dtype=np.uint8)
    for mode, N, n in (("median", 2, SWEEP_LANES + more), ("mean", 3, SWEEP_LANES + more), ("normal", 2, SWEEP_LANES * 3 + more)):
        yield f"sweep.{mode}.ragged", mode, _rng(f"sweep.ragged.{mode}").integers(0, 256, size=(N, up3(n)), dtype=np.uint8)


# ----------------------------------------------------------------------------------------------- wrong stand-ins
def _stat_of(mode):
    return _median if mode == "median" else _mean


def _bytewise(members, mode, spread, centre=None, stat=None, spread_stat=None, spread_centre=None):
    stack = np.stack([m.astype(np.int64) for m in members])
    stat = stat or _stat_of(mode)
    r = stat(stack) if centre is None else centre(stack)
    sp = None
    if spread:
        c = r if spread_centre is None else spread_centre(stack)
        sp = (spread_stat or stat)(np.abs(stack - c)).astype(np.uint8)
    return r.astype(np.uint8), sp


def _sorted_pick(which):
    def stat(stack):
        s = np.sort(stack, axis=0)
        N = stack.shape[0]
        return s[(N - 1) // 2] if which == "lower" else s[N // 2]
    return stat


def _median_half_up(stack):
    s = np.sort(stack, axis=0)
    N = stack.shape[0]
    return (s[(N - 1) // 2] + s[N // 2] + 1) >> 1


def _mean_half_up(stack):
    N = stack.shape[0]
    return (2 * stack.sum(axis=0) + N) // (2 * N)


def _late(out):
    r, sp = out
    shift = lambda a: None if a is None else np.concatenate([a[:1], a[:-1]])
    return shift(r), shift(sp)


def wrong(kind, members, mode, spread=False):
    """The reduce as a wrong kernel of `kind` would compute it (kinds that do not touch `mode` return the reference)."""
    members = list(members)
    N = len(members)
    ref = lambda: reduce_ref(members, mode, spread)
    if kind == "upper_median":
        return _bytewise(members, mode, spread, stat=_sorted_pick("upper")) if mode == "median" else ref()
    if kind == "lower_median":
        return _bytewise(members, mode, spread, stat=_sorted_pick("lower")) if mode == "median" else ref()
    if kind == "median_half_up":
        return _bytewise(members, mode, spread, stat=_median_half_up) if mode == "median" else ref()
    if kind == "mean_half_up":
        return _bytewise(members, mode, spread, stat=_mean_half_up) if mode == "mean" else ref()
    if kind == "mean_truncated":
        return _bytewise(members, mode, spread, stat=lambda st: st.sum(axis=0) // st.shape[0]) if mode == "mean" else ref()
    if kind == "mean_for_median":
        return _bytewise(members, mode, spread, stat=_mean) if mode == "median" else ref()
    if kind == "member0_only":
        return reduce_ref(members[:1], mode, spread)
    if kind == "last_member_dropped":
        return reduce_ref(members[:-1], mode, spread) if N > 1 else ref()
    if kind == "late_byte":
        return _late(ref())
    if kind == "spread_wrong_centre":          # deviations taken around member 0 instead of the result
        if mode == "normal" or not spread:
            return ref()
        return _bytewise(members, mode, spread, spread_centre=lambda st: st[0])
    if mode != "normal":
        return ref()
    if kind == "channelwise_median_normal":
        return reduce_ref(members, "median", spread)
    if kind == "no_renormalisation":
        r, sp = normal_finish(normal_sum(members), N, renormalise=False)
        return r, (sp if spread else None)
    if kind == "reciprocal_255":
        unit = (np.arange(256, dtype=F) * (F(1.0) / F(255.0))).astype(F)
        r, sp = normal_finish(normal_sum(members, unit), N)
        return r, (sp if spread else None)
    if kind == "fused_l2":
        r, sp = normal_finish(normal_sum(members), N, fused_l2=True)
        return r, (sp if spread else None)
    raise KeyError(kind)


# stand-in -> the named case of the grid that tells it from the reference (tests/test_ensemble_cpu.py checks each; the
# spread_wrong_centre entry is seen in the spread)
WRONG = {
    "upper_median": "pairs.median",
    "lower_median": "pairs.median",
    "median_half_up": "pairs.median",
    "mean_half_up": "pairs.mean",
    "mean_truncated": "pairs.mean",
    "mean_for_median": "sets.n3.median",
    "member0_only": "sets.n5.median",
    "last_member_dropped": "sets.n4.mean",
    "late_byte": "size.6.n2.median",
    "spread_wrong_centre": "sets.n8.median",
    "channelwise_median_normal": "normals.n3",
    "no_renormalisation": "normals.n5",
    "reciprocal_255": "normals.n2",
    "fused_l2": "normals.fma",
}


# ----------------------------------------------------------------------------------------------- robustness
def synthetic_scene(N=5, h=48, w=64, outliers=0.2, noise=6.0):
    """A deterministic scene: a smooth colour picture and a smooth normal map as the truth; member k = truth + Gaussian noise,
    with `outliers` of its pixels replaced by salt (a random colour / a random direction).  -> (truth colour [h*w*3] uint8,
    colour members [N, h*w*3], truth normals [h*w, 3] float64 unit vectors, normal members [N, h*w*3])."""
    rng = _rng("scene")
    y, x = np.mgrid[0:h, 0:w]
    colour = np.stack([128 + 100 * np.sin(x / 9.0), 128 + 100 * np.cos(y / 7.0), 128 + 60 * np.sin((x + y) / 11.0)], -1)
    nrm = np.stack([np.sin(x / 13.0) * 0.6, np.cos(y / 10.0) * 0.6, np.ones_like(x, dtype=np.float64)], -1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    truth_c = np.rint(np.clip(colour, 0, 255)).astype(np.uint8).reshape(-1)
    cm, nm = [], []
    for _ in range(N):
        c = np.clip(colour + noise * rng.normal(size=colour.shape), 0, 255)
        salt = rng.random(size=(h, w)) < outliers
        c[salt] = rng.integers(0, 256, size=(int(salt.sum()), 3))
        cm.append(np.rint(c).astype(np.uint8).reshape(-1))
        v = nrm + (noise / 127.5) * rng.normal(size=nrm.shape)
        salt = rng.random(size=(h, w)) < outliers
        r = rng.normal(size=(int(salt.sum()), 3))
        v[salt] = r
        v /= np.linalg.norm(v, axis=-1, keepdims=True)
        nm.append(_unit_bytes(v).reshape(-1))
    return truth_c, np.stack(cm), nrm.reshape(-1, 3), np.stack(nm)


def angular_error_deg(bytes_flat, truth):
    v = bytes_flat.reshape(-1, 3).astype(np.float64) / 127.5 - 1.0
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    return float(np.degrees(np.arccos(np.clip((v * truth).sum(1), -1.0, 1.0))).mean())


def robustness_figures(N=5):
    """-> dict: the mean absolute error of every colour member and of their median and mean, and the mean angular error (degrees)
    of every normal member and of the 'normal' reduce, on synthetic_scene."""
    truth_c, cm, truth_n, nm = synthetic_scene(N)
    mae = lambda a: float(np.abs(a.astype(np.int64) - truth_c.astype(np.int64)).mean())
    return {"member_mae": [mae(m) for m in cm], "median_mae": mae(reduce_ref(list(cm), "median")[0]),
            "mean_mae": mae(reduce_ref(list(cm), "mean")[0]),
            "member_deg": [angular_error_deg(m, truth_n) for m in nm],
            "normal_deg": angular_error_deg(reduce_ref(list(nm), "normal")[0], truth_n)}
