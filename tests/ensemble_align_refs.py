"""Ensembles that agree: the reference of drn_ensemble_align_affine / ensemble.align_members and of
drn_ensemble_reduce_affine_u8 / ensemble.reduce_members(affine=...) written out in numpy, independently of ensemble.py - the sums
in plain int64 arithmetic, the rule in np.float64 scalars operation by operation, the apply in np.float32 operation by operation,
the reduce behind it by tests/ensemble_refs.py -, the case grids that the CPU and the GPU tests share, the wrong stand-ins the
grids have to tell from the reference, and the synthetic scene of the robustness figures."""
import zlib
from fractions import Fraction

import numpy as np

import ensemble_refs as R

F = np.float32
D = np.float64
FLAT = 2.0 ** -6
CHUNK = 8192                         # csrc/ensemble_align.hip: bytes of one clip per 32-bit partial
SOLVE_WAVES = 1024 * 4               # its waves per clip, a chunk each: one sweep of the solve is SOLVE_WAVES * CHUNK bytes
SOLVE_THREADS = 1024                 # the second launch's workgroup
SWEEP_LANES = R.SWEEP_LANES          # csrc/ensemble.hip: lanes of the capped grid, per clip row in the affine reduce


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ----------------------------------------------------------------------------------------------- the solve
def sums_ref(clip):
    """clip [N, n] uint8 -> (S [N], G [N][N]) as Python integers: S_k = sum m_k, G_jk = sum m_j m_k, in int64, block by block."""
    N, n = clip.shape
    S = [0] * N
    G = [[0] * N for _ in range(N)]
    for lo in range(0, n, 1 << 20):
        x = clip[:, lo:lo + (1 << 20)].astype(np.int64)
        for k in range(N):
            S[k] += int(x[k].sum())
        for j in range(N):
            for k in range(j, N):
                G[j][k] += int((x[j] * x[k]).sum())
    for j in range(N):
        for k in range(j):
            G[j][k] = G[k][j]
    return S, G


def _fma_c(e, a, b):
    """e - a * b with one rounding, as a fused multiply-add gives it."""
    return D(float(Fraction(float(e)) - Fraction(float(a)) * Fraction(float(b))))


def solve_ref(n, S, G, wrong=None):
    """The rule from the exact sums of one clip -> (affine float32 [N, 2], stats float64 [N + N * N] = means, then C row by row).
    wrong: the name of a stand-in (see SOLVE_WRONG) that changes the rule itself."""
    N = len(S)
    with np.errstate(all="ignore"):
        nn = D(n)
        mean = [D(S[k]) / nn for k in range(N)]
        C = [[D(0)] * N for _ in range(N)]
        for j in range(N):
            for k in range(N):
                lo, hi = min(j, k), max(j, k)
                if wrong == "sample_moments":
                    C[j][k] = (D(G[lo][hi]) - D(S[lo]) * D(S[hi]) / nn) / (nn - D(1))
                elif wrong == "fma_in_C":
                    C[j][k] = _fma_c(D(G[lo][hi]) / nn, mean[lo], mean[hi])
                else:
                    e = D(G[lo][hi]) / nn
                    mm = mean[lo] * mean[hi]
                    C[j][k] = e - mm
        aff = np.zeros((N, 2), dtype=F)
        aff[:, 0] = 1.0
        for k in range(1, N):
            g = None
            if N >= 3 and wrong != "moment_matching_only":
                num, den = D(0.0), D(0.0)
                for j in range(N):
                    if j == 0 and wrong != "j0_left_in":
                        continue
                    if j == k and wrong != "jk_left_in":
                        continue
                    num = num + C[0][j]
                    den = den + C[k][j]
                if np.isfinite(num) and np.isfinite(den) and num >= FLAT and den >= FLAT:
                    g = den / num if wrong == "ratio_inverted" else num / den
            if g is None:
                g = D(1.0)
                if C[0][0] >= FLAT and C[k][k] >= FLAT and C[0][k] > 0:
                    g = np.sqrt(C[0][0] / C[k][k])
            raw = g
            g = D(min(max(g, D(0.5)), D(2.0)))
            o = mean[0] - (raw if wrong == "o_from_unclamped_g" else g) * mean[k]
            if all(np.isfinite(v) for v in (g, o, C[0][0], C[k][k], C[0][k])):
                aff[k] = (F(g), F(o))
    stats = np.array(mean + [C[j][k] for j in range(N) for k in range(N)], dtype=D)
    return aff, stats


def _carry32(clip):
    """The sums as the second launch would add them with 32-bit accumulators: thread t of R * Q walks the partials of its sum with
    the stride R (R = 1024 / Q rows), wrapping at 2^32; the rows are then added exactly."""
    N, n = clip.shape
    Q = N + N * (N + 1) // 2
    rows = SOLVE_THREADS // Q
    nch = -(-n // CHUNK)

    def per_chunk(j, k):
        out = np.zeros(nch, dtype=np.int64)
        for lo in range(0, nch, 256):
            a = clip[j, lo * CHUNK:(lo + 256) * CHUNK].astype(np.int64)
            v = a if k is None else a * clip[k, lo * CHUNK:(lo + 256) * CHUNK].astype(np.int64)
            v = np.pad(v, (0, (-v.size) % CHUNK)).reshape(-1, CHUNK).sum(axis=1)
            out[lo:lo + v.size] = v
        return out

    def total(pc):
        return sum(int(pc[r::rows].sum()) % (1 << 32) for r in range(rows))
    S = [total(per_chunk(k, None)) for k in range(N)]
    G = [[0] * N for _ in range(N)]
    for j in range(N):
        for k in range(j, N):
            G[j][k] = G[k][j] = total(per_chunk(j, k))
    return S, G


def align_ref(mem, wrong=None):
    """mem [N, B, n] uint8 -> (affine float32 [N, B, 2], stats float64 [B, N + N * N])."""
    N, B, n = mem.shape
    aff = np.zeros((N, B, 2), dtype=F)
    stats = np.zeros((B, N + N * N), dtype=D)
    for b in range(B):
        clip = mem[:, 0 if wrong == "clip0_sums" else b]
        if wrong == "members_shifted":
            clip = np.roll(clip, 1, axis=0)
        S, G = _carry32(clip) if wrong == "carry32" else sums_ref(clip)
        rule = wrong if wrong in ("moment_matching_only", "j0_left_in", "jk_left_in", "ratio_inverted", "o_from_unclamped_g",
                                  "sample_moments", "fma_in_C") else None
        aff[:, b], stats[b] = solve_ref(n, S, G, rule)
    return aff, stats


def align_brute(mem):
    """The affines by a brute-force float64 evaluation: centred moments of the float members, no integer sums -> float64
    [N, B, 2] (not rounded to fp32); agrees with align_ref to rounding error away from the rule's thresholds."""
    N, B, n = mem.shape
    out = np.zeros((N, B, 2))
    out[:, :, 0] = 1.0
    for b in range(B):
        X = mem[:, b].astype(D)
        mean = X.mean(axis=1)
        Xc = X - mean[:, None]
        C = Xc @ Xc.T / n
        for k in range(1, N):
            js = [j for j in range(N) if j not in (0, k)]
            num, den = sum(C[0, j] for j in js), sum(C[k, j] for j in js)
            if N >= 3 and num >= FLAT and den >= FLAT:
                g = num / den
            elif C[0, 0] >= FLAT and C[k, k] >= FLAT and C[0, k] > 0:
                g = np.sqrt(C[0, 0] / C[k, k])
            else:
                g = 1.0
            g = min(max(g, 0.5), 2.0)
            out[k, b] = (g, mean[0] - g * mean[k])
    return out


def scene(name, N, B, n, gains=None, offsets=None, noise=3.0):
    """Members with structure: a smooth truth per clip, member k = g_k * truth + o_k + noise -> [N, B, n] uint8."""
    rng = _rng(name)
    gains = gains if gains is not None else [1.0] + list(rng.uniform(0.6, 1.6, size=N - 1))
    offsets = offsets if offsets is not None else [0.0] + list(rng.uniform(-30, 30, size=N - 1))
    i = np.arange(n)
    mem = np.zeros((N, B, n))
    for b in range(B):
        truth = 110 + 60 * np.sin(i / (5.0 + 2 * b)) + 25 * np.cos(i / 37.0 + b) + (18 * b)
        for k in range(N):
            mem[k, b] = gains[k] * truth + offsets[k] + noise * rng.normal(size=n)
    return np.rint(np.clip(mem, 0, 255)).astype(np.uint8)


SOLVE_SIZES = (1, 3, 15, 16, 17, 8191, 8192, 8193, 3 * 8192 + 5)
SOLVE_VEC = 1008                     # 63 groups of 16 bytes and 336 whole pixels: the wide path at every N
SOLVE_BIG = (SOLVE_WAVES + 3) * CHUNK + 16           # past one sweep; whole groups of 16 and whole pixels


def solve_cases(big=True):
    """-> (name, members [N, B, n] uint8): every N at 771 bytes and at 1008 (whole groups of 16: the wide path where the bases
    allow it), every size of SOLVE_SIZES at B = 1..3, one case per branch of the rule, and - `big` - every byte 255 at N = 3 past
    one sweep of the capped grid."""
    for N in range(1, 17):
        yield f"members.n{N}", scene(f"members.{N}", N, 1, 771)
        yield f"wide.n{N}", scene(f"wide.{N}", N, 2, SOLVE_VEC)
    for i, n in enumerate(SOLVE_SIZES):
        for B in (1, 2, 3):
            N = 2 + (i + B) % 5
            yield f"size.{n}.b{B}", scene(f"size.{n}.{B}", N, B, n)
    yield "branch.n2", scene("branch.n2", 2, 2, 771, gains=[1.0, 1.4], offsets=[0.0, -20.0])
    flat = scene("branch.flat", 3, 1, 771)
    flat[1] = 77                                                     # a flat member: nothing to match, g = 1
    yield "branch.flat", flat
    anti = scene("branch.anti", 2, 1, 771, gains=[1.0, 1.0], offsets=[0.0, 0.0])
    anti[1] = 255 - anti[1]                                          # C_01 <= 0: contents that disagree
    yield "branch.anti", anti
    rng = _rng("branch.num")
    num = scene("branch.num_flat", 3, 1, 771, gains=[1.0, 0.8, 1.2], offsets=[0.0, 10.0, -10.0])
    num[2, 0] = rng.permutation(num[2, 0])                           # member 2 shares nothing: num = C_02 and den = C_12 ~ 0
    yield "branch.num_flat", num
    den = scene("branch.den_flat", 3, 1, 771, gains=[1.0, 0.8, 1.2], offsets=[0.0, 10.0, -10.0])
    den[1, 0] = rng.permutation(den[1, 0])                           # member 1 shares nothing: its den = C_12 ~ 0, num = C_02 is fine
    yield "branch.den_flat", den
    yield "branch.clamp_hi", scene("branch.hi", 4, 1, 771, gains=[1.0, 0.3, 0.35, 0.32], offsets=[0.0, 40.0, 30.0, 20.0], noise=0.5)
    yield "branch.clamp_lo", scene("branch.lo", 4, 1, 771, gains=[0.3, 1.0, 0.9, 1.1], offsets=[40.0, 0.0, 5.0, -5.0], noise=0.5)
    yield "clips.b3", scene("clips.b3", 4, 3, 771)
    if big:
        yield "sweep.255", np.full((3, 1, SOLVE_BIG), 255, dtype=np.uint8)


# stand-in -> the named case that tells it from the reference (in the affines, or - the two that only move the last bits of the
# moments or only the moments of a flat clip - in the stats)
SOLVE_WRONG = {
    "moment_matching_only": "members.n5",
    "j0_left_in": "members.n4",
    "jk_left_in": "members.n4",
    "ratio_inverted": "members.n3",
    "o_from_unclamped_g": "branch.clamp_hi",
    "sample_moments": "size.17.b1",
    "clip0_sums": "clips.b3",
    "members_shifted": "members.n6",
    "carry32": "sweep.255",
    "fma_in_C": "members.n7",
}


# ----------------------------------------------------------------------------------------------- the reduce behind an affine
def apply_ref(m, g, o, fused=False, truncate=False, clamp=True):
    """A member's bytes through (g, o): fp32(g * fp32(x)), + o, clamp, half to even.  The keywords are the stand-ins."""
    x = m.astype(F)
    if fused:
        a = (np.float64(g) * x.astype(D) + np.float64(o)).astype(F)  # the product of two fp32 values is exact in float64
    else:
        a = ((F(g) * x).astype(F) + F(o)).astype(F)
    if clamp:
        a = np.clip(a, F(0.0), F(255.0))
    a = np.floor(a) if truncate else np.rint(a)
    return a.astype(np.int64).astype(np.uint8)                       # without the clamp: wrapped


def aligned_ref(mem, aff, **kw):
    """mem [N, B, n], aff [N, B, 2] -> the aligned members [N, B, n]."""
    out = np.empty_like(mem)
    for k in range(mem.shape[0]):
        for b in range(mem.shape[1]):
            out[k, b] = apply_ref(mem[k, b], aff[k, b, 0], aff[k, b, 1], **kw)
    return out


def reduce_affine_ref(mem, aff, mode, spread=False, wrong=None):
    """-> (result [B * n], spread [B * n] or None), flat uint8."""
    N, B, n = mem.shape
    flat = lambda a: [a[k].reshape(-1) for k in range(N)]
    if wrong == "fused":
        return R.reduce_ref(flat(aligned_ref(mem, aff, fused=True)), mode, spread)
    if wrong == "truncated":
        return R.reduce_ref(flat(aligned_ref(mem, aff, truncate=True)), mode, spread)
    if wrong == "no_clamp":
        return R.reduce_ref(flat(aligned_ref(mem, aff, clamp=False)), mode, spread)
    if wrong == "affine_after_the_reduce":                           # the raw members reduced, then member 1's pair on the result
        r, sp = R.reduce_ref(flat(mem), mode, spread)
        k = min(1, N - 1)
        return aligned_ref(r.reshape(1, B, n), aff[k:k + 1]).reshape(-1), sp
    if wrong == "clip0_affine":
        return R.reduce_ref(flat(aligned_ref(mem, np.repeat(aff[:, :1], B, axis=1))), mode, spread)
    if wrong == "member0_affine":
        return R.reduce_ref(flat(aligned_ref(mem, np.repeat(aff[:1], N, axis=0))), mode, spread)
    if wrong == "spread_around_the_unaligned":
        r, _ = R.reduce_ref(flat(aligned_ref(mem, aff)), mode, False)
        stat = R._median if mode == "median" else R._mean
        sp = stat(np.abs(np.stack([m.astype(np.int64) for m in flat(mem)]) - r.astype(np.int64))).astype(np.uint8)
        return r, (sp if spread else None)
    if wrong == "straddling_group_first_clip":                       # groups of 16 over the flat buffer take their first byte's clip
        idx = np.arange(B * n)
        clip_of = (idx // 16 * 16) // n
        al = np.empty((N, B * n), dtype=np.uint8)
        for k in range(N):
            fk = mem[k].reshape(-1)
            for b in range(B):
                sel = clip_of == b
                al[k, sel] = apply_ref(fk[sel], aff[k, b, 0], aff[k, b, 1])
        return R.reduce_ref(list(al), mode, spread)
    assert wrong is None, wrong
    return R.reduce_ref(flat(aligned_ref(mem, aff)), mode, spread)


# (g, o, x) as fp32 hex: fp32(fp32(g x) + o) and the fused g x + o round to different bytes (found by search on the CPU)
FMA_TRIPLES = (("0x1.41bf1cp+0", "-0x1.6e21dep+5", 149), ("0x1.fe45a8p+0", "-0x1.a2381cp+7", 206), ("0x1.a55b6ap-1", "-0x1.108522p+7", 216),
               ("0x1.6b3718p+0", "-0x1.e1074cp+4", 30), ("0x1.bebd04p+0", "-0x1.002984p+8", 170), ("0x1.f81788p-1", "-0x1.19aaaap+4", 58))


def _affines(name, N, B, identity0=True):
    rng = _rng(name)
    aff = np.stack([rng.uniform(0.5, 2.0, size=(N, B)), rng.uniform(-60, 60, size=(N, B))], -1).astype(F)
    if identity0:
        aff[0] = (1.0, 0.0)
    return aff


REDUCE_SIZES = (3, 15, 16, 17, 48, 51, 771)
REDUCE_MODES = ("median", "mean")


def reduce_cases(big=True):
    """-> (name, mode, members [N, B, n] uint8, affine [N, B, 2] fp32): every N at 771 bytes (B = 2), every size of REDUCE_SIZES at
    B = 1..3, all 256 byte values under affines that reach both clamps and under the FMA-telling triples, and - `big` - one size
    past one sweep of the capped grid on the wide and on the ragged path."""
    for N in range(1, 17):
        for mode in REDUCE_MODES:
            rng = _rng(f"r.members.{N}.{mode}")
            yield f"members.n{N}.{mode}", mode, rng.integers(0, 256, size=(N, 2, 771), dtype=np.uint8), \
                _affines(f"ra.{N}.{mode}", N, 2, identity0=N % 2 == 0)
    for i, n in enumerate(REDUCE_SIZES):
        for B in (1, 2, 3):
            for mode in REDUCE_MODES:
                N = 1 + (3 * i + B) % 6
                rng = _rng(f"r.size.{n}.{B}.{mode}")
                yield f"size.{n}.b{B}.{mode}", mode, rng.integers(0, 256, size=(N, B, n), dtype=np.uint8), \
                    _affines(f"ra.size.{n}.{B}.{mode}", N, B, identity0=False)
    ramp = np.tile(np.arange(256, dtype=np.uint8), 3)                              # 768 bytes: whole pixels
    for mode in REDUCE_MODES:
        mem = np.stack([ramp, ramp, ramp[::-1]]).reshape(3, 1, 768).repeat(2, axis=1)
        aff = np.array([[(2.0, -200.0), (1.0, 0.0)], [(2.0, 60.0), (0.5, -20.0)], [(1.5, 100.0), (0.75, -60.0)]], dtype=F)
        yield f"clamps.{mode}", mode, np.ascontiguousarray(mem), aff
    for t, (gh, oh, x) in enumerate(FMA_TRIPLES):
        g, o = F(float.fromhex(gh)), F(float.fromhex(oh))
        mem = np.stack([ramp, ramp]).reshape(2, 1, 768).copy()
        mem[:, 0, :3] = x
        yield f"fma.{t}", "median", mem, np.array([[(g, o)], [(g, o)]], dtype=F)
    if big:
        yield from reduce_big_cases()


def reduce_big_cases():
    more = 48 * 37 + 9
    n = SWEEP_LANES * 16 + more
    yield "sweep.median", "median", _rng("r.sweep").integers(0, 256, size=(3, 1, n + (-n) % 3), dtype=np.uint8), _affines("ra.sweep", 3, 1)
    n = SWEEP_LANES + more
    yield "sweep.mean.ragged", "mean", _rng("r.sweep.r").integers(0, 256, size=(2, 1, n + (-n) % 3), dtype=np.uint8), \
        _affines("ra.sweep.r", 2, 1)


REDUCE_WRONG = {
    "fused": "fma.0",
    "truncated": "members.n3.median",
    "no_clamp": "clamps.median",
    "affine_after_the_reduce": "members.n5.median",
    "clip0_affine": "size.771.b2.mean",
    "member0_affine": "members.n4.mean",
    "spread_around_the_unaligned": "members.n5.mean",
    "straddling_group_first_clip": "size.51.b3.median",
}


# ----------------------------------------------------------------------------------------------- robustness
def aligned_scene(gains, offsets, h=96, w=128, salt=0.2, noise=6.0):
    """One picture with structure (a shaded ramp and a disc), N members = g_k * truth + o_k + Gaussian noise with `salt` of the
    bytes replaced by a random byte, as in ensemblebench --parity -> (what member 0 shows without noise, float [n]; members
    [N, 1, n] uint8)."""
    rng = _rng("aligned.scene")
    y, x = np.mgrid[0:h, 0:w]
    truth = 40 + 120 * (x / w) * (0.5 + 0.5 * np.sin(y / 9.0)) + 40 * ((x - 60) ** 2 + (y - 40) ** 2 < 400)
    truth = np.repeat(truth[..., None], 3, -1).reshape(-1)
    mem = []
    for g, o in zip(gains, offsets):
        m = g * truth + o + rng.normal(0, noise, truth.shape)
        s = rng.random(truth.shape) < salt
        m = np.where(s, rng.integers(0, 256, truth.shape), m)
        mem.append(np.rint(np.clip(m, 0, 255)).astype(np.uint8))
    return np.clip(gains[0] * truth + offsets[0], 0, 255), np.stack(mem)[:, None, :]


SCENE_GAINS, SCENE_OFFSETS = (1.0, 0.7, 1.3, 0.85, 1.15), (0.0, 30.0, -20.0, 10.0, -5.0)


def robustness_figures(gains=SCENE_GAINS, offsets=SCENE_OFFSETS):
    """-> dict: the mean byte error against member 0's space of today's median, of the members aligned by moment matching alone and
    of the members aligned by the cross rule, with the gains each rule found."""
    ref, mem = aligned_scene(gains, offsets)
    err = lambda r: float(np.abs(r.astype(np.float64) - ref).mean())
    out = {"unaligned": err(R.reduce_ref([m[0] for m in mem], "median")[0])}
    for key, wrong in (("moment", "moment_matching_only"), ("cross", None)):
        aff, _ = align_ref(mem, wrong)
        out[key] = err(reduce_affine_ref(mem, aff, "median")[0])
        out[key + "_gains"] = [float(a) for a in aff[:, 0, 0]]
    out["true_gains"] = [gains[0] / g for g in gains]
    return out


def compose_ref(members, flags, reduce, spread=False):
    """The aligned ensemble composed by hand: members[k][i] = member k's uint8 array [B, ...] of result i, flags[i] = that
    result's normalize_normal flag -> per result (the reduce, its spread or None, the affines [N, B, 2] or None for a normal)."""
    out = []
    for i, flag in enumerate(flags):
        arrs = [np.ascontiguousarray(m[i]) for m in members]
        B = arrs[0].shape[0]
        if flag:
            r, sp = R.reduce_ref([a.reshape(-1) for a in arrs], "normal", spread)
            aff = None
        else:
            mem = np.stack([a.reshape(B, -1) for a in arrs])
            aff, _ = align_ref(mem)
            r, sp = reduce_affine_ref(mem, aff, reduce, spread)
        out.append((r.reshape(arrs[0].shape), None if sp is None else sp.reshape(arrs[0].shape), aff))
    return out
