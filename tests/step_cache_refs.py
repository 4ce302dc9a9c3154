"""References, the case grid and wrong stand-ins for the step cache (step_cache.py, csrc/step_cache.hip).  Shared by
tests/test_step_cache_cpu.py and tests/test_step_cache_gpu.py; nothing here runs on the GPU.  Everything works on raw bf16 bits
(uint16 arrays), so that no framework's rounding stands between a test and the rule.

The probe's order (include/drn.h): chunks of 8192 consecutive values of one clip; value j of a chunk belongs to lane (j / 8) % 256;
a lane adds its values in increasing j from 0.0; the wave's butterfly over lane ^ 32, 16, 8, 4, 2, 1; the four waves as
((w0 + w1) + w2) + w3; then per clip 64 contiguous runs of ceil(chunks / 64) partials, each from 0.0, and the runs in order."""
import math

import numpy as np

CHUNK = 8192
QNAN64 = 0x7FF8000000000000

# n: around the 16-byte group, around one chunk, several chunks with a ragged end; B x chunks past one sweep of the 2048 blocks
SIZES = (1, 7, 8, 9, 8191, 8192, 8193, 3 * 8192 + 5)
BATCHES = (1, 2, 3)
BIG = ((3, 701 * 8192 + 5), (2, 1030 * 8192))          # 2103 ragged chunks (2-byte loads), 2060 whole ones (16-byte loads)
# residual / apply: one sweep is 2048 x 256 lanes x 8 values = 4 Mi values on the vector path, 512 Ki on the other
EW_SIZES = SIZES + (2048 * 256 * 8 + 8 * 300 + 3, 2048 * 256 + 77)


def f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_bits(x):
    """fp32 -> bf16 bits, round to nearest even, every NaN -> 0x7FC0 (torch's .bfloat16())."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(np.asarray(x, dtype=np.float32)), np.uint16(0x7FC0), r)


def is_nan(bits):
    bits = np.asarray(bits, dtype=np.uint16)
    return ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)


def same_as_torch(bits, torch_bits):
    """The rule's bits against torch's own (a.float() -/+ b.float()).bfloat16(): identical wherever the result is no NaN, and a NaN
    where torch has one.  (Which NaN torch writes depends on the path its conversion takes: c10's scalar rule gives 0x7FC0, the
    rule here; the vectorised CPU loop writes 0xFFFF for the same value.)"""
    bits, torch_bits = np.asarray(bits, dtype=np.uint16), np.asarray(torch_bits, dtype=np.uint16)
    nan = is_nan(torch_bits)
    return bool(np.array_equal(is_nan(bits), nan) and np.array_equal(bits[~nan], torch_bits[~nan]) and (bits[nan] == 0x7FC0).all())


def all_finite_bf16():
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    return b[(b & 0x7F80) != 0x7F80]


def rand_bits(name, shape, scale=1.0):
    """Deterministic bf16 values ~ N(0, scale) from a name."""
    seed = int.from_bytes(name.encode(), "little") % (2 ** 32)
    return bf16_bits(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * np.float32(scale))


# ----------------------------------------------------------------------------------------------- the probe
def _chunk_partial(v):
    """One chunk's terms (<= 8192, fp64) -> its partial, lane by lane as the kernel's block adds them."""
    lanes = np.zeros(256, dtype=np.float64)
    for j0 in range(0, v.size, 8):                        # eight consecutive values go to lane (j0 / 8) % 256, in order
        lane = (j0 // 8) % 256
        for t in v[j0:j0 + 8]:
            lanes[lane] = lanes[lane] + t
    waves = []
    for w in range(4):
        s = lanes[64 * w:64 * w + 64].copy()
        for d in (32, 16, 8, 4, 2, 1):
            s = s + s[np.arange(64) ^ d]
        waves.append(s[0])
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def _chunk_partials_fast(v):
    """All chunks of one clip at once (the same order, vectorised over chunks) - for the sizes where the loop above is too slow;
    tests/test_step_cache_cpu.py holds the two against each other."""
    nc = -(-v.size // CHUNK)
    pad = np.zeros(nc * CHUNK, dtype=np.float64)
    pad[:v.size] = v
    q = pad.reshape(nc, 4, 256, 8)
    s = np.zeros((nc, 256), dtype=np.float64)
    for t in range(4):
        for e in range(8):
            s = s + q[:, t, :, e]
    s = s.reshape(nc, 4, 64)
    for d in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, np.arange(64) ^ d]
    return ((s[:, 0, 0] + s[:, 1, 0]) + s[:, 2, 0]) + s[:, 3, 0]


def _clip_sum(parts):
    nc = parts.size
    seg = -(-nc // 64)
    total = np.float64(0.0)
    for lane in range(64):
        run = np.float64(0.0)
        for p in parts[lane * seg:min((lane + 1) * seg, nc)]:
            run = run + p
        total = total + run
    return total


def ordered_sum(v, fast=None):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if fast if fast is not None else v.size > 4 * CHUNK:
            parts = _chunk_partials_fast(v)
        else:
            parts = np.array([_chunk_partial(v[k:k + CHUNK]) for k in range(0, v.size, CHUNK)], dtype=np.float64)
        return _clip_sum(parts)


def terms(xbits, rbits, variant=None):
    """Per value (|x - ref| with the fp32 subtraction, |ref|) as fp64.  variant: a wrong stand-in."""
    x, r = f32(xbits), f32(rbits)
    with np.errstate(invalid="ignore", over="ignore"):
        if variant == "fp64_subtract":
            num = np.abs(x.astype(np.float64) - r.astype(np.float64))
        elif variant == "signed":
            num = (x - r).astype(np.float32).astype(np.float64)
        else:
            num = np.abs((x - r).astype(np.float32)).astype(np.float64)
        den = np.abs(x if variant == "den_from_x" else r).astype(np.float64)
    return num, den


def probe_ref(xbits, rbits, variant=None, fast=None):
    """stats [B, 2] fp64 = (num_b, den_b) of x, ref [B, n] bf16 bits, in the documented order; a NaN sum is the one quiet NaN."""
    xbits, rbits = np.asarray(xbits, dtype=np.uint16), np.asarray(rbits, dtype=np.uint16)
    B, n = xbits.shape
    num, den = terms(xbits, rbits, variant)
    out = np.zeros((B, 2), dtype=np.float64)
    for b in range(B):
        if variant == "neighbour_chunk":
            # the ragged last chunk runs on into the next clip's values (the last clip's stops at the end of the tensor)
            flat_n, flat_d = num.reshape(-1), den.reshape(-1)
            hi = min(b * n + -(-n // CHUNK) * CHUNK, B * n)
            out[b] = ordered_sum(flat_n[b * n:hi], fast), ordered_sum(flat_d[b * n:hi], fast)
        else:
            out[b] = ordered_sum(num[b], fast), ordered_sum(den[b], fast)
    if variant == "whole_batch":
        out[:] = out.sum(0)
    bits = out.view(np.uint64)
    bits[np.isnan(out)] = QNAN64
    return out


def delta_ref(stats):
    worst = 0.0
    for num, den in np.asarray(stats, dtype=np.float64):
        d = math.inf
        if den != 0.0 and math.isfinite(num) and math.isfinite(den):
            d = float(num) / float(den)
            if not math.isfinite(d):
                d = math.inf
        worst = max(worst, d)
    return worst


def residual_ref(xbits, rbits):
    with np.errstate(invalid="ignore", over="ignore"):
        return bf16_bits((f32(xbits) - f32(rbits)).astype(np.float32))


def apply_ref(xbits, rbits):
    with np.errstate(invalid="ignore", over="ignore"):
        return bf16_bits((f32(xbits) + f32(rbits)).astype(np.float32))


def probe_cases():
    """(name, B, n, x element offset, ref element offset, stats offset in doubles): the geometry grid of the probe."""
    cases = [(f"n{n}_B{B}", B, n, 0, 0, 0) for n in SIZES for B in BATCHES]
    for off in range(1, 8):                               # every tensor off the 16-byte grid, alone and together
        cases += [(f"x+{off}", 2, 8192 + 16, off, 0, 0), (f"ref+{off}", 2, 8192 + 16, 0, off, 0),
                  (f"both+{off}", 3, 8193, off, off, off), (f"stats+{off}", 1, 24, 0, 0, off)]
    cases += [(f"big_B{B}_n{n}", B, n, 0, 0, 0) for B, n in BIG]
    return cases


# ----------------------------------------------------------------------------------------------- the rule, by hand
def hand_loop(inputs, thr, max_run, head, tail, final, variant=None):
    """The step cache over a three-stage net on bf16 bits, composed by hand -> (outputs, log).  head / tail / final: bits [B, n]
    -> bits.  variant: a wrong stand-in of the rule (None = the rule)."""
    n_steps = len(inputs)
    ref = R = prev_x1 = None
    run = 0
    outs, log = [], []
    for i, inp in enumerate(inputs):
        x1 = head(inp)
        forced = i == 0 or i == n_steps - 1 or run >= max_run
        delta = None
        if not forced:
            against = prev_x1 if variant == "prev_x1" else ref
            pv = variant if variant in ("den_from_x", "signed", "whole_batch", "fp64_subtract", "neighbour_chunk") else None
            delta = delta_ref(probe_ref(x1, against, pv))
        if not forced and delta < thr:
            x = apply_ref(x1, R)
            run += 1
            if variant == "refresh_ref":
                ref = x1
            if variant == "refresh_R":
                R = residual_ref(x, ref)
            log.append((False, delta))
        else:
            ref = x1
            x = tail(x1)
            R = residual_ref(x, inp if variant == "R_before_head" else ref)
            run = 0
            log.append((True, delta))
        prev_x1 = x1
        outs.append(final(x))
    return outs, log
