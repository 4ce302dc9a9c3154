"""Tiles joined in latent space: the references of drn_latent_tile_gather / drn_latent_tile_step_join (tiles.latent_gather /
latent_step_join) written out in numpy on raw bf16 bits, independently of tiles.py; the case grid of
tests/test_latent_tiles_gpu.py; and the wrong stand-ins that tests/test_latent_tiles_cpu.py shows the grid to separate.

bf16 tensors are uint16 arrays of their bits; all arithmetic is numpy float32, one rounding per operation."""
import zlib

import numpy as np

# what a wrong step-join kernel could do instead; step_join_ref(..., variant=name)
VARIANTS = ("one_buffer", "blend_first", "blend_at_one", "swap_xy", "ramp_at_row0", "writes_in_front", "lost_at",
            "cfg_unrounded", "w_j_over_O")
# a blend that is not the contract but rounds like it: a + wgt * (b - a) with the product unrounded.  Dyadic ramps (overlaps 1 and
# 3) and the product weights of two-axis ramps do not show it; single-axis ramps of 5 and 8 do, on both value grids below
NEAR_VARIANTS = ("fma",)
GATHER_VARIANTS = ("lost_at", "c_in_rounded", "one_copy")

PLANES = (1, 6)
CANVASES = ((7, 5), (6, 8), (9, 19))            # odd and even row pitch
TILES = ((3, 3), (4, 5), (5, 4), (6, 8))        # and one tile as large as the canvas, per canvas
RAMP_AT = (0, 1, 2)
OVERLAPS = ((0, 0), (1, 1), (5, 0), (0, 5), (2, 5), (8, 8))
GRIDS = ((5, "x"), (8, "y"))                    # value grids: single-axis ramps; latent 8 = the default tile_overlap 64
SIGMA_DATA = 0.5
SIGMAS = (80.0, 1.3125, 0.02)
GUIDANCE = 1.5


def f32(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def bf16_bits(x):
    """float32 -> bf16 bits, round to nearest even (finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def rbf(x):
    return f32(bf16_bits(x))


def scalars(sigma, sigma_next):
    """(c_in, c_skip, c_out, sigma, dt) as the scheduler computes them: fp32, one rounding per operation."""
    s, sd = np.float32(sigma), np.float32(SIGMA_DATA)
    den = s * s + sd * sd
    c_in = np.float32(1.0) / np.sqrt(den)
    c_skip = (sd * sd) / den
    c_out = (s * sd) / np.sqrt(den)
    return tuple(float(np.float32(v)) for v in (c_in, c_skip, c_out, s, np.float32(sigma_next) - s))


def ramp_table(O, variant=None):
    """fp32 [O]: float32((j + 1) / (O + 1))."""
    if variant == "w_j_over_O":
        return np.array([j / O for j in range(O)], dtype=np.float32)
    return np.array([(j + 1) / (O + 1) for j in range(O)], dtype=np.float32)


def _axis(idx, table):
    f = np.ones(len(idx), dtype=np.float32)
    for k, i in enumerate(idx):
        if 0 <= i < len(table):
            f[k] = table[i]
    return f


def gather_ref(canvas, h, w, y_at, x_at, c_in, copies, variant=None):
    """canvas bits [planes, Hc, Wc] -> bits [copies, planes, h, w]: bf16(fp32(crop) * c_in), `copies` times."""
    if variant == "lost_at":
        y_at = x_at = 0
    c = np.float32(c_in)
    if variant == "c_in_rounded":               # c_in taken in the tensor's own format
        c = rbf(np.array([c_in], dtype=np.float32))[0]
    one = bf16_bits(f32(canvas[:, y_at:y_at + h, x_at:x_at + w]) * c)
    if variant == "one_copy" and copies == 2:   # the second copy never written
        return np.stack([one, np.zeros_like(one)])
    return np.stack([one] * copies)


def step_join_ref(mo, un, g, cur, nxt, geo, scal, variant=None):
    """mo (and un, or None) bits [planes, h, w], cur / nxt bits [planes, Hc, Wc], geo = (y_at, x_at, ry, rx, Oy, Ox),
    scal = (c_skip, c_out, sigma, dt) -> nxt after the join (a new array).
      m = un is None ? c : bf16(c + bf16(g * bf16(c - u)));  b = bf16(sm + ((sm - (c_skip * sm + c_out * m)) / sigma) * dt), sm from cur
      wgt = wy * wx in fp32;  nxt <- b where wgt == 1, else bf16(a + wgt * (b - a)) as three fp32 operations."""
    y_at, x_at, ry, rx, Oy, Ox = geo
    c_skip, c_out, sigma, dt = (np.float32(v) for v in scal)
    g = np.float32(g)
    h, w = mo.shape[1:]
    out = nxt.copy()
    wy, wx = ramp_table(Oy, variant), ramp_table(Ox, variant)
    if variant == "lost_at":
        y_at = x_at = 0
    y_lo, x_lo = (0, 0) if variant == "writes_in_front" else (ry, rx)
    ys, xs = np.arange(y_lo, h), np.arange(x_lo, w)
    iy, ix = (ys, xs) if variant == "ramp_at_row0" else (ys - ry, xs - rx)
    if variant == "swap_xy":
        fy, fx = _axis(iy, wx), _axis(ix, wy)
    else:
        fy, fx = _axis(iy, wy), _axis(ix, wx)
    wgt = (fy[:, None] * fx[None, :])[None]
    assert wgt.dtype == np.float32
    at = (slice(None), slice(y_at + y_lo, y_at + h), slice(x_at + x_lo, x_at + w))
    c = f32(mo[:, y_lo:, x_lo:])
    if un is None:
        m = c
    else:
        u = f32(un[:, y_lo:, x_lo:])
        m = rbf(c + g * (c - u)) if variant == "cfg_unrounded" else rbf(c + rbf(g * rbf(c - u)))
    a = f32(out[at])
    sm = a if variant == "one_buffer" else f32(cur[at])
    if variant == "blend_first":                # the sample cross-faded, then stepped, instead of the step's result cross-faded
        sm = np.where(wgt == 1.0, sm, rbf(a + wgt * (sm - a)))
    denoised = c_skip * sm + c_out * m
    deriv = (sm - denoised) / sigma
    b = rbf(sm + deriv * dt)
    assert b.dtype == np.float32
    if variant == "blend_first":
        out[at] = bf16_bits(b)
        return out
    d = b - a
    if variant == "fma":
        v = (a.astype(np.float64) + wgt.astype(np.float64) * d.astype(np.float64)).astype(np.float32)
    else:
        mm = wgt * d
        v = a + mm
    assert v.dtype == np.float32
    res = rbf(v) if variant == "blend_at_one" else np.where(wgt == 1.0, b, rbf(v))
    out[at] = bf16_bits(res)
    return out


def case_bits(name, shape, scale):
    """Deterministic bf16 bits of a case: normal values of the given scale."""
    seed = zlib.crc32(name.encode())
    return bf16_bits((np.random.RandomState(seed).standard_normal(size=shape) * scale).astype(np.float32))


def geometry_cases(canvas):
    """(planes, cfg, h, w, geo, sigma index) of the geometry grid at one canvas size.  Tile sizes, ramp pairs and written origins
    are crossed; planes, CFG and the step's sigma alternate with the case's number, and the tile's corner walks through every
    position with it."""
    Hc, Wc = canvas
    cases = []
    k = 0
    for (h, w) in TILES + (canvas,):
        if h > Hc or w > Wc:
            continue
        for (Oy, Ox) in OVERLAPS:
            for ry in RAMP_AT:
                for rx in RAMP_AT:
                    if not (ry < h and rx < w and ry + Oy <= h and rx + Ox <= w):
                        continue
                    k += 1
                    geo = (k % (Hc - h + 1), (k // 2) % (Wc - w + 1), ry, rx, Oy, Ox)
                    cases.append((PLANES[k % 2], bool((k // 2) % 2), h, w, geo, k % 3))
    return cases


def case_inputs(canvas, i, case):
    """-> mo, un (or None), cur, nxt bits and (c_in, c_skip, c_out, sigma, dt).  The canvases hold noise of the step's sigma."""
    planes, cfg, h, w, geo, si = case
    Hc, Wc = canvas
    tag = f"{Hc}x{Wc}.{i}"
    sigma = SIGMAS[si]
    scal = scalars(sigma, SIGMAS[si + 1] if si + 1 < len(SIGMAS) else 0.0)
    spread = float(np.sqrt(sigma * sigma + 1.0))
    mo = case_bits("m" + tag, (planes, h, w), 1.0)
    un = case_bits("u" + tag, (planes, h, w), 1.0) if cfg else None
    return mo, un, case_bits("c" + tag, (planes, Hc, Wc), spread), case_bits("n" + tag, (planes, Hc, Wc), spread), scal


def grid_values():
    """Every finite bf16 in [-4, 4]: 33 026 values."""
    pos = np.arange(0, 0x4080 + 1, dtype=np.uint32)            # +0 .. 4.0
    return np.concatenate([pos, pos | 0x8000]).astype(np.uint16)


GRID_ROLLS = (1, 129, 16385, 16514, 16641, 17000)     # (16 513 values per sign: the last four pair x with about -x, -2x, -x/2)
PAIR_ROWS = {"bf16": 12, "random": 16}      # lines per plane: 198 156 = 12 * 16 513, 2^20 = 16 * 65 536


def grid_pairs(kind):
    """(a, b) bits: what the next canvas holds against the step's result.  'bf16': every finite bf16 in [-4, 4] against six rolled
    copies of itself (198 156 pairs); 'random': 2^20 random pairs at scale 80."""
    if kind == "bf16":
        v = grid_values()
        return np.concatenate([np.roll(v, r) for r in GRID_ROLLS]), np.tile(v, len(GRID_ROLLS))
    return case_bits("grid.a", (1 << 20,), 80.0), case_bits("grid.b", (1 << 20,), 80.0)


GRID_SCALARS = (0.25, 1.0, 1.0, -1.0)           # with a current canvas of zeros the step's result IS the model's output


def value_grid(kind, O, axis):
    """The pairs of grid_pairs under every weight of a single-axis ramp of O -> mo, cur, nxt bits, geo and the step's scalars.
    Pair p sits at plane p // R, line p % R (R = PAIR_ROWS: a row for an x ramp, a column for a y ramp) in every sample of the
    line: nxt holds a, the model's output b; the line's last sample lies behind the ramp (weight 1)."""
    a, b = grid_pairs(kind)
    R = PAIR_ROWS[kind]
    assert a.size % R == 0
    a, b = a.reshape(-1, R, 1), b.reshape(-1, R, 1)
    planes = a.shape[0]
    if axis == "x":
        mo = np.broadcast_to(b, (planes, R, O + 1)).copy()
        nxt = np.zeros((planes, R + 2, O + 4), dtype=np.uint16)
        nxt[:, 1:R + 1] = a
        nxt[:, 0], nxt[:, R + 1] = nxt[:, 1], nxt[:, R]
        geo = (1, 2, 0, 0, 0, O)
    else:
        mo = np.broadcast_to(b.reshape(planes, 1, R), (planes, O + 1, R)).copy()
        nxt = np.zeros((planes, O + 3, R + 3), dtype=np.uint16)
        nxt[:, :, 2:R + 2] = a.reshape(planes, 1, R)
        nxt[:, :, :2], nxt[:, :, R + 2] = nxt[:, :, 2:3], nxt[:, :, R + 1]
        geo = (1, 2, 0, 0, O, 0)
    return mo, np.zeros_like(nxt), nxt, geo, GRID_SCALARS


BIG = dict(planes=2, canvas=(45, 310), tile=(40, 300), geo=(3, 7, 3, 5, 18, 17))     # more than one workgroup per axis
