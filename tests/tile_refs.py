"""Spatial tiles: the blend reference of drn_tile_blend_u8 / tiles.blend_tile written out in numpy, independently of tiles.py,
the case grid of tests/test_tiles_gpu.py, and the wrong stand-ins that tests/test_tiles_cpu.py shows the grid to separate."""
import numpy as np

# what a wrong kernel could do instead; blend_ref(..., variant=name)
VARIANTS = ("half_up", "trunc", "w_j_over_O", "min_w", "sum_w", "ramp_at_row0", "swap_xy", "lost_at", "writes_in_front",
            "reversed_channels", "frame_off_by_one")
# blends that are not the contract but round like it: "fma" is a + wgt * (b - a) with the product unrounded, "lerp2" is
# a * (1 - wgt) + b * wgt.  The byte-pair grid separates both at the overlap pair (5, 3) and neither at (1, 1) and (3, 3), where
# every weight is dyadic
NEAR_VARIANTS = ("fma", "lerp2")

OVERLAPS = ((0, 0), (1, 1), (3, 0), (0, 3), (2, 5), (5, 3))
GRID_OVERLAPS = ((1, 1), (3, 3), (5, 3))
FRAMES = ((1, 1), (2, 3))
WIDTHS = (4, 5, 6, 19)              # row pitches of 12, 15, 18 and 57 bytes: every pitch residue mod 4
HEIGHTS = (7, 21)
TILES = ((3, 3), (5, 4), (8, 7), (12, 11))
RAMP_AT = (0, 1, 4)
GRID_FRAMES = 21846                 # 3 channels x 21846 frames >= 65536 byte pairs


def ramp_table(O, variant=None):
    """fp32 [O]: float32((j + 1) / (O + 1))."""
    if variant == "w_j_over_O":
        return np.array([j / O for j in range(O)], dtype=np.float32)
    return np.array([(j + 1) / (O + 1) for j in range(O)], dtype=np.float32)


def _axis(idx, table):
    """The factor of every sample of one axis: the ramp's weight inside it, exactly 1.0 in front of it (only a wrong kernel
    asks) and behind it."""
    f = np.ones(len(idx), dtype=np.float32)
    for k, i in enumerate(idx):
        if 0 <= i < len(table):
            f[k] = table[i]
    return f


def blend_ref(canvas, tile, geo, variant=None):
    """canvas uint8 [F, H, W, 3], tile uint8 [F, h, w, 3], geo = (y_at, x_at, ry, rx, Oy, Ox) -> the canvas after the blend (a new
    array).  wgt = wy * wx in fp32; where wgt == 1 the tile's byte; else a + wgt * (b - a) as three fp32 operations, rounded half
    to even, clamped."""
    y_at, x_at, ry, rx, Oy, Ox = geo
    assert canvas.dtype == np.uint8 and tile.dtype == np.uint8 and canvas.ndim == 4 and tile.ndim == 4
    h, w = tile.shape[1:3]
    out = canvas.copy()
    wy, wx = ramp_table(Oy, variant), ramp_table(Ox, variant)
    if variant == "lost_at":
        y_at = x_at = 0
    y_lo, x_lo = (0, 0) if variant == "writes_in_front" else (ry, rx)
    ys, xs = np.arange(y_lo, h), np.arange(x_lo, w)
    iy, ix = (ys, xs) if variant == "ramp_at_row0" else (ys - ry, xs - rx)
    if variant == "swap_xy":            # the row table read by column and the column table by row
        fy, fx = _axis(iy, wx), _axis(ix, wy)
    else:
        fy, fx = _axis(iy, wy), _axis(ix, wx)
    if variant == "min_w":
        wgt = np.minimum(fy[:, None], fx[None, :])
    elif variant == "sum_w":
        wgt = (fy[:, None] + fx[None, :]) - np.float32(1.0)
    else:
        wgt = fy[:, None] * fx[None, :]
    assert wgt.dtype == np.float32
    wgt = wgt[None, :, :, None]
    src = tile[:, y_lo:, x_lo:]
    if variant == "reversed_channels":
        src = src[..., ::-1]
    if variant == "frame_off_by_one":
        src = np.roll(src, 1, axis=0)
    a = out[:, y_at + y_lo:y_at + h, x_at + x_lo:x_at + w].astype(np.float32)
    b = src.astype(np.float32)
    if variant == "fma":
        v = (a.astype(np.float64) + wgt.astype(np.float64) * (b.astype(np.float64) - a)).astype(np.float32)   # exact, rounded once
    elif variant == "lerp2":
        v = a * (np.float32(1.0) - wgt) + b * wgt
    else:
        d = b - a
        m = wgt * d
        v = a + m
    assert v.dtype == np.float32
    if variant == "half_up":
        r = np.floor(v + np.float32(0.5))
    elif variant == "trunc":
        r = np.floor(v)
    else:
        r = np.rint(v)
    res = np.where(wgt == 1.0, b, np.clip(r, 0.0, 255.0)).astype(np.uint8)
    out[:, y_at + y_lo:y_at + h, x_at + x_lo:x_at + w] = res
    return out


def case_bytes(name, shape):
    """Deterministic bytes of a case: every value 0..255 turns up, neighbours unrelated."""
    seed = int.from_bytes(name.encode(), "little") % (2 ** 31)
    return np.random.RandomState(seed).randint(0, 256, size=shape, dtype=np.uint8)


def geometry_cases(W):
    """(frames, H, h, w, geo) of the geometry grid at one canvas width.  Tile sizes, ramp pairs and written origins are crossed;
    the tile's corner walks through every position with the case's number, so the row segments start at every byte residue."""
    cases = []
    k = 0
    for H in HEIGHTS:
        for (h, w) in TILES:
            if h > H or w > W:
                continue
            for (Oy, Ox) in OVERLAPS:
                for ry in RAMP_AT:
                    for rx in RAMP_AT:
                        if not (ry < h and rx < w and ry + Oy <= h and rx + Ox <= w):
                            continue
                        k += 1
                        frames = FRAMES[k % 2]
                        cases.append((frames, H, h, w, (k % (H - h + 1), (k // 2) % (W - w + 1), ry, rx, Oy, Ox)))
        # a written width of one pixel, with and without a one-column ramp; a tile that covers the canvas exactly
        h, w = (3, 3) if W < 19 else (5, 7)
        for Ox in (0, 1):
            k += 1
            cases.append((FRAMES[k % 2], H, h, w, (k % (H - h + 1), k % (W - w + 1), 1, w - 1, 1, Ox)))
        for (Oy, Ox) in ((0, 0), (1, 1), (3, 3)):
            cases.append((FRAMES[1], H, H, W, (0, 0, 0, 0, Oy, Ox)))
            cases.append((FRAMES[0], H, H, W, (0, 0, 2, 1, Oy, min(Ox, W - 1))))
    return cases


def case_inputs(W, i, case):
    (B, T), H, h, w, geo = case
    return case_bytes(f"c{W}.{i}", (B * T, H, W, 3)), case_bytes(f"t{W}.{i}", (B * T, h, w, 3))


def segment_residues(W, case, base=0):
    """The byte residues mod 4 at which the case's canvas row segments start."""
    _, H, h, w, (y_at, x_at, ry, rx, Oy, Ox) = case
    F = case[0][0] * case[0][1]
    return {(base + ((f * H + y_at + y) * W + x_at + rx) * 3) % 4 for f in range(F) for y in range(ry, h)}


def value_grid(Oy, Ox):
    """All 65 536 byte pairs under every weight of the overlap pair: canvas [F, Oy + 3, Ox + 4, 3], tile [F, Oy + 1, Ox + 1, 3] and
    the geometry.  Pair p = 3 f + c (mod 65 536) sits in channel c of frame f at every pixel: canvas byte p >> 8, tile byte
    p & 255.  The tile's last row and column lie behind the ramps."""
    p = (np.arange(GRID_FRAMES * 3, dtype=np.int64) % 65536).reshape(GRID_FRAMES, 1, 1, 3)
    canvas = np.broadcast_to((p >> 8).astype(np.uint8), (GRID_FRAMES, Oy + 3, Ox + 4, 3)).copy()
    tile = np.broadcast_to((p & 255).astype(np.uint8), (GRID_FRAMES, Oy + 1, Ox + 1, 3)).copy()
    return canvas, tile, (1, 2, 0, 0, Oy, Ox)
