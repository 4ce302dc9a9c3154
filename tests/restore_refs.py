"""Shared references of the restore tests (fit.plan_restore / restore_frames, drn_restore_frames_u8): the float64 evaluation (the
plan's fp32 tap tables written out here a second time as dense matrices, applied in float64, no rounding), the fp32 torch
specification's own error against it before its rounding (E_ref, the unit of the bound), the bound, the case grid and the wrong
stand-ins the bound has to catch.  Everything here runs on the CPU; every case is computed once and shared."""
import importlib

import torch
import torch.nn.functional as F

# model-side (H', W') -> source-side (H, W), what it exercises
GEOMETRIES = [
    ((16, 32), (27, 40)),       # up both axes, 120-byte rows
    ((32, 32), (37, 23)),       # up in y, down in x, 69-byte rows
    ((16, 16), (45, 61)),       # 183-byte rows: every row at another alignment
    ((64, 64), (24, 40)),       # shrinking, Ky 6 / Kx 4
    ((32, 32), (8, 9)),         # 8 taps per axis, 27-byte rows
    ((16, 32), (16, 45)),       # one axis at scale 1
    ((64, 128), (135, 240)),    # several tiles on both axes
]
# all weights dyadic, every fp32 operation exact, ties real: bit for bit.  (The x2 shrink is dyadic away from the picture's
# border only: its first and last row and column have three taps of 3/7, 3/7, 1/7; see dyadic_mask)
DYADIC = [
    ((16, 32), (32, 64)),       # x2 up
    ((32, 64), (16, 32)),       # x2 down
    ((16, 16), (64, 64)),       # x4 up
    ((16, 32), (16, 32)),       # identity: the kernel launched directly is a copy
]
# beyond the issue's grid, for the kernel: the sizes at which drn_restore_frames_u8 takes another turn
EXTRA = [
    ((64, 256), (24, 64)),      # a tile's source rows overflow the raw buffer: it is refilled several times per chunk
    ((16, 16), (1, 1)),         # one output pixel: 3 bytes, all of them head or tail; 16 taps per axis
    ((16, 32), (3, 5)),         # 15-byte rows
    ((32, 32), (33, 129)),      # a last tile of one column: 387-byte rows
]
BATCHES = (1, 2)
TIMES = ((1, 1), (3, 3), (3, 2))        # (Ts, Td): frames in the model-size clip, frames returned
M_BOUND = 4                             # the margin drn_env_project and drn_fit_frames got over the same kind of yardstick
FLAT = ((16, 32), (27, 40))             # the flat-frames clip: 256 frames, frame v filled with v


def geometry_id(g):
    (hm, wm), (h, w) = g
    return f"{hm}x{wm}_to_{h}x{w}"


def fit_module(pkg):
    return importlib.import_module(pkg.__name__ + ".fit")


def restore_plan(pkg, g, T):
    """The way back of a stretch of T frames of the geometry's source size to its model size."""
    fit = fit_module(pkg)
    (hm, wm), (h, w) = g
    return fit.plan_restore(fit.plan_fit(T, h, w, "stretch", hm, wm))


# ----------------------------------------------------------------------------------------------- float64 reference
def dense(lo_n, w, n_in):
    """A (lo, n) + zero-padded weight table as a dense float64 [n_out, n_in] matrix, one tap at a time."""
    m = torch.zeros(lo_n.shape[0], n_in, dtype=torch.float64)
    for r, (lo, n) in enumerate(lo_n.tolist()):
        for k in range(n):
            m[r, lo + k] = float(w[r, k])
    return m


def apply64(src, my, mx, T):
    """uint8 [B,Ts,H',W',3] -> float64 [B,T,H,W,3] on the 0..255 scale, frames 0 .. T - 1."""
    return torch.einsum("yh,bthwc,xw->btyxc", my, src[:, :T].double(), mx)


def reference64(src, rplan):
    return apply64(src, dense(rplan.y_lo_n, rplan.y_w, rplan.H_model), dense(rplan.x_lo_n, rplan.x_w, rplan.W_model), rplan.T)


def round_u8(x):
    """Round half to even, clamp, uint8: what the specification and the kernel end with."""
    return x.round().clamp(0, 255).to(torch.uint8)


def bound_excess(got, ref64, e_ref):
    """(every element within 0.5 + M_BOUND * E_ref of ref64, the measured ratio max((|got - ref64| - 0.5)+ / E_ref)).  Another
    shape misses."""
    if tuple(got.shape) != tuple(ref64.shape):
        return False, float("inf")
    over = ((got.double() - ref64).abs() - 0.5).clamp_min(0.0)
    worst = float(over.max())
    ok = bool((over <= M_BOUND * e_ref).all())
    return ok, (worst / e_ref if e_ref > 0 else (0.0 if worst == 0 else float("inf")))


def dyadic_mask(rplan):
    """[H, W] bool: the outputs all of whose taps, on both axes, have dyadic weights (k / 1024 exactly)."""
    def axis(w):
        return ((w.double() * 1024).round() == w.double() * 1024).all(dim=1)
    return axis(rplan.y_w)[:, None] & axis(rplan.x_w)[None, :]


# ----------------------------------------------------------------------------------------------- cases
def source(B, T, H, W, seed=0):
    g = torch.Generator().manual_seed(20241020 + seed)
    x = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.int32).to(torch.uint8)
    x[0, 0, 0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)          # the ends of the range
    return x


_CASES = {}


def case(pkg, g, B, Ts, Td):
    """One case, computed once: source, plan, the float64 reference, the fp32 specification before and after its rounding,
    E_ref."""
    key = (g, B, Ts, Td)
    if key not in _CASES:
        fit = fit_module(pkg)
        rplan = restore_plan(pkg, g, Td)
        src = source(B, Ts, *g[0], seed=sum(g[1]))
        ref64 = reference64(src, rplan)
        spec32 = fit._restore_torch(src, rplan, rounded=False)
        _CASES[key] = dict(src=src, rplan=rplan, ref64=ref64, spec32=spec32, spec=round_u8(spec32),
                           e_ref=float((spec32.double() - ref64).abs().max()), name=f"{geometry_id(g)}_B{B}_T{Ts}to{Td}")
    return _CASES[key]


def grid(geometries=None):
    for g in (GEOMETRIES if geometries is None else geometries):
        for B in BATCHES:
            for Ts, Td in TIMES:
                yield g, B, Ts, Td


def flat_clip():
    """[1, 256, 16, 32, 3]: frame v filled with value v."""
    (hm, wm), _ = FLAT
    return torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1, 1).expand(1, 256, hm, wm, 3).contiguous()


# ----------------------------------------------------------------------------------------------- wrong stand-ins
def _shift_lo(m):
    """Every row's taps one source sample later (the last column's weight falls off the end)."""
    out = torch.zeros_like(m)
    out[:, 1:] = m[:, :-1]
    return out


def _unnormalised(n_in, n_out):
    """The triangle's raw weights over torch's support, not divided by their sum."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for r in range(n_out):
        c = scale * (r + 0.5)
        for j in range(max(0, int(c - support + 0.5)), min(int(c + support + 0.5), n_in)):
            m[r, j] = max(0.0, 1.0 - abs((j - c + 0.5) / support))
    return m


def _square(m, rows, cols):
    """A table applied to the other axis: cut or zero-padded to that axis's shape."""
    out = torch.zeros(rows, cols, dtype=m.dtype)
    r, c = min(rows, m.shape[0]), min(cols, m.shape[1])
    out[:r, :c] = m[:r, :c]
    return out


def _resize(c, **kw):
    p = c["rplan"]
    x = c["src"][:, :p.T].double()
    B = x.shape[0]
    x = x.permute(0, 1, 4, 2, 3).reshape(B * p.T, 3, p.H_model, p.W_model)
    x = F.interpolate(x, size=(p.H, p.W), mode="bilinear", **kw)
    return x.reshape(B, p.T, 3, p.H, p.W).permute(0, 1, 3, 4, 2)


def wrong_stand_ins():
    """name -> f(case) -> uint8 [B,T,H,W,3] a wrong kernel would give; each must miss the bound at some grid case."""
    def tables(c):
        p = c["rplan"]
        return dense(p.y_lo_n, p.y_w, p.H_model), dense(p.x_lo_n, p.x_w, p.W_model)

    def truncated(c):
        return c["spec32"].floor().clamp(0, 255).to(torch.uint8)

    def bilinear(c):
        return round_u8(_resize(c, antialias=False, align_corners=False))

    def corners(c):
        return round_u8(_resize(c, antialias=True, align_corners=True))

    def lo_off_by_one(c):
        my, mx = tables(c)
        return round_u8(apply64(c["src"], my, _shift_lo(mx), c["rplan"].T))

    def swapped(c):
        my, mx = tables(c)
        return round_u8(apply64(c["src"], _square(mx, *my.shape), _square(my, *mx.shape), c["rplan"].T))

    def unnormalised(c):
        p = c["rplan"]
        return round_u8(apply64(c["src"], _unnormalised(p.H_model, p.H), _unnormalised(p.W_model, p.W), p.T))

    def reversed_channels(c):
        return round_u8(c["ref64"].flip(-1))

    def next_frame(c):
        Ts = c["src"].shape[1]
        idx = (torch.arange(c["rplan"].T) + 1).clamp_max(Ts - 1)
        my, mx = tables(c)
        return round_u8(apply64(c["src"].index_select(1, idx), my, mx, c["rplan"].T))

    def time_not_cut(c):
        my, mx = tables(c)
        return round_u8(apply64(c["src"], my, mx, c["src"].shape[1]))

    def padded_pitch(c):
        good = round_u8(c["ref64"])
        B, T, H, W, _ = good.shape
        pitch = (W * 3 + 3) // 4 * 4
        rows = torch.zeros(B * T * H, pitch, dtype=torch.uint8)
        rows[:, :W * 3] = good.reshape(B * T * H, W * 3)
        return rows.reshape(-1)[:good.numel()].reshape(good.shape)

    return {"truncation in place of rounding": truncated, "no antialias when shrinking": bilinear,
            "corner-aligned centres": corners, "lo off by one": lo_off_by_one, "x and y tables swapped": swapped,
            "unnormalised weights": unnormalised, "channels reversed": reversed_channels, "frame t + 1 instead of t": next_frame,
            "time not cut": time_not_cut, "output row pitch rounded up to 4 bytes": padded_pitch}


def round_half_up(c):
    return (c["spec32"] + 0.5).floor().clamp(0, 255).to(torch.uint8)
