"""Shared references of the fit tests (fit.py, drn_fit_frames): the float64 evaluation (tap tables written out here a second time,
applied in float64, then 2v - 1, no bf16 rounding), the fp32 torch specification's own error against it (E_ref, the unit of the
bound), the bound, the case grid and the wrong stand-ins the bound has to catch.  Everything here runs on the CPU; every case is
computed once and shared."""
import functools
import importlib

import torch
import torch.nn.functional as F

# (Hs, Ws) -> mode, fit_height, fit_width, what it exercises
GEOMETRIES = [
    ((27, 40), "crop", 16, 16),         # 4 taps along x, x offset 4
    ((37, 23), "crop", 32, 32),         # up-sampling, 2 taps, y offset (9 by the plan's own rule: round(37 * 32 / 23) = 51 rows)
    ((45, 61), "crop", 16, 16),         # 6 taps along y
    ((135, 240), "stretch", 64, 128),   # the 1.875 ratio of 1080p -> 576 x 1024 over several tiles
    ((16, 32), "crop", 0, 0),           # identity
    ((18, 35), "crop", 0, 0),           # pure crop: rows 1..16, columns 1..32
    ((50, 20), "stretch", 16, 16),      # different tap counts per axis: Ky 8, Kx 4
]
GEOMETRY_IDS = ["27x40_crop16x16", "37x23_crop32x32", "45x61_crop16x16", "135x240_stretch64x128", "16x32_identity",
                "18x35_purecrop", "50x20_stretch16x16"]
BATCHES = (1, 2)
FRAMES = (1, 3, 9, 10)                  # -> 1, 9, 9, 17 output frames
SCALE1 = (4, 5)                         # the geometries at scale 1 on both axes: bit-exact against today's ingest
M_BOUND = 4                             # the margin drn_env_project got over the same kind of yardstick


def fit_module(pkg):
    return importlib.import_module(pkg.__name__ + ".fit")


# ----------------------------------------------------------------------------------------------- float64 reference
@functools.lru_cache(maxsize=None)
def ref_taps(n_in, n_full, off, n_out):
    """Dense float64 [n_out, n_in] matrix of torch's antialiased triangle filter, one output sample at a time."""
    scale = n_in / n_full
    support = max(scale, 1.0)
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for r in range(n_out):
        c = scale * (off + r + 0.5)
        lo, hi = max(0, int(c - support + 0.5)), min(int(c + support + 0.5), n_in)
        w = [max(0.0, 1.0 - abs((j - c + 0.5) / support)) for j in range(lo, hi)]
        tot = sum(w)
        for j, v in zip(range(lo, hi), w):
            m[r, j] = v / tot
    return m


def time_index(T, T_out):
    return torch.tensor([min(t, T - 1) for t in range(T_out)], dtype=torch.long)


def apply64(src, my, mx, t_idx):
    """[B,T,H,W,3] -> float64 [B,3,T',H',W'], still in [0, 1]."""
    x = src.double().index_select(1, t_idx)
    return torch.einsum("yh,bthwc,xw->bctyx", my, x, mx)


def reference64(src, plan):
    my = ref_taps(plan.H, plan.H_full, plan.y0, plan.H_out)
    mx = ref_taps(plan.W, plan.W_full, plan.x0, plan.W_out)
    return apply64(src, my, mx, time_index(plan.T, plan.T_out)) * 2.0 - 1.0


def ulp_bf16(x):
    """Spacing of bf16 (8 significant bits) at |x|, x float64; below the smallest normal: the subnormal spacing."""
    _, e = torch.frexp(x.abs())                       # |x| = m * 2^e, m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(e, -125), e)       # (frexp(0) has exponent 0)
    return torch.ldexp(torch.ones_like(x), e.clamp_min(-125) - 8)


def bound_excess(got, ref64, e_ref):
    """(every element within 0.5 ulp_bf16(ref64) + M_BOUND * E_ref, the measured ratio max((|got - ref64| - 0.5 ulp)+ / E_ref))."""
    over = ((got.double() - ref64).abs() - 0.5 * ulp_bf16(ref64)).clamp_min(0.0)
    worst = float(over.max())
    ok = bool((over <= M_BOUND * e_ref).all())
    return ok, (worst / e_ref if e_ref > 0 else (0.0 if worst == 0 else float("inf")))


def todays_ingest(frames):
    """The nodes' ingest as it is without fit, on frames already on the grid: [B,T,H,W,3] -> bf16 [B,3,T,H,W]."""
    return (frames.permute(0, 4, 1, 2, 3) * 2.0 - 1.0).to(torch.bfloat16)


# ----------------------------------------------------------------------------------------------- cases
def source(B, T, H, W, seed=0):
    g = torch.Generator().manual_seed(20241019 + seed)
    x = torch.rand(B, T, H, W, 3, generator=g)
    x[0, 0, 0, 0] = torch.tensor([0.0, 1.0, 0.5])      # the ends of the range and the zero of 2v - 1
    return x


_CASES = {}


def case(pkg, gi, B, T):
    """One grid case, computed once: source, plan, the float64 reference, the fp32 specification before its bf16 cast, E_ref."""
    key = (gi, B, T)
    if key not in _CASES:
        fit = fit_module(pkg)
        (H, W), mode, fh, fw = GEOMETRIES[gi]
        plan = fit.plan_fit(T, H, W, mode, fh, fw)
        src = source(B, T, H, W, seed=gi)
        ref64 = reference64(src, plan)
        spec32 = fit._fit_torch(src, plan, "cpu", round_bf16=False)
        _CASES[key] = dict(src=src, plan=plan, ref64=ref64, spec32=spec32, e_ref=float((spec32.double() - ref64).abs().max()),
                           name=f"{GEOMETRY_IDS[gi]}_B{B}_T{T}")
    return _CASES[key]


def grid(geometries=None):
    for gi in (range(len(GEOMETRIES)) if geometries is None else geometries):
        for B in BATCHES:
            for T in FRAMES:
                yield gi, B, T


def scattered_rows(Hs=120, Ws=40, Hd=16, Wd=32):
    """Tables no resize produces, for the kernels' chunk cutter: output rows read 2 source rows alternately near the top
    (0..7) and near the bottom (100..107) of the source, so no two consecutive output rows fit a 48-row stage together and a tile
    is cut into one chunk per row.  All weights are dyadic.  -> (a plan of the five tables, the dense float64 [Hd, Hs] and
    [Wd, Ws] matrices of the row and column tables)."""
    i = torch.arange(Hd)
    plan = type("P", (), {})()
    plan.T_out, plan.H_out, plan.W_out = 3, Hd, Wd
    plan.t_idx = torch.tensor([1, 0, 1], dtype=torch.int32)
    plan.y_lo_n = torch.stack([i // 2 + 100 * (i % 2), torch.full((Hd,), 2)], 1).to(torch.int32)
    plan.y_w = torch.tensor([[0.25, 0.75]], dtype=torch.float32).repeat(Hd, 1)
    plan.x_lo_n = torch.stack([torch.arange(Wd), torch.full((Wd,), 3)], 1).to(torch.int32)
    plan.x_w = torch.tensor([[0.5, 0.125, 0.375]], dtype=torch.float32).repeat(Wd, 1)
    assert int(plan.y_lo_n[:, 0].max()) + 2 <= Hs and Wd + 2 <= Ws
    assert all(abs(int(plan.y_lo_n[r + 1, 0]) - int(plan.y_lo_n[r, 0])) + 2 > 48 for r in range(Hd - 1))
    dense = []
    for lo_n, w, n_in in ((plan.y_lo_n, plan.y_w, Hs), (plan.x_lo_n, plan.x_w, Ws)):
        m = torch.zeros(lo_n.shape[0], n_in, dtype=torch.float64)
        for r, (lo, n) in enumerate(lo_n.tolist()):
            m[r, lo:lo + n] = w[r, :n].double()
        dense.append(m)
    return plan, dense[0], dense[1]


# ----------------------------------------------------------------------------------------------- wrong stand-ins
def _shift_lo(m):
    """Every row's taps one source sample later (the last column's weight falls off the end)."""
    out = torch.zeros_like(m)
    out[:, 1:] = m[:, :-1]
    return out


@functools.lru_cache(maxsize=None)
def _unnormalised(n_in, n_full, off, n_out):
    scale = n_in / n_full
    m = ref_taps(n_in, n_full, off, n_out)
    raw = torch.zeros_like(m)
    for r in range(n_out):
        c = scale * (off + r + 0.5)
        for j in range(n_in):
            raw[r, j] = max(0.0, 1.0 - abs((j - c + 0.5) / max(scale, 1.0)))
    return raw * (m != 0)


def _resize(src, plan, **kw):
    """F.interpolate in float64 to the resized size, then the crop: the plan's geometry with another filter."""
    x = src.double().index_select(1, time_index(plan.T, plan.T_out))
    B = x.shape[0]
    x = x.permute(0, 1, 4, 2, 3).reshape(B * plan.T_out, 3, plan.H, plan.W)
    x = F.interpolate(x, size=(plan.H_full, plan.W_full), mode="bilinear", **kw)
    x = x[:, :, plan.y0:plan.y0 + plan.H_out, plan.x0:plan.x0 + plan.W_out]
    return x.reshape(B, plan.T_out, 3, plan.H_out, plan.W_out).permute(0, 2, 1, 3, 4) * 2.0 - 1.0


def _square(m, rows, cols):
    """A table applied to the other axis: cut or zero-padded to that axis's shape."""
    out = torch.zeros(rows, cols, dtype=m.dtype)
    r, c = min(rows, m.shape[0]), min(cols, m.shape[1])
    out[:r, :c] = m[:r, :c]
    return out


def wrong_stand_ins():
    """name -> f(case) -> [B,3,T',H',W'] values a wrong kernel would give; each must miss the bound at some grid case."""
    def tables(c):
        p = c["plan"]
        return (ref_taps(p.H, p.H_full, p.y0, p.H_out), ref_taps(p.W, p.W_full, p.x0, p.W_out), time_index(p.T, p.T_out))

    def bilinear(c):
        return _resize(c["src"], c["plan"], antialias=False, align_corners=False)

    def corners(c):
        return _resize(c["src"], c["plan"], antialias=True, align_corners=True)

    def unnormalised(c):
        p = c["plan"]
        _, _, ti = tables(c)
        return apply64(c["src"], _unnormalised(p.H, p.H_full, p.y0, p.H_out), _unnormalised(p.W, p.W_full, p.x0, p.W_out),
                       ti) * 2.0 - 1.0

    def lo_off_by_one(c):
        my, mx, ti = tables(c)
        return apply64(c["src"], my, _shift_lo(mx), ti) * 2.0 - 1.0

    def swapped(c):
        my, mx, ti = tables(c)
        return apply64(c["src"], _square(mx, *my.shape), _square(my, *mx.shape), ti) * 2.0 - 1.0

    def no_offset(c):
        p = c["plan"]
        _, _, ti = tables(c)
        return apply64(c["src"], ref_taps(p.H, p.H_full, 0, p.H_out), ref_taps(p.W, p.W_full, 0, p.W_out), ti) * 2.0 - 1.0

    def wraps(c):
        p = c["plan"]
        my, mx, _ = tables(c)
        return apply64(c["src"], my, mx, torch.arange(p.T_out) % p.T) * 2.0 - 1.0

    def frame_off_by_one(c):
        p = c["plan"]
        my, mx, _ = tables(c)
        return apply64(c["src"], my, mx, (torch.arange(p.T_out) + 1).clamp_max(p.T - 1)) * 2.0 - 1.0

    def unscaled(c):
        return apply64(c["src"], *tables(c))

    def reversed_channels(c):
        return c["ref64"].flip(1)

    def truncated(c):
        return (c["spec32"].contiguous().view(torch.int32) & -65536).view(torch.float32)

    return {"bilinear without antialias": bilinear, "align_corners=True centres": corners, "unnormalised weights": unnormalised,
            "lo off by one": lo_off_by_one, "x and y tables swapped": swapped, "crop offset dropped": no_offset,
            "t_idx wraps": wraps, "frame off by one": frame_off_by_one, "lost * 2 - 1": unscaled,
            "channels reversed": reversed_channels, "truncation to bf16": truncated}
