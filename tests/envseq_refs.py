"""Shared references of the env_sequence tests (a light per frame: drn_env_cubes, drn_env_project_seq): the case grids, the
float64 evaluations, the fp32 torch specification's own error against them (E_ref, the unit of the kernels' bounds) and
independent numpy fp32 stand-ins of both entries with the wrong variants the bounds have to catch.  Everything here runs on the
CPU; every case is computed once.  The projection's references, tie mask and bound are those of tests/envmap_refs.py."""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

import envmap_refs as ER

# ------------------------------------------------------------------------------------------------ drn_env_cubes: cases
PANO_SIZES = [(24, 48), (17, 31)]            # He, We: the second is a multiple of nothing
N_LIGHTS = 3
CUBE_RES = [8, 32]
FLIPS = [False, True]
ROTS = [0.0, 90.0, 37.0, 359.0]              # 37 and 359: We * rot / 360 is no integer, int() and round() differ
BRIGHTNESS = [1.0, 0.5, 2.0]
SLICES = [(0, 3), (1, 2), (2, 1)]            # (n0, n): whole, a run from the middle, the last panorama alone


def _cube_cases():
    """The full product of (panorama size, R, flip, env_rot): 32 cases.  Brightness and the slice do not interact with the index
    arithmetic those four decide, so they cycle through their 9 combinations along the list (period 9 against 32 cases: every
    combination appears three times or more, with both flips and every rotation)."""
    combos = list(itertools.product(BRIGHTNESS, SLICES))
    out = []
    for i, (size, R, flip, rot) in enumerate(itertools.product(PANO_SIZES, CUBE_RES, FLIPS, ROTS)):
        b, (n0, n) = combos[i % len(combos)]
        out.append(dict(size=size, R=R, flip=flip, rot=rot, brightness=b, n0=n0, n=n))
    return out


CUBE_CASES = _cube_cases()
CUBE_CASE_IDS = [f"{c['size'][0]}x{c['size'][1]}_R{c['R']}_flip{int(c['flip'])}_rot{int(c['rot'])}_b{c['brightness']}_n{c['n0']}+{c['n']}"
                 for c in CUBE_CASES]

# err_i = |got_i - ref64_i| / s_i <= M_CUBES * E_ref at every element, s_i = the largest of the element's four cleaned taps.
# The rule is envmap_refs.py's: the smallest power of two that leaves 2x over the worst ratio measured on an MI355X, never above
# M_MAX.  Measured (profiles/envseq_parity.txt): 0.96 - 1.08 over the 32 cases, so 2 * 1.08 = 2.16 -> 4.  (E_ref is the error of ONE
# other fp32 evaluation, which sums its taps in another order; where the two round in opposite directions the kernel lands a
# little above E_ref.)
M_CUBES = 4
M_MAX = ER.M_MAX


def panoramas(He, We):
    """N_LIGHTS HDR panoramas, each envmap_refs.panorama()-like (rand^4 * 50) with its own seed; one NaN, one +inf, one -inf, one
    negative, one 65504 and one 0 texel planted across the frames."""
    p = torch.stack([torch.rand(He, We, 3, generator=torch.Generator().manual_seed(20250311 + k)).pow(4) * 50.0
                     for k in range(N_LIGHTS)])
    p[0, 3, 5, 0] = float("nan")
    p[1, 7, 13] = float("inf")
    p[2, 10, 20, 1] = float("-inf")
    p[0, 12, 2] = -3.5
    p[1, 5, 9] = 65504.0
    p[2, 15, 30] = 0.0
    return p


def _sample(pe, latlong, grid, c, dtype):
    """The specification in `dtype`: apply_hdr_preprocessing (elementwise, fp32: the values every evaluation gathers) and the
    grid_sample of latlong_to_cubemap_official with the fp32 grid the kernel receives -> [n, 6, R, R, 3]."""
    out = []
    for k in range(c["n0"], c["n0"] + c["n"]):
        clean = pe.apply_hdr_preprocessing(latlong[k], c["brightness"], c["flip"], c["rot"], "cpu")
        src = clean.permute(2, 0, 1).unsqueeze(0).to(dtype).expand(6, -1, -1, -1)
        out.append(F.grid_sample(src, grid.to(dtype), mode="bilinear", padding_mode="border", align_corners=False).permute(0, 2, 3, 1))
    return torch.stack(out)


def _tap_scale(pe, latlong, grid, c):
    """s_i: per output element the largest of its four cleaned tap values (float64 index arithmetic from the fp32 grid)."""
    He, We = latlong.shape[1:3]
    g = grid.double().numpy()
    ix = np.clip(((g[..., 0] + 1.0) * We - 1.0) / 2.0, 0.0, We - 1.0)
    iy = np.clip(((g[..., 1] + 1.0) * He - 1.0) / 2.0, 0.0, He - 1.0)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, We - 1), np.minimum(y0 + 1, He - 1)
    out = []
    for k in range(c["n0"], c["n0"] + c["n"]):
        clean = pe.apply_hdr_preprocessing(latlong[k], c["brightness"], c["flip"], c["rot"], "cpu").double().numpy()
        out.append(np.maximum(np.maximum(clean[y0, x0], clean[y0, x1]), np.maximum(clean[y1, x0], clean[y1, x1])))
    return torch.from_numpy(np.stack(out))


def cube_err(got, c):
    """max_i |got_i - ref64_i| / s_i; where s_i = 0 the result must be exactly 0 (else inf).  NaN anywhere -> inf."""
    got = got.double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    s, ref = c["scale"], c["ref"]
    zero = s == 0
    if bool((got[zero] != 0).any()):
        return float("inf")
    return ((got - ref).abs()[~zero] / s[~zero]).max().item()


_CACHE = {}


def cube_case(pkg, i):
    """Inputs and references of CUBE_CASES[i], computed once: latlong [3, He, We, 3] raw, grid [6, R, R, 2] (fp32, CPU), ref
    (float64), scale (s_i), e_ref, roll, shape of the output."""
    key = ("cubes", i)
    if key not in _CACHE:
        pe = ER.pe_module(pkg)
        c = dict(CUBE_CASES[i])
        He, We = c["size"]
        latlong, grid = panoramas(He, We), pe.cube_sample_grid(c["R"], "cpu")
        c.update(latlong=latlong, grid=grid, ref=_sample(pe, latlong, grid, c, torch.float64), scale=_tap_scale(pe, latlong, grid, c),
                 roll=pe.sequence_roll(We, c["rot"]), shape=(c["n"], 6, c["R"], c["R"], 3))
        c["spec32"] = _sample(pe, latlong, grid, c, torch.float32)
        c["e_ref"] = cube_err(c["spec32"], c)
        assert 0.0 < c["e_ref"] < 1e-5, c["e_ref"]
        _CACHE[key] = c
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ drn_env_cubes: stand-in
CUBE_MUTANTS = ["flip_lost", "roll_wrong_way", "roll_before_flip", "roll_rounded", "brightness_after_clamp", "not_cleaned",
                "panorama_0", "n0_ignored", "grid_xy_swapped", "align_corners", "wrap", "he_we_exchanged"]


def standin_cubes(latlong, grid, n0, n, brightness, flip, rot_deg, mutant=None):
    """What drn_env_cubes computes, written independently of the package and of the kernel's index arithmetic: the cleaned,
    flipped and rolled panorama is built as an array (numpy fp32, np.roll) and gathered once per tap.  `mutant` names one
    deliberate mistake."""
    f = np.float32
    latlong, grid = latlong.numpy(), grid.numpy()
    He, We = latlong.shape[1:3]
    gx, gy = (grid[..., 1], grid[..., 0]) if mutant == "grid_xy_swapped" else (grid[..., 0], grid[..., 1])
    roll = (round if mutant == "roll_rounded" else int)(We * rot_deg / 360) if rot_deg != 0 else 0
    if mutant == "roll_wrong_way":
        roll = -roll

    def clean(p):
        p = p.astype(f)
        if mutant == "not_cleaned":
            return p * f(brightness) if brightness != 1.0 else p
        with np.errstate(invalid="ignore", over="ignore"):
            if brightness != 1.0 and mutant != "brightness_after_clamp":
                p = p * f(brightness)
            p = np.clip(np.nan_to_num(p, nan=0.0, posinf=65504.0, neginf=0.0), f(0.0), f(65504.0)).astype(f)
            if brightness != 1.0 and mutant == "brightness_after_clamp":
                p = p * f(brightness)
        return p

    def coord(g, size):
        if mutant == "align_corners":
            u = (g + f(1.0)) / f(2.0) * f(size - 1)
        else:       # one fused multiply-add: the product of two fp32 numbers and the - 1 are exact in float64, rounded once
            u = ((g + f(1.0)).astype(f).astype(np.float64) * size - 1.0).astype(f) / f(2.0)
        if mutant == "wrap":
            u = np.where(u < 0, u + f(size), u).astype(f)
            i0 = np.floor(u)
            return (u - i0).astype(f), i0.astype(np.int64) % size, (i0.astype(np.int64) + 1) % size
        u = np.minimum(f(size - 1), np.maximum(u, f(0.0))).astype(f)
        i0 = np.floor(u)
        return (u - i0).astype(f), i0.astype(np.int64), np.minimum(i0.astype(np.int64) + 1, size - 1)

    sx, sy = (He, We) if mutant == "he_we_exchanged" else (We, He)
    wx, x0, x1 = coord(gx, sx)
    wy, y0, y1 = coord(gy, sy)
    if mutant == "he_we_exchanged":
        x0, x1, y0, y1 = np.minimum(x0, We - 1), np.minimum(x1, We - 1), np.minimum(y0, He - 1), np.minimum(y1, He - 1)
    wx, wy = wx[..., None], wy[..., None]
    out = []
    for k in range(n):
        src = 0 if mutant == "panorama_0" else (k if mutant == "n0_ignored" else n0 + k)
        p = clean(latlong[src])
        if mutant == "roll_before_flip":
            p = np.roll(p, roll, axis=1)
        if flip and mutant != "flip_lost":
            p = p[:, ::-1]
        if mutant != "roll_before_flip":
            p = np.roll(p, roll, axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            e = (p[y0, x0] * ((f(1.0) - wx) * (f(1.0) - wy)) + p[y0, x1] * (wx * (f(1.0) - wy))
                 + p[y1, x0] * ((f(1.0) - wx) * wy) + p[y1, x1] * (wx * wy)).astype(f)
        out.append(e)
    return torch.from_numpy(np.stack(out))


# ------------------------------------------------------------------------------------------------ drn_env_project_seq: cases
# geometry (H, W, T, spin, R) from envmap_refs.CASES (their tie share is asserted there), three cube maps, a table per case,
# the chunk written at t0 of outputs that hold T_all frames
PROJ_CASES = [dict(base=0, cube_of=[2, 0, 1], t0=1, T_all=5), dict(base=2, cube_of=[1, 1, 0, 2], t0=2, T_all=7)]
PROJ_CASE_IDS = [ER.CASE_IDS[c["base"]] + "_cubes" + "".join(str(k) for k in c["cube_of"]) + f"_t{c['t0']}of{c['T_all']}" for c in PROJ_CASES]
PROJ_MUTANTS = ["cube_of_ignored", "cube_of_next", "t0_ignored", "stride_T"]
SENTINEL = -7.0          # outside [-1, 1]: no tone map produces it


def proj_case(pkg, i):
    """Inputs and references of PROJ_CASES[i], computed once: cubes [3, 6, R, R, 3], vec, rot (fp32, CPU), cube_of, t0, T_all, ref
    (float64 pair [3, T, H, W]), mask, e_ref."""
    key = ("proj", i)
    if key not in _CACHE:
        pe = ER.pe_module(pkg)
        c = dict(PROJ_CASES[i])
        H, W, T, spin, R = ER.CASES[c["base"]]
        assert len(c["cube_of"]) == T
        cubes = torch.stack([pe.latlong_to_cubemap_official(pe.apply_hdr_preprocessing(p, 1.0, False, 0.0, "cpu"), [R, R])
                             for p in panoramas(24, 48)]).contiguous()
        vec, rot = pe.latlong_vec((H, W), device="cpu").contiguous(), pe.spin_table(spin, T).contiguous()
        per = [ER.ref64(pe, cubes[k], vec, rot[t:t + 1]) for t, k in enumerate(c["cube_of"])]
        ref = tuple(torch.cat([p[j] for p in per], dim=1) for j in (0, 1))
        per32 = [ER.torch_path(pe, cubes[k], vec, rot[t:t + 1], ER.LOG_SCALE, torch.float32) for t, k in enumerate(c["cube_of"])]
        spec32 = tuple(torch.cat([p[j] for p in per32], dim=1) for j in (0, 1))
        mask = ER.tie_mask(vec, rot)
        e_ref = ER.max_err(spec32, ref, mask)
        assert 0.0 < e_ref < 1e-4, e_ref
        c.update(cubes=cubes, vec=vec, rot=rot, ref=ref, mask=mask, e_ref=e_ref, spin=spin, T=T, H=H, W=W, R=R)
        _CACHE[key] = c
    return _CACHE[key]


def standin_project_seq(c, mutant=None):
    """What drn_env_project_seq leaves in two sentinel-filled [3, T_all, H, W] outputs, from envmap_refs.standin (one cube map, all
    frames) evaluated per light.  `mutant` names one deliberate mistake."""
    T, H, W, T_all, t0 = c["T"], c["H"], c["W"], c["T_all"], c["t0"]
    per_light = [ER.standin(c["cubes"][k], c["vec"], c["spin"], T) for k in range(c["cubes"].shape[0])]
    out = [np.full(3 * T_all * H * W, SENTINEL, np.float32) for _ in (0, 1)]
    plane = (T if mutant == "stride_T" else T_all) * H * W
    at = 0 if mutant == "t0_ignored" else t0
    for t in range(T):
        k = 0 if mutant == "cube_of_ignored" else c["cube_of"][(t + 1) % T if mutant == "cube_of_next" else t]
        for j in (0, 1):
            frame = per_light[k][j][:, t].numpy()
            for ch in range(3):
                o = ch * plane + (at + t) * H * W
                out[j][o:o + H * W] = frame[ch].reshape(-1)
    return tuple(torch.from_numpy(o).view(3, T_all, H, W) for o in out)


def sequence_references(pe, cubes, vec, rot):
    """envmap_refs.references for a light per frame: frame t from its own cube map cubes[t] under rot[t] -> per frame a dict of
    ref (float64 pair [3, 1, H, W]), mask [1, H, W] and e_ref, the fp32 torch path's own error on that frame's inputs.  E_ref
    depends on the light (a dark texel beside a bright one under a pixel raises it a hundredfold), so it has no fixed ceiling
    here."""
    out = []
    for t, cube in enumerate(cubes):
        cube, r = cube.contiguous(), rot[t:t + 1].contiguous()
        ref, mask = ER.ref64(pe, cube, vec, r), ER.tie_mask(vec, r)
        e_ref = ER.max_err(ER.torch_path(pe, cube, vec, r, ER.LOG_SCALE, torch.float32), ref, mask)
        assert e_ref > 0.0
        out.append(dict(ref=ref, mask=mask, e_ref=e_ref))
    return out


def proj_err(out, c):
    """(max |out - ref64| over the chunk's frames outside the tie mask, every other frame still the sentinel)."""
    t0, T = c["t0"], c["T"]
    out = tuple(o.cpu() for o in out)
    err = ER.max_err(tuple(o[:, t0:t0 + T] for o in out), c["ref"], c["mask"])
    rest = all(bool((o[:, :t0] == SENTINEL).all()) and bool((o[:, t0 + T:] == SENTINEL).all()) for o in out)
    return (err if math.isfinite(err) else float("inf")), rest
