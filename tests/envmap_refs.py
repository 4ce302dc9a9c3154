"""Shared references of the env_spin tests (the rotating environment light, drn_env_project): the float64 evaluation of the torch
path, the fp32 torch path's own error against it (E_ref, the unit of the kernel's bound), the tie mask, and an independent fp32
stand-in with the wrong variants the bound has to catch.  Everything here runs on the CPU; every case is computed once."""
import importlib
import math

import numpy as np
import torch

LOG_SCALE = 10000.0
# (H, W, T, spin degrees, cube resolution R): odd sizes, sizes off the 256-thread block, more than one block, a full turn and a
# negative turn (frame 2 of the third case sits at -45 degrees, where a whole column of pixels lies on a face diagonal)
CASES = [(16, 24, 3, 111.0, 8), (18, 32, 5, 360.0, 32), (33, 47, 4, -90.0, 32), (18, 32, 4, 360.0, 16)]
CASE_IDS = ["16x24_T3_spin111_R8", "18x32_T5_spin360_R32", "33x47_T4_spin-90_R32", "18x32_T4_spin360_R16"]

# max|hip - ref64| <= M_BOUND * E_ref outside the tie mask.  Measured on an MI355X (profiles/envmap_parity.txt): against the float64
# evaluation the ratio max|hip - ref64| / E_ref is 0.99 - 1.00 at the four grid cases and at NODE_CASE - the kernel lands on the fp32
# torch path's own error.  The same bound is asked of the kernel against the DEVICE torch path (envmap_conditions, NODE_CASE): two
# fp32 evaluations that err in opposite directions at one pixel, measured ratio 1.97.  The rule is the smallest power of two that
# leaves 2x headroom over the worst ratio the bound is applied to (2 would do for the float64 comparisons alone), and never more
# than 16 (device powf / log1pf differ from the CPU libm by a few ulp; a larger ratio would mean a fast-math intrinsic or a wrong
# rounding order).  E_ref itself moves by a few per cent with the host CPU (4.4e-6 / 5.0e-6 at the second case on two hosts).
M_BOUND = 4
M_MAX = 16
TIE_REL = 1e-5           # two largest |components| of the float64 query direction this close: the face choice depends on rounding
TIE_SHARE_MAX = 0.01     # per frame


def pe_module(pkg):
    return importlib.import_module(pkg.__name__ + ".preprocess_envmap")


def panorama():
    """24 x 48 HDR panorama: rand^4 * 50 with one 65504 texel and one 0 texel."""
    g = torch.Generator().manual_seed(20240607)
    p = torch.rand(24, 48, 3, generator=g).pow(4) * 50.0
    p[7, 13] = 65504.0
    p[15, 30] = 0.0
    return p


def smooth_panorama():
    """A smooth panorama without symmetry in the azimuth, so a turn the wrong way round is far off."""
    ang = torch.linspace(-math.pi, math.pi, 49)[:-1] + math.pi / 48
    lat = torch.linspace(0, math.pi, 25)[:-1] + math.pi / 48
    x = torch.sin(lat)[:, None] * torch.sin(ang)[None]
    z = -torch.sin(lat)[:, None] * torch.cos(ang)[None]
    y = torch.cos(lat)[:, None].expand(24, 48)
    # channel 0 is dim enough for env_ldr (reinhard * 16, clamped at 1) not to saturate; the other two carry env_log
    return torch.stack([0.05 * (0.75 + 0.4 * x + 0.1 * z * y), 0.75 + 0.4 * z, 0.75 + 0.3 * x * z + 0.2 * y], -1)


def _rot4(c, s, dtype):
    return torch.tensor([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], dtype=dtype)


def torch_path(pe, cube, vec, rot, log_scale, dtype):
    """The package's per-frame loop (project_frame = the specification) in `dtype`, from the fp32 cube / directions / (cos, sin) table
    the kernel receives -> (env_ldr, env_log) as [3, T, H, W] in [-1, 1]."""
    cube, vec = cube.to(dtype), vec.to(dtype)
    ldr, log = [], []
    for t in range(rot.shape[0]):
        m = pe.project_frame(cube, vec, _rot4(float(rot[t, 0]), float(rot[t, 1]), dtype), log_scale)
        ldr.append(m["env_ev0"])
        log.append(m["env_log"])
    return tuple(torch.stack(x).permute(3, 0, 1, 2) * 2.0 - 1.0 for x in (ldr, log))


def ref64(pe, cube, vec, rot, log_scale=LOG_SCALE):
    return torch_path(pe, cube, vec, rot, log_scale, torch.float64)


def tie_mask(vec, rot):
    """[T, H, W] bool at OUTPUT positions: pixels whose float64 query direction has its two largest |components| within TIE_REL
    relative.  There the face legitimately depends on rounding and the per-face clamp makes the value discontinuous."""
    H, W = vec.shape[:2]
    out = []
    for t in range(rot.shape[0]):
        vq = vec.double().view(-1, 3) @ _rot4(float(rot[t, 0]), float(rot[t, 1]), torch.float64)[:3, :3].T
        a = vq.abs().sort(dim=-1, descending=True).values
        tie = ((a[:, 0] - a[:, 1]) <= TIE_REL * a[:, 0]).view(H, W)
        share = tie.float().mean().item()
        assert share <= TIE_SHARE_MAX, f"frame {t}: {share:.4f} of the pixels lie on a face tie"
        out.append(torch.flip(tie, dims=[0, 1]))
    return torch.stack(out)


def max_err(got, ref, mask):
    """max |got - ref| over both outputs, tie pixels left out.  got / ref: pairs of [3, T, H, W]."""
    keep = (~mask).unsqueeze(0)
    return max(((g.double().cpu() - r).abs() * keep).max().item() for g, r in zip(got, ref))


_CACHE = {}


NODE_CASE = (18, 32, 3, 120.0, 512)      # the 512^2 cube map the node builds: what envmap_conditions is compared at
NODE_CASE_ID = "18x32_T3_spin120_R512"


def references(pe, cube, vec, rot):
    """The float64 evaluation, the tie mask and E_ref for one set of kernel inputs (fp32, on the CPU)."""
    cube, vec, rot = cube.contiguous(), vec.contiguous(), rot.contiguous()
    ref = ref64(pe, cube, vec, rot)
    mask = tie_mask(vec, rot)
    e_ref = max_err(torch_path(pe, cube, vec, rot, LOG_SCALE, torch.float32), ref, mask)
    assert 0.0 < e_ref < 1e-4, e_ref
    return dict(cube=cube, vec=vec, rot=rot, ref=ref, mask=mask, e_ref=e_ref, shape=(3, rot.shape[0]) + tuple(vec.shape[:2]))


def case(pkg, i):
    """Inputs and references of CASES[i] (i = "node": NODE_CASE), computed once: cube / vec / rot (fp32, CPU), ref (float64 pair),
    mask, e_ref."""
    if i not in _CACHE:
        pe = pe_module(pkg)
        H, W, T, spin, R = NODE_CASE if i == "node" else CASES[i]
        latlong = pe.apply_hdr_preprocessing(panorama(), 1.0, False, 0.0, "cpu")
        _CACHE[i] = references(pe, pe.latlong_to_cubemap_official(latlong, [R, R]), pe.latlong_vec((H, W), device="cpu"),
                               pe.spin_table(spin, T))
    return _CACHE[i]


def node_case_on(pe, device):
    """NODE_CASE with the cube map and the directions built on `device`, as envmap_conditions builds them there, copied to the
    host: the float64 reference of the two device paths then starts from the very tensors they start from."""
    H, W, T, spin, R = NODE_CASE
    latlong = pe.apply_hdr_preprocessing(panorama(), 1.0, False, 0.0, device)
    return references(pe, pe.latlong_to_cubemap_official(latlong, [R, R]).cpu(), pe.latlong_vec((H, W), device=device).cpu(),
                      pe.spin_table(spin, T))


# ------------------------------------------------------------------------------------------------ independent fp32 stand-in
MUTANTS = ["rot_sign", "t_over_Tm1", "frame_off_by_one", "no_flips", "faces_2_3", "ldr_log_swapped", "no_scale", "wrap"]


def _srgb(v):
    f = np.float32
    p = f(1.055) * np.power(np.clip(v, f(1e-8), f(1.0)), f(1.0 / 2.4)) - f(0.055)
    return np.where(v <= f(0.0031308), f(12.92) * v, p).astype(np.float32)


def standin(cube, vec, spin, T, log_scale=LOG_SCALE, mutant=None):
    """What drn_env_project computes, written independently of the package: one gather per pixel (no masked grid_sample), numpy fp32,
    its own (cos, sin) from the spin.  `mutant` names one deliberate mistake."""
    f = np.float32
    cube, vec = cube.numpy(), vec.numpy()
    H, W, _ = vec.shape
    R = cube.shape[1]
    ldr, log = np.empty((3, T, H, W), f), np.empty((3, T, H, W), f)
    vx, vy, vz = vec[..., 0], vec[..., 1], vec[..., 2]
    for t in range(T):
        tt = t + 1 if mutant == "frame_off_by_one" else t
        th = math.radians(spin) * tt / ((T - 1) if mutant == "t_over_Tm1" else T)
        c, s = f(np.cos(th)), f(np.sin(th))
        if mutant == "rot_sign":
            s = -s
        x, y, z = -(c * vx + s * vz), -vy, -(c * vz - s * vx)
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        is_x = (ax >= ay) & (ax >= az)
        is_y = ~is_x & (ay >= az)
        ma = np.maximum(np.where(is_x, ax, np.where(is_y, ay, az)), f(1e-12))
        face = np.where(is_x, np.where(x > 0, 0, 1), np.where(is_y, np.where(y > 0, 2, 3), np.where(z > 0, 4, 5)))
        if mutant == "faces_2_3":
            face = np.where(face == 2, 3, np.where(face == 3, 2, face))
        fx = np.where(is_x, np.where(x > 0, -z, z), np.where(is_y, x, np.where(z > 0, x, -x))) / ma
        fy = np.where(is_x, -y, np.where(is_y, np.where(y > 0, z, -z), -y)) / ma

        def coord(g):
            u = ((g + f(1.0)) * f(R) - f(1.0)) / f(2.0)
            if mutant == "wrap":
                u = np.where(u < 0, u + f(R), u)
                i0 = np.floor(u)
                return u - i0, i0.astype(np.int64) % R, (i0.astype(np.int64) + 1) % R
            u = np.minimum(f(R - 1), np.maximum(u, f(0.0)))
            i0 = np.floor(u)
            return u - i0, i0.astype(np.int64), np.minimum(i0.astype(np.int64) + 1, R - 1)

        wx, x0, x1 = coord(fx)
        wy, y0, y1 = coord(fy)
        wx, wy = wx.astype(f)[..., None], wy.astype(f)[..., None]
        e = (cube[face, y0, x0] * ((f(1.0) - wx) * (f(1.0) - wy)) + cube[face, y0, x1] * (wx * (f(1.0) - wy))
             + cube[face, y1, x0] * ((f(1.0) - wx) * wy) + cube[face, y1, x1] * (wx * wy)).astype(f)
        ev0 = _srgb(np.clip(e / (e + f(1.0)) * f(16.0), f(0.0), f(1.0)))
        lg = np.clip(_srgb(np.log1p(e) / f(np.log1p(log_scale))), f(0.0), f(1.0))
        if mutant != "no_flips":
            ev0, lg = ev0[::-1, ::-1], lg[::-1, ::-1]
        if mutant != "no_scale":
            ev0, lg = ev0 * f(2.0) - f(1.0), lg * f(2.0) - f(1.0)
        ldr[:, t], log[:, t] = ev0.transpose(2, 0, 1), lg.transpose(2, 0, 1)
    if mutant == "ldr_log_swapped":
        ldr, log = log, ldr
    return torch.from_numpy(ldr), torch.from_numpy(log)


# ------------------------------------------------------------------------------------------------ guard bands (as tests/dit_refs.py, fp32)
SENTINEL32 = 0x7FE5A5A5       # a NaN pattern no tone map produces


def guarded32(n, pad, device):
    """ONE allocation of pad + n + pad fp32 elements filled with the sentinel -> (buffer, the n-element window in its middle)."""
    buf = torch.full((n + 2 * pad,), SENTINEL32, dtype=torch.int32, device=device).view(torch.float32)
    return buf, buf[pad:pad + n]


def assert_guard32(buf, pad, written=True):
    """Both bands still hold the sentinel; the window holds it nowhere (written) or everywhere (not written)."""
    bits = buf.view(torch.int32)
    assert bool((bits[:pad] == SENTINEL32).all()) and bool((bits[-pad:] == SENTINEL32).all()), "a guard band was written"
    hits = int((bits[pad:-pad] == SENTINEL32).sum())
    assert hits == (0 if written else bits.numel() - 2 * pad), f"{hits} window elements hold the sentinel"
