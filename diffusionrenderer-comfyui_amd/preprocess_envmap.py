"""Environment-map conditions of the forward (relighting) renderer: env_ldr / env_log / env_nrm.

Preprocessing per clip, outside the denoising loop.  With static lighting it runs once and is
plain torch on the device.  Mirrors the public functions the reference's forward node imports (nodes.py:25-31):
render_projection_from_panorama (:408-467), tonemap_image_direct (:469-526), latlong_vec (:320-338),
clear_environment_cache, get_cache_stats, with the same tone-mapping arithmetic (rgb2srgb :109-113, reinhard :115-117,
hdr_mapping :119-140), HDR clean-up (:263-286) and lat-long -> cube-map resampling (:161-206); all of these are pinned to the
reference's own functions by tests/golden/envmap.safetensors (tests/test_envmap_spin_cpu.py).

env_spin (degrees over the clip) fills in the reference's unused per-frame hook `y_rot = rotate_y(0.0)` (:340-348, :442): frame
t of T is projected under the y-rotation radians(env_spin) * t / T.  The per-frame torch loop (project_frame) specifies it and
is what CPU devices run; on a GPU one launch of drn_env_project (csrc/envmap.hip) projects every frame.

env_sequence (off by default) lights frame t with frame t of the env_map batch, of which the reference reads frame 0 only
(process_comfyui_tensor :247-261): per frame the clean-up, the cube map and project_frame.  That torch loop specifies it and is what
CPU devices run; on a GPU drn_env_cubes builds the cube maps of 16 frames in one launch and drn_env_project_seq projects them.

One deliberate difference: the reference projects the cube map with nvdiffrast (`dr.texture(..., boundary_mode='cube')`,
:448-449), a CUDA-only third-party library that is neither installed here nor portable to ROCm.  `cube_lookup` below is
a from-scratch bilinear cube-map fetch (major-axis face selection, the inverse of the reference's own `cube_to_dir`
face convention, per-face bilinear filtering with clamped edges).  PARITY UNPINNED for that lookup (no nvdiffrast to
compare with); it agrees with sampling the panorama directly up to the cube-map's own resampling error
(tests/test_envmap.py).
"""
import hashlib
import logging
import time
from typing import Dict, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

logger = logging.getLogger(__name__)


class EnvironmentMapCache:
    """LRU cache of processed environment maps (reference :23-66)."""

    def __init__(self, max_size: int = 10):
        self.cache, self.access_times, self.max_size = {}, {}, max_size

    @staticmethod
    def _key(env_hash, resolution, fmt, brightness, flip, rot):
        return f"{env_hash}_{resolution}_{fmt}_{brightness}_{flip}_{rot}"

    def get(self, env_hash, resolution, fmt, brightness, flip, rot):
        k = self._key(env_hash, resolution, fmt, brightness, flip, rot)
        if k in self.cache:
            self.access_times[k] = time.time()
            return self.cache[k]
        return None

    def put(self, env_hash, resolution, fmt, brightness, flip, rot, result):
        k = self._key(env_hash, resolution, fmt, brightness, flip, rot)
        if len(self.cache) >= self.max_size and k not in self.cache:
            oldest = min(self.access_times, key=self.access_times.get)
            del self.cache[oldest], self.access_times[oldest]
        self.cache[k] = result
        self.access_times[k] = time.time()

    def clear(self):
        self.cache.clear()
        self.access_times.clear()


_env_cache = EnvironmentMapCache()


def clear_environment_cache():
    _env_cache.clear()


def get_cache_stats() -> Dict[str, int]:
    return {"cache_size": len(_env_cache.cache), "max_size": _env_cache.max_size}


def compute_tensor_hash(t: torch.Tensor) -> str:
    flat = t.detach().reshape(-1)
    idx = torch.linspace(0, flat.numel() - 1, min(1000, flat.numel())).long()
    sample = flat[idx.to(flat.device)].float().cpu().numpy().tobytes()
    return hashlib.md5(sample + str(tuple(t.shape)).encode()).hexdigest()


# ---------------------------------------------------------------------------------------------- tone mapping
def rgb2srgb_official(rgb: torch.Tensor) -> torch.Tensor:
    return torch.where(rgb <= 0.0031308, 12.92 * rgb, 1.055 * torch.pow(torch.clamp(rgb, 1e-8, 1.0), 1.0 / 2.4) - 0.055)


def reinhard_official(x: torch.Tensor, max_point: float = 16.0) -> torch.Tensor:
    return x / (x + 1.0) * max_point


def hdr_mapping_official(env_hdr: torch.Tensor, log_scale: float = 10000.0) -> Dict[str, torch.Tensor]:
    env_ev0 = rgb2srgb_official(reinhard_official(env_hdr, max_point=16.0).clamp(0, 1))
    env_log = rgb2srgb_official(torch.log1p(env_hdr) / np.log1p(log_scale)).clamp(0, 1)
    return {"env_hdr": env_hdr, "env_ev0": env_ev0, "env_log": env_log}


# ---------------------------------------------------------------------------------------------- geometry
def safe_normalize(v: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    return v / (torch.norm(v, dim=-1, keepdim=True) + eps)


def cube_to_dir(s: int, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Face s, face coordinates (x, y) in [-1, 1] -> direction (reference :142-155)."""
    one = torch.ones_like(x)
    return [torch.stack([one, -y, -x], -1), torch.stack([-one, -y, x], -1), torch.stack([x, one, y], -1),
            torch.stack([x, -one, -y], -1), torch.stack([x, -y, one], -1), torch.stack([-x, -y, -one], -1)][s]


def latlong_to_cubemap_official(latlong_map: torch.Tensor, res) -> torch.Tensor:
    """(H, W, C) equirectangular -> (6, res0, res1, C) cube map by bilinear grid_sample (reference :161-206)."""
    dev = latlong_map.device
    cube = torch.zeros(6, res[0], res[1], latlong_map.shape[-1], dtype=torch.float32, device=dev)
    gy, gx = torch.meshgrid(torch.linspace(-1.0 + 1.0 / res[0], 1.0 - 1.0 / res[0], res[0], device=dev),
                            torch.linspace(-1.0 + 1.0 / res[1], 1.0 - 1.0 / res[1], res[1], device=dev), indexing="ij")
    src = latlong_map.permute(2, 0, 1).unsqueeze(0).float()
    for s in range(6):
        v = safe_normalize(cube_to_dir(s, gx, gy))
        tu = torch.atan2(v[..., 0:1], -v[..., 2:3]) / (2 * np.pi) + 0.5
        tv = torch.acos(torch.clamp(v[..., 1:2], min=-1, max=1)) / np.pi
        grid = (torch.cat((tu, tv), dim=-1) * 2.0 - 1.0).unsqueeze(0)
        cube[s] = F.grid_sample(src, grid, mode="bilinear", padding_mode="border", align_corners=False)[0].permute(1, 2, 0)
    return cube


def cube_lookup(cubemap: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """Bilinear cube-map fetch: cubemap (6, R, R, C), dirs (..., 3) -> (..., C).  Inverse of cube_to_dir's convention."""
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    ax, ay, az = x.abs(), y.abs(), z.abs()
    is_x = (ax >= ay) & (ax >= az)
    is_y = (~is_x) & (ay >= az)
    ma = torch.where(is_x, ax, torch.where(is_y, ay, az)).clamp_min(1e-12)
    face = torch.where(is_x, torch.where(x > 0, 0, 1), torch.where(is_y, torch.where(y > 0, 2, 3), torch.where(z > 0, 4, 5)))
    # face coordinates (fx, fy) such that cube_to_dir(face, fx, fy) is parallel to dirs
    fx = torch.where(is_x, torch.where(x > 0, -z, z), torch.where(is_y, x, torch.where(z > 0, x, -x))) / ma
    fy = torch.where(is_x, -y, torch.where(is_y, torch.where(y > 0, z, -z), -y)) / ma
    R = cubemap.shape[1]
    out = torch.zeros(dirs.shape[:-1] + (cubemap.shape[-1],), dtype=cubemap.dtype, device=cubemap.device)
    grid = torch.stack([fx, fy], -1)
    for s in range(6):
        m = face == s
        if m.any():
            g = grid[m].view(1, 1, -1, 2)
            tex = cubemap[s].permute(2, 0, 1).unsqueeze(0)
            out[m] = F.grid_sample(tex, g, mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0].t()
    return out


def latlong_vec(res: Tuple[int, int] = None, device="cuda", resolution: Tuple[int, int] = None) -> torch.Tensor:
    """(H, W, 3) direction of every lat-long pixel (reference :320-338); `resolution=` is the keyword the node uses."""
    H, W = res if res is not None else resolution
    gy, gx = torch.meshgrid(torch.linspace(0.0 + 1.0 / H, 1.0 - 1.0 / H, H, device=device),
                            torch.linspace(-1.0 + 1.0 / W, 1.0 - 1.0 / W, W, device=device), indexing="ij")
    sintheta, costheta = torch.sin(gy * np.pi), torch.cos(gy * np.pi)
    sinphi, cosphi = torch.sin(gx * np.pi), torch.cos(gx * np.pi)
    return torch.stack((sintheta * sinphi, costheta, -sintheta * cosphi), dim=-1)


# ---------------------------------------------------------------------------------------------- loading / clean-up
def process_comfyui_tensor(t: torch.Tensor) -> torch.Tensor:
    if t.ndim == 4:
        if t.shape[1] in (3, 4):
            t = t.permute(0, 2, 3, 1)
        t = t[0]
    if t.shape[-1] == 4:
        t = t[..., :3]
    elif t.shape[-1] == 1:
        t = t.repeat(1, 1, 3)
    return t


def load_hdr_file(path: str) -> torch.Tensor:
    import imageio.v3 as iio          # optional dependency of the node pack (requirements.txt:5)
    img = np.asarray(iio.imread(path))
    if img.dtype == np.uint8:
        img = img.astype(np.float32) / 255.0
    elif img.dtype == np.uint16:
        img = img.astype(np.float32) / 65535.0
    else:
        img = img.astype(np.float32)
    if img.ndim == 2:
        img = np.stack([img] * 3, axis=-1)
    elif img.shape[-1] == 4:
        img = img[..., :3]
    return torch.from_numpy(img)


def _load(env_input: Union[str, torch.Tensor]) -> torch.Tensor:
    if isinstance(env_input, str):
        return load_hdr_file(env_input)
    if isinstance(env_input, torch.Tensor):
        return process_comfyui_tensor(env_input)
    raise ValueError(f"Unsupported input type: {type(env_input)}")


def apply_hdr_preprocessing(latlong: torch.Tensor, env_brightness: float, env_flip: bool, env_rot: float, device) -> torch.Tensor:
    latlong = latlong.to(device).float().clone()
    if env_brightness != 1.0:
        latlong = latlong * env_brightness
    latlong = torch.nan_to_num(latlong, nan=0.0, posinf=65504.0, neginf=0.0).clamp(0.0, 65504.0)
    if env_flip:
        latlong = torch.flip(latlong, dims=[1])
    if env_rot != 0:
        latlong = torch.roll(latlong, shifts=int(latlong.shape[1] * env_rot / 360), dims=1)
    return latlong


def _frames(t: torch.Tensor, n: int) -> torch.Tensor:
    return t.unsqueeze(0).expand(n, -1, -1, -1) if n > 1 else t.unsqueeze(0)


# ---------------------------------------------------------------------------------------------- rotating light (env_spin)
def rotate_y(angle: float, device="cpu") -> torch.Tensor:
    """4x4 rotation about +Y, fp32 from fp64 np.cos / np.sin (reference :340-348)."""
    c, s = np.cos(angle), np.sin(angle)
    return torch.tensor([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], dtype=torch.float32, device=device)


def spin_angles(env_spin: float, num_frames: int):
    """theta_t = radians(env_spin) * t / T of every frame: env_spin = 360 is one full turn over the clip."""
    return [float(np.radians(env_spin)) * t / num_frames for t in range(num_frames)]


def spin_table(env_spin: float, num_frames: int) -> torch.Tensor:
    """[T, 2] fp32 (cos theta_t, sin theta_t): the entries of rotate_y(theta_t), as drn_env_project takes them (host tensor)."""
    return torch.stack([rotate_y(a)[0, [0, 2]] for a in spin_angles(env_spin, num_frames)])


def project_frame(cubemap: torch.Tensor, vec: torch.Tensor, y_rot: torch.Tensor, log_scale: float = 10000.0) -> Dict[str, torch.Tensor]:
    """One frame of the projection at the reference's rotation hook (:441-450): vec (H, W, 3) turned by the 4x4 y_rot, looked up,
    flipped and tone-mapped.  This loop body is the specification of drn_env_project (csrc/envmap.hip)."""
    H, W = vec.shape[:2]
    vq = (vec.view(-1, 3) @ y_rot[:3, :3].T).view(H, W, 3)
    return hdr_mapping_official(torch.flip(cube_lookup(cubemap, -vq), dims=[0, 1]), log_scale=log_scale)


def _projection(env_input, resolution, env_brightness, env_flip, env_rot, device, num_frames, use_cache, env_spin, backend):
    """The cached worker behind render_projection_from_panorama / envmap_conditions.  Returns a dict: the torch path holds
    'env_ldr' / 'env_log' as (T, H, W, 3) in [0, 1]; the kernel path holds 'cond_ldr' / 'cond_log' as [3, T, H, W] in [-1, 1]."""
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    on_gpu = torch.device(device).type == "cuda"
    if backend == "hip" and not on_gpu:
        raise ValueError(f"backend='hip' needs a GPU device, got {device!r} (the torch path is what CPU devices run)")
    use_hip = backend == "hip" or (backend == "auto" and env_spin != 0 and on_gpu)
    # the cache key tells (env_spin, num_frames) apart through the format string; static lighting keeps the key it had
    fmt = ("proj" if env_spin == 0 else f"proj_spin{float(env_spin)}_T{num_frames}") + ("_hip" if use_hip else "")
    if use_cache:
        h = compute_tensor_hash(env_input) if isinstance(env_input, torch.Tensor) else hashlib.md5(str(env_input).encode()).hexdigest()
        hit = _env_cache.get(h, resolution, fmt, env_brightness, env_flip, env_rot)
        if hit is not None:
            return _expand_static(hit, num_frames, static=env_spin == 0)
    H, W = resolution
    latlong = apply_hdr_preprocessing(_load(env_input), env_brightness, env_flip, env_rot, device)
    cubemap = latlong_to_cubemap_official(latlong, [512, 512])
    vec = latlong_vec((H, W), device=device)
    if use_hip:
        from . import native                      # all frames in one launch, written in the conditions' final layout and range
        rot = spin_table(env_spin, num_frames if env_spin != 0 else 1).to(cubemap.device)
        ldr, log = native.env_project(cubemap.contiguous(), vec.contiguous(), rot, 10000.0)
        result = {"cond_ldr": ldr, "cond_log": log}        # static light: ONE frame, cached as such (its key carries no T)
    elif env_spin == 0:
        # camera = identity, y-rotation 0 (reference :441-446)
        env_proj = torch.flip(cube_lookup(cubemap, -vec), dims=[0, 1])
        m = hdr_mapping_official(env_proj, log_scale=10000.0)
        result = {"env_ldr": _frames(m["env_ev0"], num_frames), "env_log": _frames(m["env_log"], num_frames)}
    else:
        ms = [project_frame(cubemap, vec, rotate_y(a, device=device)) for a in spin_angles(env_spin, num_frames)]
        result = {"env_ldr": torch.stack([m["env_ev0"] for m in ms]), "env_log": torch.stack([m["env_log"] for m in ms])}
    if use_cache:
        _env_cache.put(h, resolution, fmt, env_brightness, env_flip, env_rot, result)
    return _expand_static(result, num_frames)


def _expand_static(d, num_frames, static=False):
    """The kernel path's one static frame [3, 1, H, W] expanded over the clip, after the cache (everything else: as stored)."""
    if "cond_ldr" in d and d["cond_ldr"].shape[1] == 1 and num_frames > 1:
        return {k: v.expand(-1, num_frames, -1, -1) for k, v in d.items()}
    if static and "env_ldr" in d and d["env_ldr"].shape[0] != num_frames:
        # the torch path stores its one frame expanded to the clip it was first asked for, under a key without T: a clip of
        # another length (a long clip's windows and then one window alone, say) gets the same frame at its own length
        return {k: _frames(v[0], num_frames) for k, v in d.items()}
    return d


# ---------------------------------------------------------------------------------------------- a light per frame (env_sequence)
SEQ_CUBE_RES = 512       # the cube map every frame's panorama is resampled to (what _projection builds for a static light)
SEQ_CHUNK = 16           # frames whose cube maps are in memory at once on the kernel path: 16 x 18.9 MB at R = 512


def process_comfyui_sequence(t: torch.Tensor) -> torch.Tensor:
    """process_comfyui_tensor's layout rules on EVERY frame of an env_map batch -> [N, He, We, 3]; a 3-D tensor is N = 1.
    Frame 0 is what process_comfyui_tensor returns."""
    if t.ndim == 3:
        t = t.unsqueeze(0)
    elif t.ndim == 4 and t.shape[1] in (3, 4):
        t = t.permute(0, 2, 3, 1)
    if t.shape[-1] == 4:
        t = t[..., :3]
    elif t.shape[-1] == 1:
        t = t.repeat(1, 1, 1, 3)
    return t


def _load_sequence(env_input: Union[str, torch.Tensor]) -> torch.Tensor:
    if isinstance(env_input, str):
        return load_hdr_file(env_input).unsqueeze(0)
    if isinstance(env_input, torch.Tensor):
        return process_comfyui_sequence(env_input)
    raise ValueError(f"Unsupported input type: {type(env_input)}")


def sequence_frames(env_input, clip_frames: int):
    """The frames of a light sequence, checked against the clip: [N, He, We, 3] with N == clip_frames, or None when N = 1 (a
    single light: today's path, today's cache key).  Any other N raises before any GPU work."""
    frames = _load_sequence(env_input)
    N = frames.shape[0]
    if N == 1:
        return None
    if N != clip_frames:
        raise ValueError(f"env_sequence: env_map holds N = {N} frames but the clip has T = {clip_frames}; a light sequence needs "
                         f"one env_map frame per clip frame (or a single frame)")
    return frames


def sequence_cube_of(n_lights: int, num_frames: int):
    """cube_of[t] = min(t, N - 1): frame t is lit by light t; over frames a fit padded in time, the last light repeats."""
    return [min(t, n_lights - 1) for t in range(num_frames)]


def _sequence_hash(frames: torch.Tensor) -> str:
    """EVERY frame's compute_tensor_hash plus N (that function samples 1000 elements of a tensor: over a whole sequence it would
    miss a small light that moves)."""
    return hashlib.md5("".join(compute_tensor_hash(f) for f in frames).encode() + str(frames.shape[0]).encode()).hexdigest()


_grid_cache = {}


def cube_sample_grid(res: int, device) -> torch.Tensor:
    """[6, res, res, 2] fp32: the grid_sample coordinates (x, y) of every cube texel, by the very torch expressions of
    latlong_to_cubemap_official - grid_sample of a panorama with grid[s] is that function's face s.  It does not depend on the
    panorama, so it is computed once per (res, device); drn_env_cubes reads it and evaluates no transcendental itself."""
    key = (int(res), str(torch.device(device)))
    if key not in _grid_cache:
        dev = torch.device(device)
        gy, gx = torch.meshgrid(torch.linspace(-1.0 + 1.0 / res, 1.0 - 1.0 / res, res, device=dev),
                                torch.linspace(-1.0 + 1.0 / res, 1.0 - 1.0 / res, res, device=dev), indexing="ij")
        faces = []
        for s in range(6):
            v = safe_normalize(cube_to_dir(s, gx, gy))
            tu = torch.atan2(v[..., 0:1], -v[..., 2:3]) / (2 * np.pi) + 0.5
            tv = torch.acos(torch.clamp(v[..., 1:2], min=-1, max=1)) / np.pi
            faces.append(torch.cat((tu, tv), dim=-1) * 2.0 - 1.0)
        _grid_cache[key] = torch.stack(faces).contiguous()
    return _grid_cache[key]


def sequence_roll(width: int, env_rot: float) -> int:
    """apply_hdr_preprocessing's roll, `int(We * env_rot / 360)` as torch.roll takes it, brought into [0, We)."""
    return int(width * env_rot / 360) % width if env_rot != 0 else 0


def project_sequence_hip(frames, cube_of, vec, rot, env_brightness, env_flip, roll, res=SEQ_CUBE_RES, chunk=SEQ_CHUNK,
                         log_scale=10000.0):
    """The kernel path of a light sequence: frames [N, He, We, 3] raw, vec [H, W, 3] and rot [T, 2] on the device, cube_of a host
    list of T non-decreasing light indices -> (cond_ldr, cond_log) as [3, T, H, W] in [-1, 1].  Per chunk of at most `chunk`
    frames one drn_env_cubes launch builds the cube maps the chunk looks up, one drn_env_project_seq launch projects the chunk
    into the clip's outputs; the cube maps of one chunk are all that is in memory."""
    from . import native
    T, (H, W) = rot.shape[0], vec.shape[:2]
    assert len(cube_of) == T and all(b >= a for a, b in zip(cube_of, cube_of[1:])), "cube_of: T non-decreasing indices"
    grid = cube_sample_grid(res, frames.device)
    out = (torch.empty((3, T, H, W), dtype=torch.float32, device=frames.device),
           torch.empty((3, T, H, W), dtype=torch.float32, device=frames.device))
    most = max(cube_of[min(t0 + chunk, T) - 1] - cube_of[t0] + 1 for t0 in range(0, T, chunk))
    cubes = torch.empty((most, 6, res, res, 3), dtype=torch.float32, device=frames.device)
    for t0 in range(0, T, chunk):
        t1 = min(t0 + chunk, T)
        k0, n = cube_of[t0], cube_of[t1 - 1] - cube_of[t0] + 1
        native.env_cubes(frames, grid, k0, n, env_brightness, env_flip, roll, out=cubes[:n])
        local = torch.tensor([k - k0 for k in cube_of[t0:t1]], dtype=torch.int32)          # rebased to the chunk's first panorama
        native.env_project_seq(cubes[:n], local, vec, rot[t0:t1], log_scale, out=out, t0=t0)
    return out


def _projection_sequence(frames, resolution, env_brightness, env_flip, env_rot, device, num_frames, use_cache, env_spin, backend):
    """_projection for a light sequence (frames: what sequence_frames returned).  Frame t of num_frames is lit by frame
    min(t, N - 1) under the rotation of spin_angles(env_spin, num_frames)[t].  The per-frame torch loop specifies it and is what
    CPU devices run; on a GPU two launches per 16 frames (project_sequence_hip)."""
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    on_gpu = torch.device(device).type == "cuda"
    if backend == "hip" and not on_gpu:
        raise ValueError(f"backend='hip' needs a GPU device, got {device!r} (the torch path is what CPU devices run)")
    use_hip = backend == "hip" or (backend == "auto" and on_gpu)       # ahead of the torch loop: profiles/envmap_sequence.txt
    N = frames.shape[0]
    fmt = f"proj_seq{N}_spin{float(env_spin)}_T{num_frames}" + ("_hip" if use_hip else "")
    if use_cache:
        h = _sequence_hash(frames)
        hit = _env_cache.get(h, resolution, fmt, env_brightness, env_flip, env_rot)
        if hit is not None:
            return hit
    H, W = resolution
    cube_of = sequence_cube_of(N, num_frames)
    vec = latlong_vec((H, W), device=device)
    if use_hip:
        rot = spin_table(env_spin, num_frames).to(device)
        ldr, log = project_sequence_hip(frames.to(device).float().contiguous(), cube_of, vec.contiguous(), rot, env_brightness,
                                        env_flip, sequence_roll(frames.shape[2], env_rot))
        result = {"cond_ldr": ldr, "cond_log": log}
    else:
        ms, k_have, cubemap = [], None, None
        for t, a in enumerate(spin_angles(env_spin, num_frames)):
            if cube_of[t] != k_have:
                k_have = cube_of[t]
                latlong = apply_hdr_preprocessing(frames[k_have], env_brightness, env_flip, env_rot, device)
                cubemap = latlong_to_cubemap_official(latlong, [SEQ_CUBE_RES, SEQ_CUBE_RES])
            ms.append(project_frame(cubemap, vec, rotate_y(a, device=device)))
        result = {"env_ldr": torch.stack([m["env_ev0"] for m in ms]), "env_log": torch.stack([m["env_log"] for m in ms])}
    if use_cache:
        _env_cache.put(h, resolution, fmt, env_brightness, env_flip, env_rot, result)
    return result


def _tonemap_sequence(frames, resolution, device, num_frames, use_cache=True):
    """tonemap_image_direct on every frame of a pre-rendered ball video: one F.interpolate over the batch, then the tone maps."""
    N = frames.shape[0]
    fmt = f"ball_seq{N}_T{num_frames}"
    if use_cache:
        h = _sequence_hash(frames)
        hit = _env_cache.get(h, resolution, fmt, 1.0, False, 0.0)
        if hit is not None:
            return hit
    H, W = resolution
    env = frames.to(device).float()
    if tuple(env.shape[1:3]) != (H, W):
        # planes made contiguous first: a permuted [N, He, We, 3] batch is a channels-last tensor, which F.interpolate answers
        # in channels-last memory, while the single-light call gets planes - the same values in another order in memory
        env = F.interpolate(env.permute(0, 3, 1, 2).contiguous(), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    # the tone maps frame by frame, not on the batch: torch's CPU pow runs the last few elements in memory (what is left of its
    # 32-wide vector loop) through another routine, so inside a batch the end of a frame would differ from the single-light
    # call in the last bit wherever H * W * 3 is no multiple of 32
    ms = [hdr_mapping_official(env[k], log_scale=10000.0) for k in range(N)]
    idx = sequence_cube_of(N, num_frames)
    result = {"env_ldr": torch.stack([ms[k]["env_ev0"] for k in idx]), "env_log": torch.stack([ms[k]["env_log"] for k in idx])}
    if use_cache:
        _env_cache.put(h, resolution, fmt, 1.0, False, 0.0, result)
    return result


def render_projection_from_panorama(env_input, resolution: Tuple[int, int], env_brightness: float = 1.0, env_flip: bool = True,
                                    env_rot: float = 180.0, device="cuda", num_frames: int = 1, use_cache: bool = True,
                                    env_spin: float = 0.0, backend: str = "auto", env_sequence: bool = False,
                                    clip_frames: int = None, **kwargs) -> Dict[str, torch.Tensor]:
    """Panorama -> 512^2 cube map -> lat-long projection -> tone maps: {'env_ldr','env_log'} as (T, H, W, 3) in [0, 1].

    env_spin (degrees): frame t of T is projected under the y-rotation radians(env_spin) * t / T, at the reference's own
    rotate_y hook; 0 = today's static light, one image expanded over T.  backend: 'auto' = the HIP kernel (drn_env_project) when
    the light turns and the device is a GPU, else torch (static lighting keeps its bits); 'torch' / 'hip' force a path.  The
    kernel writes the conditions' [-1, 1] tensors; what this function returns from them is (c + 1) / 2, permuted - a view
    in this function's layout, within one rounding of the tone maps themselves (envmap_conditions hands on the kernel's own).

    env_sequence: frame t is lit by frame t of env_input ([N, He, We, 3], read by process_comfyui_sequence), under frame t's own
    rotation when env_spin is set.  N must be 1 (today's path, bit for bit) or clip_frames, the clip's own frame count, which
    defaults to num_frames; where num_frames is larger (a fit padded the clip in time) the last light repeats.  backend 'auto'
    takes the kernels (drn_env_cubes, drn_env_project_seq) on a GPU."""
    frames = sequence_frames(env_input, num_frames if clip_frames is None else clip_frames) if env_sequence else None
    if frames is not None:
        d = _projection_sequence(frames, resolution, env_brightness, env_flip, env_rot, device, num_frames, use_cache, env_spin,
                                 backend)
    else:
        d = _projection(env_input, resolution, env_brightness, env_flip, env_rot, device, num_frames, use_cache, env_spin, backend)
    if "env_ldr" in d:
        return d
    return {"env_ldr": (d["cond_ldr"].permute(1, 2, 3, 0) + 1.0) * 0.5, "env_log": (d["cond_log"].permute(1, 2, 3, 0) + 1.0) * 0.5}


def tonemap_image_direct(env_input, resolution: Tuple[int, int], device="cuda", num_frames: int = 1, use_cache: bool = True,
                         **kwargs) -> Dict[str, torch.Tensor]:
    """A pre-rendered HDR image (chrome ball) -> resize -> tone maps."""
    if use_cache:
        h = compute_tensor_hash(env_input) if isinstance(env_input, torch.Tensor) else hashlib.md5(str(env_input).encode()).hexdigest()
        hit = _env_cache.get(h, resolution, "ball", 1.0, False, 0.0)
        if hit is not None:
            return _expand_static(hit, num_frames, static=True)
    H, W = resolution
    env = _load(env_input).to(device).float()
    if tuple(env.shape[:2]) != (H, W):
        env = F.interpolate(env.permute(2, 0, 1).unsqueeze(0), size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    m = hdr_mapping_official(env, log_scale=10000.0)
    result = {"env_ldr": _frames(m["env_ev0"], num_frames), "env_log": _frames(m["env_log"], num_frames)}
    if use_cache:
        _env_cache.put(h, resolution, "ball", 1.0, False, 0.0, result)
    return result


def envmap_conditions(env_map, resolution, num_frames, env_format="proj", env_brightness=1.0, env_flip=False, env_rot=0.0,
                      device="cuda", env_spin=0.0, backend="auto", env_sequence=False, clip_frames=None) -> Dict[str, torch.Tensor]:
    """The three forward-renderer conditions as (1, 3, T|1, H, W) tensors in [-1, 1] / unit vectors (reference nodes.py:283-304).
    env_spin / backend / env_sequence / clip_frames: see render_projection_from_panorama.  env_nrm holds camera-space directions
    and does not turn, nor change with the light."""
    if env_format not in ("proj", "ball"):
        raise ValueError(f"unknown env_format {env_format!r}")
    if env_format == "ball" and env_spin != 0:
        raise ValueError("env_spin needs env_format='proj': a pre-rendered ball cannot be rotated")
    # a sequence of one frame is a single light: None here, and today's path with today's cache key below
    frames = sequence_frames(env_map, num_frames if clip_frames is None else clip_frames) if env_sequence else None
    if env_format == "proj" and frames is None:
        d = _projection(env_map, resolution, env_brightness, env_flip, env_rot, device, num_frames, True, env_spin, backend)
    elif env_format == "proj":
        d = _projection_sequence(frames, resolution, env_brightness, env_flip, env_rot, device, num_frames, True, env_spin, backend)
    elif frames is None:
        d = tonemap_image_direct(env_map, resolution, device, num_frames)
    else:
        d = _tonemap_sequence(frames, resolution, device, num_frames)
    if "cond_ldr" in d:            # the kernel wrote the final layout and range
        env_ldr, env_log = d["cond_ldr"].unsqueeze(0), d["cond_log"].unsqueeze(0)
    else:
        env_ldr = d["env_ldr"].permute(3, 0, 1, 2).unsqueeze(0) * 2.0 - 1.0
        env_log = d["env_log"].permute(3, 0, 1, 2).unsqueeze(0) * 2.0 - 1.0
    env_nrm = latlong_vec(resolution, device=device).permute(2, 0, 1).unsqueeze(0).unsqueeze(2)
    return {"env_ldr": env_ldr, "env_log": env_log, "env_nrm": env_nrm}
