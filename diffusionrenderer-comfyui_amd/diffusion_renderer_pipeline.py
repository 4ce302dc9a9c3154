"""Drop-in boundary: CleanDiffusionRendererPipeline with the reference's constructor and generate_video
signatures (diffusion_renderer_pipeline.py:38-111, :242-321).  Shape inference -> config -> (cached) model ->
sample -> decode -> post-process -> uint8 (B,T,H,W,C) numpy array.

Kept from the reference: attribute knobs (`guidance`, `num_steps`, `seed`, `set_model_type`), the shape-key
search order, the md5 config cache, every tensor of the batch cast to (device, dtype), ValueError when no usable
key exists.  Only the pre-loaded-model path is contractual: the reference's dynamic loader calls a method that
does not exist; here it raises a clear error instead.
"""
import dataclasses
import hashlib
import json
import os
from typing import Dict

import numpy as np
import torch

from . import native as N
from .diffusion_renderer_config import get_config_from_tensor_shape, validate_config
from .ensemble import check_ensemble, member_seed, reduce_results
from .fit import restore_frames, restore_frames_guided
from .model_diffusion_renderer import CleanDiffusionRendererModel
from .sampler import check_sampler
from .step_cache import MAX_RUN, check_step_cache
from .tiles import blend_tile, latent_tile, plan_tiles
from .windows import Window, check_window_align, plan_windows, ramp_weights

_SHAPE_KEYS = ("rgb", "image", "basecolor", "normal", "depth", "roughness", "metallic")


class CleanDiffusionRendererPipeline:
    def __init__(self, checkpoint_dir: str, checkpoint_name: str, model_type: str = "inverse", vae_instance=None,
                 model_instance=None, guidance: float = 2.0, num_steps: int = 20, height: int = 1024, width: int = 1024,
                 num_video_frames: int = 1, seed: int = 42, dtype: torch.dtype = torch.bfloat16):
        self.checkpoint_dir = checkpoint_dir
        self.checkpoint_name = checkpoint_name
        self.model_type = model_type.lower() if model_type else None
        self.vae_instance = vae_instance
        self.pre_loaded_model_instance = model_instance
        self.guidance = guidance
        self.num_steps = num_steps
        self.default_height = height
        self.default_width = width
        self.default_num_video_frames = num_video_frames
        self.seed = seed
        # long clips (windows.py): a clip of more than `window_frames` frames (8k + 1; 0 = off, 57 = the training length) is
        # rendered as windows of that length overlapping by `window_overlap` frames, cross-faded where the decoded frames
        # become uint8
        self.window_frames = 0
        self.window_overlap = 8
        # windows that agree (windows.align_affine): every window after the first is matched in gain and offset to the
        # previous window's carry over the overlap, on the device, before the cross-fade; False = today's calls, today's bits
        self.window_align = False
        # the fit's way back (fit.py): a RestorePlan -> the uint8 outputs are resampled to the source's size on the device, before
        # the D2H copy; None = the outputs keep the model's size (today's path, today's bits)
        self.restore_plan = None
        # the guided way back (fit.py): a fit.RestoreGuide (the plan, the source picture and the source as the model
        # saw it, on the device) -> where a restore plan is set, the outputs come back by joint bilateral upsampling with the
        # source as the guide (drn_restore_guided_u8); None = the plain way back (today's path, today's bits)
        self.restore_guide = None
        # large pictures (tiles.py): a picture larger than tile_height x tile_width (multiples of 16; 0 = that axis is not tiled,
        # both 0 = off; 576 x 1024 = the training size) is rendered as overlapping tiles of exactly that size, each an independent
        # sample, cross-faded over `tile_overlap` rows / columns where the results lie as uint8 on the device
        self.tile_height = 0
        self.tile_width = 0
        self.tile_overlap = 64
        # how tiles are joined: "pixel" = independent samples, cross-faded as uint8 (above); "latent" = joint
        # sampling: ONE noisy latent canvas for the picture, every tile's Euler step cross-faded into it at every step, so that
        # neighbours agree; needs tile_overlap on the tokenizer's 8-grid and a canvas-shaped init_noise
        self.tile_join = "pixel"
        # the sampler of the denoising loop (sampler.py): "euler" = the reference's first-order EDM Euler (today's
        # calls, today's bits); "dpmpp_2m" = DPM-Solver++(2M), second order at the same cost per step, so `num_steps` can be lower;
        # not with tile_join = "latent"
        self.sampler = "euler"
        # seed ensembles (ensemble.py): `ensemble` = N > 1 renders every call N times, under the seeds seed, seed + 1,
        # ... (wrapped at 2^64), and reduces the N uint8 results per pixel on the device: normal passes by the renormalised vector
        # sum, every other pass by `ensemble_reduce` ("median" / "mean"); 1 = off (today's calls, today's bits); not with an
        # init_noise
        self.ensemble = 1
        self.ensemble_reduce = "median"
        # ensembles that agree (ensemble.py): with `ensemble` > 1, every non-normal pass's members are first matched
        # to member 0 in gain and offset - one (g, o) per member and clip, solved on the device from the members' Gram matrix - and
        # the reduce reads every byte through its member's pair; False = off (today's calls, today's bits); ignored at ensemble = 1.
        # `last_ensemble_align`: per batch and pass of the last call the fp32 [N, B, 2] affines on the device, None for a normal
        # pass; empty where the switch was off
        self.ensemble_align = False
        self.last_ensemble_align = []
        # step cache (step_cache.py): a threshold in (0, 1] lets every sample loop skip the DiT blocks behind the first
        # on steps where the first block's output moved by less than that (relative L1) since the last computed step, at most
        # `step_cache_max_run` steps in a row; 0 = off (today's calls, today's bits); not with tile_join = "latent".  Windows, pixel
        # tiles and ensemble members each run their own loop and so their own cache.  `last_step_cache`: per sample loop of the
        # last call its log, per step (computed, delta or None)
        self.step_cache = 0.0
        self.step_cache_max_run = MAX_RUN
        self.last_step_cache = []
        self.device = torch.device("cuda")    # torch "cuda" == HIP on ROCm (reference :81)
        self.dtype = dtype
        self.config = None
        self.model = None
        self._config_cache = {}
        self._model_cache = {}

    def set_model_type(self, model_type: str):
        new = model_type.lower()
        if self.model_type != new:
            self.model_type = new
            self.config = None
            self.model = None
            self.__dict__.pop("_h2d_cache", None)     # a new renderer starts from a new clip

    @staticmethod
    def _resolved(device) -> torch.device:
        """torch.device("cuda") (what the reference's constructor stores, :81) names the CURRENT device; tensors report an
        indexed one ("cuda:0").  Compare devices only after resolving the default index."""
        d = torch.device(device)
        if d.type == "cuda" and d.index is None:
            return torch.device("cuda", torch.cuda.current_device())
        return d

    @staticmethod
    def _get_config_hash(config) -> str:
        return hashlib.md5(json.dumps(config, sort_keys=True, default=str).encode()).hexdigest()

    def _ensure_model_loaded(self, input_tensor_shape: tuple):
        new_config = get_config_from_tensor_shape(self.model_type, input_tensor_shape)
        new_config["model_type"] = self.model_type
        h = self._get_config_hash(new_config)
        if self.config is not None and self._get_config_hash(self.config) == h:
            return self.model
        if h in self._model_cache:
            self.config = new_config
            self.model = self._model_cache[h]
            return self.model
        self.config = new_config
        validate_config(self.config)
        inst = self.pre_loaded_model_instance
        if isinstance(inst, dict):
            # {"inverse": model, "forward": model}: the two renderers are different checkpoints (in_channels 33 vs 153); the
            # reference reuses the inverse-built net for both and cannot run the forward pass
            inst = inst.get(self.model_type)
        if inst is not None:
            self.model = self._configure_pre_loaded_model(inst, self.config)
        else:
            self.model = self._load_model_with_config()
        self._model_cache[h] = self.model
        return self.model

    def _configure_pre_loaded_model(self, model_instance, config):
        """Re-point a loaded model at a new shape/condition config without touching weights (reference :168-198).

        The weights' own network config (channel counts) stays the model's: the reference rewrites
        `model.config` wholesale, which silently mismatches in_channels for the forward pass."""
        net_cfg = model_instance.config.get("net") if isinstance(model_instance.config, dict) else None
        model_instance.config = dict(config)
        if net_cfg is not None and model_instance.net is not None:
            model_instance.config["net"] = net_cfg
        model_instance.condition_keys = config.get("condition_keys", ["image", "depth", "normal", "basecolor", "roughness", "metallic"])
        model_instance.condition_drop_rate = config.get("condition_drop_rate", 0.0)
        model_instance.append_condition_mask = config.get("append_condition_mask", True)
        model_instance.input_data_key = config.get("input_data_key", "video")
        if self.vae_instance:
            model_instance.vae = self.vae_instance
        return model_instance.to(self.device)

    def _move_to_device(self, data_batch):
        """Every tensor -> (device, dtype) as the reference does (:200-208); the copy of an unchanged source tensor is
        reused across calls (the inverse node hands the same clip to 5 consecutive passes)."""
        out = {}
        cache = self.__dict__.setdefault("_h2d_cache", {})
        dev = self._resolved(self.device)
        live = {}
        for k, v in data_batch.items():
            if not isinstance(v, torch.Tensor):
                out[k] = v
                continue
            key = (id(v), v._version, tuple(v.shape), v.dtype)
            hit = live.get(key) or cache.get(key)          # (rgb and video are usually the SAME tensor: one copy)
            if hit is None or hit[0] is not v or hit[1].device != dev:
                hit = (v, v.to(device=dev, dtype=self.dtype))
            live[key] = hit
            out[k] = hit[1]
        # only the tensors of the batch in hand stay referenced (the node builds a fresh clip tensor per call: an entry of an
        # earlier call can never hit again and would pin ~0.6 GB of host + HBM per cfg-3 clip)
        self._h2d_cache = live
        return out

    def _load_model_with_config(self):
        path = os.path.join(self.checkpoint_dir, self.checkpoint_name)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"checkpoint not found: {path} (pass a pre-loaded model_instance, as the loader node does)")
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(path)
        else:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        if "model" in sd:
            sd = sd["model"]
        model = CleanDiffusionRendererModel(self.config, device=self.device)
        model.load_state_dict(sd, strict=True)
        if self.vae_instance:
            model.vae = self.vae_instance
        return model

    def generate_video(self, data_batch: Dict[str, torch.Tensor], normalize_normal: bool = False, seed: int = None,
                       init_noise: torch.Tensor = None, to_host: bool = True) -> np.ndarray:
        """to_host=False (here and in the two methods below): the result stays on the pipeline's device, a torch.uint8 tensor
        [B, T, H, W, 3] with the bytes of the array the default call returns."""
        return self._render([data_batch], [[bool(normalize_normal)]], seed, init_noise, clips=True, to_host=to_host)[0][0]

    def generate_video_passes(self, data_batch: Dict[str, torch.Tensor], normalize_normal, seed: int = None,
                              init_noise: torch.Tensor = None, to_host: bool = True):
        """P G-buffer passes of ONE clip stepped together: `data_batch["context_index"]` is [P, 1], the
        clip tensors keep batch 1, `normalize_normal` is a sequence of P flags.  Returns the P uint8 arrays generate_video
        would return for the passes run one after the other (reference nodes.py:191-213): same seed -> same start noise,
        one encode instead of P, one batched denoiser call per step."""
        return self._render([data_batch], [[bool(f) for f in normalize_normal]], seed, init_noise, to_host=to_host)[0]

    def generate_video_each(self, data_batches, normalize_normal, seed: int = None, init_noise: torch.Tensor = None,
                            to_host: bool = True):
        """generate_video for several batches over ONE clip (the inverse node's passes run one after the other), returned in
        order.  With windows the loop is windows outside, batches inside: the batches share the clip tensor, so they share each
        window's slice of it, and the upload and encode caches still see one clip per window instead of one per window and pass."""
        batches = list(data_batches)
        flags = [bool(f) for f in normalize_normal]
        if len(flags) != len(batches):
            raise ValueError(f"{len(flags)} normalize_normal flags for {len(batches)} batches")
        return [o[0] for o in self._render(batches, [[f] for f in flags], seed, init_noise, clips=True, to_host=to_host)]

    def _restored(self, u8, frames=None, t0=0):
        """The uint8 result [B, T', H', W', 3] at the source's size where a restore plan is set (fit.restore_frames, on the device),
        cut to the plan's T frames, or to `frames` (a window's written frames: a windowed clip has no time padding).  With a
        restore guide the way back is fit.restore_frames_guided; t0: the clip's frame the first of these frames is (a window's
        `out_at`), where the guide is read."""
        if self.restore_plan is None:
            return u8
        if self.restore_guide is not None:
            guide = self.restore_guide
            gplan = dataclasses.replace(guide.plan, T=int(self.restore_plan.T if frames is None else frames))
            return restore_frames_guided(u8, gplan, guide.hi, guide.lo, t0=int(t0))
        rplan = self.restore_plan if frames is None else dataclasses.replace(self.restore_plan, T=int(frames))
        return restore_frames(u8, rplan)

    def _window_plan(self, data_batch):
        """The windows of this clip, or None where the clip is one sequence (windows off, or a clip that fits one)."""
        if not self.window_frames:
            return None
        inst = self.pre_loaded_model_instance
        if isinstance(inst, dict):
            inst = inst.get(self.model_type)
        if getattr(inst if inst is not None else self.model, "process_group", None) is not None:
            raise NotImplementedError("windows under sequence parallelism are not implemented: set window_frames = 0")
        ref = self._shape_tensor(data_batch)
        T = ref.shape[2] if ref.ndim == 5 else 1
        plan = plan_windows(T, self.window_frames, self.window_overlap)     # ValueError on a bad length / overlap
        return plan if len(plan) > 1 else None

    def _tile_plan(self, data_batch):
        """The spatial tiles of this picture (tiles.plan_tiles), or None where it is one tile (tiles off, or a picture that fits)."""
        if not (self.tile_height or self.tile_width):
            return None
        inst = self.pre_loaded_model_instance
        if isinstance(inst, dict):
            inst = inst.get(self.model_type)
        if getattr(inst if inst is not None else self.model, "process_group", None) is not None:
            raise NotImplementedError("tiles under sequence parallelism are not implemented: set tile_height = tile_width = 0")
        ref = self._shape_tensor(data_batch)
        if ref.ndim != 5:
            return None
        return plan_tiles(ref.shape[3], ref.shape[4], self.tile_height, self.tile_width, self.tile_overlap)   # ValueError on a bad size

    def _check_settings(self, init_noise=None):
        """ValueError for settings that cannot be rendered, before any GPU work."""
        if self.tile_join not in ("pixel", "latent"):
            raise ValueError(f"tile_join must be 'pixel' or 'latent', got {self.tile_join!r}")
        check_sampler(self.sampler, self.tile_join)
        check_window_align(self.window_align, self.window_frames, self.window_overlap, self.tile_height, self.tile_width)
        check_ensemble(self.ensemble, self.ensemble_reduce, init_noise, self.ensemble_align)
        check_step_cache(self.step_cache, self.step_cache_max_run, self.tile_join)

    def _render(self, batches, flags, seed, init_noise, clips=False, to_host=True):
        """Per batch, per pass: uint8 [B, T, H, W, 3] (numpy on the host, or with to_host=False torch tensors on the pipeline's
        device).  A picture of one tile is `_walk`, untouched.  A larger one is rendered tile by tile in raster order around that
        same walk: every 5-D tensor of the picture's (H, W) is cropped to the tile (once per tensor identity: rgb / video, and the
        batches of one clip, share a crop), the walk runs on the crops with its result left on the device at the tile's size -
        windows, carries and passes as they are, same seed, same start noise: every tile has one shape -, and each result is
        cross-faded into that pass's full-size canvas (tiles.blend_tile).  After the last tile the restore plan is applied once
        per canvas (it also cuts the time padding; with a restore guide, guided), then the copy to the host.  Device memory: one full-size uint8 canvas per
        pass plus one tile's results.

        tile_join = "latent"  changes where the tiles' samples come from and nothing behind them: `_joint_samples`
        denoises all tiles of every window together on one latent canvas, and the same walk then decodes each tile's crop of
        the final canvases instead of sampling - post-process, carries and the pixel cross-fade as above, because the decoder
        sees each tile's own context.  At tile_overlap = 0 there is nothing to join: "latent" is then the hard-cut tiling above
        with each tile started from its crop of the canvas noise (`_tile_noises`)."""
        self._check_settings(init_noise)
        self.last_step_cache = []
        self.last_ensemble_align = []
        if not batches:
            return []
        if self.ensemble > 1:
            return self._render_ensemble(batches, flags, seed, clips, to_host)[0]
        return self._render_member(batches, flags, seed, init_noise, clips, to_host)

    def _render_ensemble(self, batches, flags, seed, clips=False, to_host=True, spread=False):
        """`ensemble` = N members of one call -> (results, spreads or None), per batch and pass as `_render`
        returns them.  Member k is the one render below - windows, tiles, sampler and passes as they are inside it - under the
        seed (seed + k) mod 2^64, its results left on the device at the model's size: the restore plan and guide are taken
        away for the members and put back whatever happens.  Per batch and pass the N results are reduced per pixel
        (ensemble.reduce_members: 'normal' where the pass's flag is set, `ensemble_reduce` elsewhere), each member's tensor freed
        as soon as its pass is reduced; the way back then runs ONCE, on the reduced result (guided where a guide is set; the
        spreads take the plain way back), which also cuts the time padding; the copy to the host comes last.  Device memory: N
        results of one call at the model's size.  With `ensemble_align` (ignored at ensemble = 1) the members of
        every non-normal pass are solved and reduced through their affines, still per batch and pass, still at the model's size
        in front of the one way back; the affines stay on the device in `last_ensemble_align`."""
        base = seed if seed is not None else self.seed
        rplan, rguide = self.restore_plan, self.restore_guide
        self.restore_plan = self.restore_guide = None
        try:
            members = [self._render_member(batches, flags, member_seed(base, k), None, clips, False)
                       for k in range(int(self.ensemble))]
        finally:
            self.restore_plan, self.restore_guide = rplan, rguide
        if self.ensemble_align and int(self.ensemble) > 1:
            results, spreads, self.last_ensemble_align = reduce_results(members, flags, self.ensemble_reduce, spread=spread,
                                                                        align=True)
        else:
            results, spreads = reduce_results(members, flags, self.ensemble_reduce, spread=spread)
        del members
        results = [[self._restored(r) for r in rs] for rs in results]
        host = (lambda t: t.cpu().numpy()) if to_host else (lambda t: t)
        if not spread:
            return [[host(r) for r in rs] for rs in results], None
        try:
            self.restore_guide = None                              # a spread is no picture of the source: the plain way back
            spreads = [[self._restored(s) for s in ss] for ss in spreads]
        finally:
            self.restore_guide = rguide
        return [[host(r) for r in rs] for rs in results], [[host(s) for s in ss] for ss in spreads]

    def generate_video_ensemble(self, data_batches, normalize_normal, seed: int = None, to_host: bool = True):
        """generate_video_each under `self.ensemble` members, with the members' spread: -> (results, spreads), two lists of uint8
        [B, T, H, W, 3] in the batches' order.  A spread is the median (mean) absolute deviation of the members per byte, or for a
        normal pass 255 * (1 - the mean resultant length) in all three channels; it comes back through the plain restore also
        where a guide is set.  At ensemble = 1 the reduce still runs on the one member: a normal pass is renormalised, every
        other result is the member and its spread 0."""
        batches = list(data_batches)
        flags = [bool(f) for f in normalize_normal]
        if len(flags) != len(batches):
            raise ValueError(f"{len(flags)} normalize_normal flags for {len(batches)} batches")
        self._check_settings()
        self.last_step_cache = []
        self.last_ensemble_align = []
        if not batches:
            return [], []
        results, spreads = self._render_ensemble(batches, [[f] for f in flags], seed, clips=True, to_host=to_host, spread=True)
        return [r[0] for r in results], [s[0] for s in spreads]

    def _render_member(self, batches, flags, seed, init_noise, clips=False, to_host=True):
        """One sample of `_render`'s call: everything `_render`'s text says, behind its checks."""
        tiles = self._tile_plan(batches[0])
        if tiles is None:
            return self._walk(batches, flags, seed, init_noise, clips, to_host)
        H, W = self._shape_tensor(batches[0]).shape[3:5]
        canvas = None
        # tile_join = "latent": the tiles are sampled jointly first; the walk then decodes each tile's crop of the final canvases.
        # Without an overlap the tiles share no latent: each is sampled on its own, from its crop of the ONE canvas noise
        joint = noises = None
        if self.tile_join == "latent":
            if self.tile_overlap:
                joint = self._joint_samples(batches, tiles, seed, init_noise)
            else:
                noises = self._tile_noises(batches, tiles, seed, init_noise)
        rplan, self.restore_plan = self.restore_plan, None         # the way back runs once, on the joined picture
        try:
            for n, tile in enumerate(tiles):
                if joint is not None:
                    outs = self._walk(batches, flags, seed, None, clips, False, provider=joint(n))
                else:
                    cropped = {}

                    def crop(v):
                        if not (isinstance(v, torch.Tensor) and v.ndim == 5 and tuple(v.shape[3:5]) == (H, W)):
                            return v
                        if id(v) not in cropped:
                            cropped[id(v)] = (v, v[..., tile.y:tile.y + tile.h, tile.x:tile.x + tile.w].contiguous())
                        return cropped[id(v)][1]
                    outs = self._walk([{k: crop(v) for k, v in b.items()} for b in batches], flags, seed,
                                      init_noise if noises is None else noises[n], clips, False)
                if canvas is None:
                    canvas = [[torch.empty(tuple(o.shape[:2]) + (H, W, 3), dtype=torch.uint8, device=o.device) for o in per_batch]
                              for per_batch in outs]
                for cs, os_ in zip(canvas, outs):
                    for c, o in zip(cs, os_):
                        blend_tile(c, o, tile)
        finally:
            self.restore_plan = rplan
        done = [[self._restored(c) for c in cs] for cs in canvas]
        return [[c.cpu().numpy() if to_host else c for c in cs] for cs in done]

    def _latent_plan(self, batches, tiles):
        """What tile_join = "latent" needs to know of a tiled picture -> (the clip's windows or None, the frames of one sample,
        the tiles in latent units, the latent canvas's shape (C, F, H/f, W/f)).  Loads the model for one tile's shape;
        ValueError for a tile_overlap off the tokenizer's grid."""
        ref = self._shape_tensor(batches[0])
        T, H, W = ref.shape[2:5]
        plan = self._window_plan(batches[0])
        Wf = T if plan is None else int(self.window_frames)
        self._ensure_model_loaded((ref.shape[0], ref.shape[1], Wf, tiles[0].h, tiles[0].w))
        f = int(getattr(self.model.vae if getattr(self.model, "vae", None) is not None else self.vae_instance,
                        "spatial_compression_factor", 8))
        if self.tile_overlap % f:
            raise ValueError(f"tile_join = 'latent' needs tile_overlap on the tokenizer's grid (a multiple of {f}), got "
                             f"{self.tile_overlap}: one latent pixel must be the same {f} x {f} pixels in every tile")
        lat = [latent_tile(t, f) for t in tiles]                   # (H and W off the grid are refused here)
        return plan, Wf, lat, (self.config["latent_shape"][0], (Wf - 1) // 8 + 1, H // f, W // f)

    def _tile_noises(self, batches, tiles, seed, init_noise):
        """tile_join = "latent" at tile_overlap = 0 -> per tile its start noise: its crop of the ONE canvas noise of the picture
        (`init_noise`, which must be canvas-shaped, or as the joint loop draws it: the seed, one randn of the canvas shape times
        sigma_0).  With it the pixel path renders the hard-cut tiling: tiles that share no latent are independent samples,
        whatever canvas they are cut from.  (The joint loop would not give that where the last row or column of tiles is
        shifted back: DESIGN.md 4i.)"""
        _, _, lat, canvas_shape = self._latent_plan(batches, tiles)
        if init_noise is not None:
            if tuple(init_noise.shape[-4:]) != canvas_shape:
                raise ValueError(f"init_noise {tuple(init_noise.shape)} is not canvas-shaped: tile_join = 'latent' starts from ONE "
                                 f"noise canvas [1 or P, {', '.join(map(str, canvas_shape))}] for the whole picture (a tile-shaped "
                                 "init_noise belongs to tile_join = 'pixel')")
            noise = init_noise
        else:
            torch.manual_seed(seed if seed is not None else self.seed)
            self.model.scheduler.set_timesteps(self.num_steps)
            noise = torch.randn(size=(1, *canvas_shape), **self.model._get_tensor_kwargs()) * self.model.scheduler.sigmas[0]
        return [noise[..., t.y:t.y + t.h, t.x:t.x + t.w].contiguous() for t in lat]

    def _joint_samples(self, batches, tiles, seed, init_noise):
        """tile_join = "latent": the joint samples of a tiled picture (model.generate_samples_joint) -> provider_of(n), the sample
        provider `_walk` takes for tile n: (window i, batch c) -> that tile's crop of the final latent canvas of window i and
        batch c.  Windows outside (every window starts from the same canvas noise, as every window starts from the same noise
        without tiles), tiles inside, batches innermost: per window and tile every clip tensor is cut, cropped and uploaded once
        (rgb / video, and the batches of one clip, share it and so share the encode), the tile's condition latents are built
        with the model's own `_get_conditions`, and only they are kept - the pixel crops are dropped tile by tile.  Held until
        the picture is done: one canvas [P, C, F, H/f, W/f] bf16 per window and batch."""
        plan, Wf, lat, canvas_shape = self._latent_plan(batches, tiles)
        T, H, W = self._shape_tensor(batches[0]).shape[2:5]
        starts = [0] if plan is None else [win.start for win in plan]
        dev = self._resolved(self.device)
        samples = []
        for start in starts:
            conds = [[] for _ in batches]
            for tile in tiles:
                parts = {}

                def part(v):
                    if not isinstance(v, torch.Tensor):
                        return v
                    if id(v) not in parts:
                        p = v
                        if p.ndim == 5 and tuple(p.shape[3:5]) == (H, W):
                            p = p[..., tile.y:tile.y + tile.h, tile.x:tile.x + tile.w]
                        if plan is not None and p.ndim == 5 and p.shape[2] == T:
                            p = p[:, :, start:start + Wf]
                        parts[id(v)] = (v, p.contiguous().to(device=dev, dtype=self.dtype))
                    return parts[id(v)][1]
                for c, b in enumerate(batches):
                    tb = {k: part(v) for k, v in b.items()}
                    self.model._get_conditions(tb)
                    conds[c].append({k: tb[k] for k in ("latent_condition", "context_index") if k in tb})
            samples.append([self.model.generate_samples_joint(cs, lat, canvas_shape, guidance=self.guidance,
                                                              seed=seed if seed is not None else self.seed,
                                                              num_steps=self.num_steps, init_noise=init_noise) for cs in conds])
            del conds

        def provider_of(n):
            t = lat[n]
            return lambda i, c: samples[i][c][..., t.y:t.y + t.h, t.x:t.x + t.w].contiguous()
        return provider_of

    def _walk(self, batches, flags, seed, init_noise, clips=False, to_host=True, provider=None):
        """The one walk from batches to uint8 frames -> per batch, per pass: uint8 [B, T, H, W, 3], numpy arrays on the host, or
        with to_host=False torch tensors on the pipeline's device (the same walk: only the buffer the written frames are copied
        into lives there, so what the inverse renderer made can feed the forward renderer without a host round trip).  Walk the clip's
        windows in order.  Per window and batch: slice every clip tensor, sample (same seed, same start noise: every window has one
        shape), decode pass by pass, cross-fade with the carry of the previous window inside the uint8 post-process, resample to
        the source's size where a restore plan is set, and copy the written frames to the host.  The window's last `overlap`
        decoded frames become the next carry.  Device memory: one window's decode plus one carry per pass, whatever T is.
        With `window_align`, a window that has a carry and is no normal pass (unit vectors have no gain or offset freedom) is first
        matched to that carry (N.window_align_affine: the affine stays on the device), and one launch applies the affine, writes
        the frames and hands on the ALIGNED last frames as the next carry, so every window lands in window 0's space.

        A clip that is one sequence is one window over the caller's own tensors (the upload cache knows them by identity) that
        writes every frame the tokenizer decoded, with no ramp and no carry.  clips: generate_video's contract for such a clip - the
        sample's rows are clips under the one flag, decoded together - where otherwise every row is a pass with a flag of its own.
        provider: (window index, batch index) -> that window's sample, in place of sampling it here (`_joint_samples`); without
        one the walk is untouched."""
        if not batches:
            return []
        plan = self._window_plan(batches[0])
        whole = plan is None
        if whole:
            plan, Wf, O, T, ramp = [Window(0, 0, 0, 0, 0)], 0, 0, 0, None       # (write_hi 0: every frame the tokenizer decodes)
        else:
            Wf, O = int(self.window_frames), int(self.window_overlap)
            T = self._shape_tensor(batches[0]).shape[2]
            ramp = torch.from_numpy(ramp_weights(O)).to(self._resolved(self.device)) if O else None
        together = clips and whole
        outs = [[None] * len(f) for f in flags]
        carry = [[None] * len(f) for f in flags]
        for i, win in enumerate(plan):
            sliced = {}             # id(clip tensor) -> (tensor, its window): rgb / video, and the batches of one clip, share a slice

            def cut(v):
                if not (isinstance(v, torch.Tensor) and v.ndim == 5 and v.shape[2] == T):
                    return v
                if id(v) not in sliced:
                    sliced[id(v)] = (v, v[:, :, win.start:win.start + Wf].contiguous())
                return sliced[id(v)][1]
            for c, (batch, fl) in enumerate(zip(batches, flags)):
                if provider is not None:        # sampled already (tile_join = "latent"): window i's sample of batch c
                    sample = provider(i, c)
                else:
                    sample = self._sample(batch if whole else {k: cut(v) for k, v in batch.items()}, seed, init_noise)
                if not together and sample.shape[0] != len(fl):
                    raise ValueError(f"{len(fl)} normalize_normal flags for {sample.shape[0]} passes")
                for p, flag in enumerate(fl):
                    video = self.model.decode(sample if together else sample[p:p + 1]).to(self.dtype).contiguous()
                    if not whole and video.shape[2] != Wf:
                        raise ValueError(f"the tokenizer decoded {video.shape[2]} frames for a window of {Wf}")
                    prev = carry[c][p]                                                # None: window 0, or hard cuts
                    hand_on = O and i + 1 < len(plan)
                    aligned = bool(self.window_align) and not whole and prev is not None and not flag
                    if aligned:
                        affine = N.window_align_affine(video, prev, win.ramp_at)
                        u8, tail = N.postprocess_window_align_u8(video, prev, ramp, affine, win.ramp_at, win.write_lo, win.write_hi,
                                                                 flag, carry_frames=O if hand_on else 0)
                    else:
                        u8 = N.postprocess_window_u8(video, prev, ramp if prev is not None else None, win.ramp_at, win.write_lo,
                                                     win.write_hi or video.shape[2], flag)
                    # frames are independent: window by window = the whole clip.  Kept: those written, up to the restore plan's T
                    # (the time padding of a whole clip is cut; a windowed clip has none)
                    if self.restore_plan is not None:
                        u8 = self._restored(u8, frames=min(u8.shape[1], self.restore_plan.T - win.out_at), t0=win.out_at)
                    if outs[c][p] is None:
                        outs[c][p] = torch.empty((u8.shape[0], u8.shape[1] if whole else T) + tuple(u8.shape[2:]), dtype=torch.uint8,
                                                 device="cpu" if to_host else u8.device)
                    outs[c][p][:, win.out_at:win.out_at + u8.shape[1]].copy_(u8)      # D2H straight into the clip's frames
                    if aligned:
                        carry[c][p] = tail
                    else:
                        carry[c][p] = video[:, :, Wf - O:].contiguous() if hand_on else None
        return [[o.numpy() if to_host else o for o in per_batch] for per_batch in outs]

    @staticmethod
    def _shape_tensor(data_batch):
        for key in _SHAPE_KEYS:
            if key in data_batch:
                return data_batch[key]
        raise ValueError(f"No suitable input tensor for shape inference found in data_batch. Looked for {list(_SHAPE_KEYS)}")

    def _sample(self, data_batch, seed, init_noise):
        effective_seed = seed if seed is not None else self.seed
        data_batch = self._move_to_device(data_batch)
        video_tensor = self._shape_tensor(data_batch)
        self._ensure_model_loaded(tuple(video_tensor.shape))
        C = self.config["latent_shape"][0]
        _, _, T, H, W = video_tensor.shape
        state_shape = [C, (T - 1) // 8 + 1, H // 8, W // 8]
        # (under "euler" the call is the reference's, argument for argument)
        other = {} if self.sampler == "euler" else {"sampler": self.sampler}
        if self.step_cache:
            other.update(step_cache=float(self.step_cache), step_cache_max_run=int(self.step_cache_max_run))
        sample = self.model.generate_samples_from_batch(data_batch, guidance=self.guidance, state_shape=state_shape,
                                                        num_steps=self.num_steps, is_negative_prompt=False,
                                                        seed=effective_seed, init_noise=init_noise, **other)
        if self.step_cache:
            self.last_step_cache.append(list(getattr(self.model.net, "step_cache_log", None) or []))
        return sample
