"""ComfyUI node API of the renderer, kept verbatim at the surface (reference nodes.py:61-347):
same class names, INPUT_TYPES / RETURN_TYPES / RETURN_NAMES / FUNCTION / CATEGORY, tensor conventions
((B,T,H,W,C) in [0,1]  <->  (B,C,T,H,W) in [-1,1]) and error types.  ComfyUI modules (folder_paths, comfy.*)
are imported lazily inside the methods that need them so the package also loads in tests and benches.
"""
import os

import numpy as np
import torch

from .diffusion_renderer_config import get_inverse_renderer_config
from .diffusion_renderer_pipeline import CleanDiffusionRendererPipeline
from .model_diffusion_renderer import CleanDiffusionRendererModel
from .ensemble import MAX_MEMBERS, REDUCES, check_ensemble
from .sampler import SAMPLERS, check_sampler
from .step_cache import check_step_cache
from .windows import check_window_align

GBUFFER_INDEX_MAPPING = {"basecolor": 0, "metallic": 1, "roughness": 2, "normal": 3, "depth": 4}   # nodes.py:35-41
INVERSE_PASSES = ["basecolor", "metallic", "roughness", "normal", "depth"]


def _progress_bar(n):
    try:
        from comfy.utils import ProgressBar
        return ProgressBar(n)
    except ImportError:
        class _NoBar:
            def update(self, *_):
                pass
        return _NoBar()


def _window_inputs():
    """Optional inputs of both renderers for long clips (windows.py; DESIGN.md "Long clips")."""
    return {"window_frames": ("INT", {"default": 0, "min": 0, "max": 1025, "step": 1,
                                      "tooltip": "0 = off: the whole clip is one sequence.  8k+1 frames (57 recommended: the "
                                                 "training length): longer clips are rendered as overlapping windows of this "
                                                 "length, cross-faded in pixel space"}),
            "window_overlap": ("INT", {"default": 8, "min": 0, "max": 512, "step": 1,
                                       "tooltip": "frames two neighbouring windows share (at most (window_frames - 1) / 2); "
                                                  "0 = hard cuts"}),
            "window_align": ("BOOLEAN", {"default": False,
                                         "tooltip": "windows are independent samples: level and contrast step from one window to "
                                                    "the next and the cross-fade only smears the step.  On: every window after the "
                                                    "first is matched in gain and offset (one pair for the three channels) to its "
                                                    "predecessor over the frames they share, on the GPU, before the cross-fade; "
                                                    "normal maps are never changed.  Needs window_overlap >= 1 and no tiles; "
                                                    "ignored where the clip fits one window"})}


def _tile_inputs():
    """Optional inputs of the renderers for large pictures (tiles.py)."""
    return {"tile_height": ("INT", {"default": 0, "min": 0, "max": 4096, "step": 16,
                                    "tooltip": "0 = off: the picture's whole height is one sequence.  A multiple of 16 (576 x 1024 "
                                               "recommended: the training size): a picture larger than tile_height x tile_width "
                                               "is rendered as overlapping tiles of exactly that size, cross-faded in pixel "
                                               "space.  Tiles apply to the FITTED picture (after fit, before fit_restore) and are "
                                               "independent samples: they share the seed but are not conditioned on each other, "
                                               "so two tiles may disagree - the cross-fade hides the seam, not the disagreement"}),
            "tile_width": ("INT", {"default": 0, "min": 0, "max": 4096, "step": 16,
                                   "tooltip": "0 = off: the picture's whole width is one sequence.  A multiple of 16 (1024 "
                                              "recommended, with tile_height 576)"}),
            "tile_overlap": ("INT", {"default": 64, "min": 0, "max": 2048, "step": 1,
                                     "tooltip": "rows / columns two neighbouring tiles share (at most half the tile's side); "
                                                "0 = hard cuts"}),
            "tile_join": (["pixel", "latent"],
                          {"default": "pixel",
                           "tooltip": "pixel: every tile is a sample of its own, joined as 8-bit pictures (above).  latent: the "
                                      "tiles are denoised together on ONE noisy latent canvas for the whole picture - at every "
                                      "step each tile's result is cross-faded into the canvas its neighbours read next, so that "
                                      "neighbouring tiles agree instead of only fading into each other; the pictures are still "
                                      "decoded tile by tile and cross-faded.  Costs: one latent canvas per window and pass held "
                                      "on the GPU (41 MB for five passes of 57 x 1072 x 1920), the same DiT calls, and "
                                      "tile_overlap must be a multiple of 8 (the tokenizer's grid; the default 64 is)"})}


def _sampler_inputs():
    """Optional inputs of the renderers for the denoising loop's sampler (sampler.py)."""
    return {"sampler": (list(SAMPLERS),
                        {"default": "euler",
                         "tooltip": "euler: the first-order EDM Euler loop (the default, unchanged).  dpmpp_2m: DPM-Solver++(2M), a "
                                    "second-order multistep sampler at the same cost per step - one model call -, so fewer steps "
                                    "reach the same answer (set `steps`); it keeps one fp32 copy of the latent as history.  Not "
                                    "with tile_join = latent"}),
            "steps": ("INT", {"default": 0, "min": 0, "max": 1000, "step": 1,
                              "tooltip": "denoising steps; 0 = leave the loaded pipeline's own number (15 from the loader node) as "
                                         "it is"}),
            "step_cache": ("FLOAT", {"default": 0.0, "min": 0.0, "max": 1.0, "step": 0.01,
                                     "tooltip": "0 = off (the default, unchanged).  > 0: a step cache (first-block cache) - every "
                                                "denoising step runs the first DiT block, and where its output moved by less than "
                                                "this (relative L1) since the last fully computed step, the other 27 blocks are "
                                                "not run and their last contribution is added instead; the first and the last step "
                                                "are always computed, and at most 3 steps in a row are skipped.  Faster, and the "
                                                "result changes; which threshold keeps a picture intact has not been measured on "
                                                "real weights.  Holds two copies of the hidden state on the GPU (302 MB per clip at "
                                                "57 x 576 x 1024).  Not with tile_join = latent"})}


def _ensemble_inputs():
    """Optional inputs of the nodes that run the inverse renderer, for seed ensembles (ensemble.py)."""
    return {"ensemble": ("INT", {"default": 1, "min": 1, "max": MAX_MEMBERS, "step": 1,
                                 "tooltip": "1 = off: one sample (the default, unchanged).  N > 1: the clip is rendered N times, "
                                            "under the seeds seed, seed + 1, ..., and the N results are reduced per pixel on the "
                                            "GPU - normal maps by the renormalised sum of the members' vectors, every other output "
                                            "by ensemble_reduce.  Costs N times the run time and N results held on the GPU; with "
                                            "sampler = dpmpp_2m at 8 steps a member costs about a quarter of a 35-step Euler pass"}),
            "ensemble_reduce": (list(REDUCES),
                                {"default": "median",
                                 "tooltip": "how the members of an ensemble become one picture, per byte: median (robust against "
                                            "a member that went wrong; the two middle values averaged at even N) or mean"}),
            "ensemble_align": ("BOOLEAN", {"default": False,
                                           "tooltip": "match every member of an ensemble to the first in gain and offset before "
                                                      "the members are reduced: relative depth and base colour come out of every "
                                                      "seed at a scale and shift of their own, and a median of members on "
                                                      "different scales blurs edges.  One gain and offset per member, output and "
                                                      "clip, solved on the GPU from all members together; normal maps are never "
                                                      "aligned; the result keeps the first member's scale.  Off: the members are "
                                                      "reduced as they are.  Ignored at ensemble = 1"})}


def _edit_inputs():
    """Optional inputs of the relight node for edits between its two stages (gbuffer_edit.py)."""
    gain = {"default": 1.0, "min": 0.0, "max": 8.0, "step": 0.01}
    offset = {"default": 0.0, "min": -1.0, "max": 1.0, "step": 0.01}
    layer = "the inserted object's {} as an IMAGE at the source's or the model's size (one frame for all, or one per frame); needs insert_mask"
    return {"edit_mask": ("MASK", {"tooltip": "where the material edit applies (1 = fully, 0 = not at all), at the source's or the "
                                              "model's size, one frame for all or one per frame; none = everywhere"}),
            "edit_base_color_tint": ("INT", {"default": 0xFFFFFF, "min": 0, "max": 0xFFFFFF, "step": 1, "display": "color",
                                             "tooltip": "the base colour is multiplied by this colour (0xRRGGBB) / 255, per channel"}),
            "edit_base_color_gain": ("FLOAT", dict(gain, tooltip="base colour gain (times the tint); 0 plus an offset = a constant")),
            "edit_roughness_gain": ("FLOAT", dict(gain, tooltip="roughness gain; 0 plus an offset = a constant roughness")),
            "edit_metallic_gain": ("FLOAT", dict(gain, tooltip="metallic gain; 0 plus an offset of 1 = fully metallic")),
            "edit_base_color_offset": ("FLOAT", dict(offset, tooltip="added to the base colour, in units of the full range")),
            "edit_roughness_offset": ("FLOAT", dict(offset, tooltip="added to the roughness, in units of the full range")),
            "edit_metallic_offset": ("FLOAT", dict(offset, tooltip="added to the metallic map, in units of the full range")),
            "insert_mask": ("MASK", {"tooltip": "the inserted object's matte (1 = the object, 0 = the scene); required with any "
                                                "insert_* layer.  The object's G-buffers are composited into the scene's under it "
                                                "and both are lit together; inserted normals are renormalised"}),
            "insert_base_color": ("IMAGE", {"tooltip": layer.format("base colour")}),
            "insert_metallic": ("IMAGE", {"tooltip": layer.format("metallic map")}),
            "insert_roughness": ("IMAGE", {"tooltip": layer.format("roughness")}),
            "insert_normal": ("IMAGE", {"tooltip": layer.format("normal map")}),
            "insert_depth": ("IMAGE", {"tooltip": layer.format("depth")})}


def _fit_inputs():
    """Optional inputs of both renderers for clips off the model's grid (fit.py)."""
    return {"fit": (["off", "crop", "stretch"],
                    {"default": "off",
                     "tooltip": "off: the clip must already be T = 8k+1 frames of H, W multiples of 16.  crop: resize (antialiased) "
                                "to cover the target size, then centre-crop; stretch: resize the whole picture to it.  Short clips "
                                "repeat their last frame up to the next 8k+1 and come back at their own length.  The outputs keep "
                                "the model's size: they are not resampled back (a crop cannot be undone)"}),
            "fit_height": ("INT", {"default": 0, "min": 0, "max": 4096, "step": 16,
                                   "tooltip": "target height, a multiple of 16; 0 = the source height rounded down to one "
                                              "(with fit_width 0 too, crop is a pure centre crop)"}),
            "fit_width": ("INT", {"default": 0, "min": 0, "max": 4096, "step": 16,
                                  "tooltip": "target width, a multiple of 16; 0 = the source width rounded down to one"}),
            "fit_restore": ("BOOLEAN", {"default": False,
                                        "tooltip": "return the outputs at the source size: they are resampled back (antialiased) "
                                                   "on the GPU.  Only works with a fit that kept the whole picture: stretch, or a "
                                                   "crop that cut nothing; any other crop is refused.  Ignored with fit off.  "
                                                   "Normal maps are resampled like any picture and not renormalised"})}


def _guide_inputs():
    """Optional inputs of the nodes that hold the source picture, for the guided way back (fit.py)."""
    return {"restore_guide": (["off", "source"],
                              {"default": "off",
                               "tooltip": "source: fit_restore brings the outputs back with the full-size input picture as a guide "
                                          "(joint bilateral upsampling): edges of the outputs land where the picture's edges are "
                                          "instead of on a ramp 2-4 pixels wide.  Ignored unless fit is on and fit_restore is set"}),
            "restore_sigma": ("FLOAT", {"default": 12.0, "min": 1.0, "max": 64.0, "step": 0.5,
                                        "tooltip": "how close in colour (levels of 255, per channel, Gaussian) a low-resolution "
                                                   "pixel's source must be to the full-size pixel to count; larger = closer to the "
                                                   "plain fit_restore"})}


def standardize_to_5d(image, name="image") -> torch.Tensor:
    """list / (H,W,C) / (B,H,W,C)->T=1 / (B,T,H,W,C) -> (B,T,H,W,C)   (reference nodes.py:156-177, :258-268)."""
    if isinstance(image, list):
        try:
            return torch.stack(image, dim=0)
        except Exception:
            return image[0].unsqueeze(0)
    if isinstance(image, torch.Tensor):
        if image.ndim == 3:
            return image.unsqueeze(0).unsqueeze(0)
        if image.ndim == 4:
            return image.unsqueeze(1)
        if image.ndim == 5:
            return image
        raise ValueError(f"Unsupported tensor dimension for '{name}': {image.ndim}. Expected 3D, 4D, or 5D.")
    raise TypeError(f"Unsupported input type for '{name}': {type(image)}. Expected torch.Tensor or list of Tensors.")


def _configure(pipeline, model_type, guidance, seed, window_frames, window_overlap, tiles=(0, 0, 64), tile_join="pixel",
               window_align=False, sampler="euler", steps=0, ensemble=1, ensemble_reduce="median", step_cache=0.0,
               ensemble_align=False):
    """What both renderers set on the pipeline before a run; the restore plan of an earlier run is cleared.  tiles:
    (tile_height, tile_width, tile_overlap); tile_join: how they are joined ("pixel" / "latent"); window_align: windows matched
    in gain and offset over the overlap (refused here, before any upload, without an overlap or with tiles); sampler: the
    denoising loop's (refused here where it is unknown, or not "euler" with tile_join = "latent"); steps: the pipeline's
    num_steps, 0 = left as it is; ensemble, ensemble_reduce: the seed ensemble (refused here where it is no integer in 1..16 or the
    reduce is unknown; the forward renderer is always handed 1: averaged renders blur); step_cache: the step cache's threshold,
    0 = off (refused here outside [0, 1], or > 0 with tile_join = "latent"); ensemble_align: the ensemble's members matched in gain
    and offset before the reduce (refused here where it is no bool; the forward renderer is always handed False)."""
    check_window_align(window_align, window_frames, window_overlap, tiles[0], tiles[1])
    check_sampler(sampler, tile_join)
    check_step_cache(step_cache, tile_join=tile_join)
    if isinstance(ensemble, np.integer):
        ensemble = int(ensemble)
    if isinstance(ensemble_align, np.bool_):
        ensemble_align = bool(ensemble_align)
    check_ensemble(ensemble, ensemble_reduce, ensemble_align=ensemble_align)
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 0:
        raise ValueError(f"steps must be a non-negative integer (0 = the pipeline's own), got {steps!r}")
    pipeline.set_model_type(model_type)
    pipeline.guidance = guidance
    pipeline.seed = seed
    pipeline.window_frames = window_frames
    pipeline.window_overlap = window_overlap
    pipeline.window_align = bool(window_align)
    pipeline.tile_height, pipeline.tile_width, pipeline.tile_overlap = tiles
    pipeline.tile_join = tile_join
    pipeline.sampler = sampler
    pipeline.step_cache = float(step_cache)
    pipeline.ensemble = ensemble
    pipeline.ensemble_reduce = ensemble_reduce
    pipeline.ensemble_align = ensemble_align
    if steps:
        pipeline.num_steps = int(steps)
    pipeline.restore_plan = None
    pipeline.restore_guide = None


def _source_guide(pipeline, image, fit, fit_height, fit_width, fit_restore, window_frames, restore_guide, restore_sigma):
    """The source clip as the guide of the way back (fit.source_guide, on the pipeline's device), or None where `restore_guide`
    is off or ignored: fit off, or fit_restore off."""
    if restore_guide not in ("off", "source"):
        raise ValueError(f"restore_guide must be 'off' or 'source', got {restore_guide!r}")
    if restore_guide == "off" or fit == "off" or not fit_restore:
        return None
    from .fit import plan_fit, source_guide
    t5 = standardize_to_5d(image)
    T, H, W = t5.shape[1:4]
    plan = plan_fit(T, H, W, fit, fit_height, fit_width, windowed=window_frames > 0 and T > window_frames)
    return source_guide(plan, t5, restore_sigma, getattr(pipeline, "device", "cuda"))


def _ingest(pipeline, clips, fit, fit_height, fit_width, fit_restore, window_frames):
    """{name: frames in [0, 1]} -> ({name: (B,C,T,H,W) in [-1, 1]}, the fit's plan).  fit off: no plan, the clips must be on the
    model's grid.  Otherwise all clips go through ONE plan (fit.py: resize / crop / pad in time, * 2 - 1, bf16 and the transpose in
    one launch on the pipeline's device), so they must be one size; with fit_restore the pipeline is handed the way back
    (ValueError for a crop that cut, before anything runs).  A uint8 clip (a byte i standing for i / 255) always goes through
    fit_frames, which uploads the bytes: with fit off under the identity plan, so it must be on the grid in H and W like any clip
    (a T off 8k+1 is refused downstream, as for fp32), and arrives as the device bf16 tensor the fp32 clip u8 / 255 becomes."""
    from .fit import fit_frames, plan_fit, plan_restore
    clips = {name: standardize_to_5d(t, name) for name, t in clips.items()}
    device = getattr(pipeline, "device", "cuda")
    if fit == "off":
        out = {}
        for name, t5 in clips.items():
            if t5.dtype != torch.uint8:
                out[name] = t5.permute(0, 4, 1, 2, 3) * 2.0 - 1.0
                continue
            same = plan_fit(*t5.shape[1:4], "crop", 0, 0, windowed=True)
            if not same.identity:
                raise ValueError(f"'{name}' is uint8 frames of (H, W) = {tuple(t5.shape[2:4])}, off the model's grid of 16: "
                                 "set fit = 'crop' or 'stretch' (with fit off a clip is taken as it is)")
            out[name] = fit_frames(t5, same, device=device)
        return out, None
    first, shape = next((name, tuple(t5.shape[1:4])) for name, t5 in clips.items())
    for name, t5 in clips.items():
        if tuple(t5.shape[1:4]) != shape:
            raise ValueError(f"fit needs G-buffers of one size: '{name}' is (T, H, W) = {tuple(t5.shape[1:4])}, "
                             f"'{first}' is {shape}")
    plan = plan_fit(*shape, fit, fit_height, fit_width, windowed=window_frames > 0 and shape[0] > window_frames)
    if fit_restore:
        pipeline.restore_plan = plan_restore(plan)      # the outputs come back at the source's size
    return {name: fit_frames(t5, plan, device=device) for name, t5 in clips.items()}, plan


def _inverse_passes(pipeline, image, guidance, seed, window_frames, window_overlap, fit, fit_height, fit_width, fit_restore,
                    to_host=True, tiles=(0, 0, 64), tile_join="pixel", restore_guide="off", restore_sigma=12.0,
                    window_align=False, sampler="euler", steps=0, ensemble=1, ensemble_reduce="median", step_cache=0.0,
                    ensemble_align=False):
    """The inverse renderer up to the pipeline's outputs -> (the five uint8 results in INVERSE_PASSES order - an iterable, rendered
    as it is walked where the passes run one by one -, the frames to keep or None, the fit's plan or None).  to_host=False: the
    results are device tensors (the pipeline's `to_host`)."""
    _configure(pipeline, "inverse", guidance, seed, window_frames, window_overlap, tiles, tile_join, window_align, sampler, steps,
               ensemble, ensemble_reduce, step_cache, ensemble_align)
    clips, plan = _ingest(pipeline, {"image": image}, fit, fit_height, fit_width, fit_restore, window_frames)
    guide = _source_guide(pipeline, image, fit, fit_height, fit_width, fit_restore, window_frames, restore_guide, restore_sigma)
    if guide is not None:
        pipeline.restore_guide = guide                  # the way back is guided by the source picture
    image_tensor = clips["image"]
    keep = plan.T if plan is not None else None
    kw = {} if to_host else {"to_host": False}
    normalize = [p == "normal" for p in INVERSE_PASSES]
    if image_tensor.shape[0] == 1 and getattr(pipeline, "batch_passes", True) and hasattr(pipeline, "generate_video_passes"):
        # the five passes share the clip, the seed and every weight: step them as one batch
        data_batch = {
            "rgb": image_tensor,
            "video": image_tensor,
            "context_index": torch.tensor([[GBUFFER_INDEX_MAPPING[p]] for p in INVERSE_PASSES], dtype=torch.long),
        }
        outs = pipeline.generate_video_passes(data_batch=data_batch, seed=seed, normalize_normal=normalize, **kw)
    else:
        batches = [{"rgb": image_tensor,
                    "video": image_tensor,
                    "context_index": torch.full((image_tensor.shape[0], 1), GBUFFER_INDEX_MAPPING[p], dtype=torch.long)}
                   for p in INVERSE_PASSES]
        if window_frames and hasattr(pipeline, "generate_video_each"):
            # windows outside, passes inside: every window of the clip is uploaded and encoded once, not once per pass
            outs = pipeline.generate_video_each(batches, normalize, seed=seed, **kw)
        else:       # pass by pass, each rendered as the loop below asks for it: the progress bar moves per pass
            outs = (pipeline.generate_video(data_batch=b, normalize_normal=f, seed=seed, **kw) for b, f in zip(batches, normalize))
    return outs, keep, plan


def _forward_pass(pipeline, inputs, env_map, guidance, seed, env_format, env_brightness, env_flip_horizontal, env_rotation,
                  env_spin, window_frames, window_overlap, fit, fit_height, fit_width, fit_restore, restore_plan=None,
                  tiles=(0, 0, 64), tile_join="pixel", restore_guide=None, env_sequence=False, window_align=False,
                  sampler="euler", steps=0, step_cache=0.0):
    """The forward renderer on the five G-buffers `inputs` (depth, normal, roughness, metallic, base_color) -> the image
    (B,T,H,W,C) in [0, 1].  restore_plan: a way back that is not this fit's own (the relight node: the inverse stage's fit);
    restore_guide: its guide (a fit.RestoreGuide), or None for the plain way back.  env_sequence: frame t is lit by frame t of
    env_map, which then holds one frame per frame of the clip as handed in (or a single one)."""
    _configure(pipeline, "forward", guidance, seed, window_frames, window_overlap, tiles, tile_join, window_align, sampler, steps,
               step_cache=step_cache)
    key_mapping = {"base_color": "basecolor", "depth": "depth", "normal": "normal", "roughness": "roughness",
                   "metallic": "metallic"}
    # with a fit, all five G-buffers go through ONE plan: they must be the same clip geometry
    clips, plan = _ingest(pipeline, inputs, fit, fit_height, fit_width, fit_restore, window_frames)
    if restore_plan is not None:
        pipeline.restore_plan = restore_plan
        pipeline.restore_guide = restore_guide
    data_batch = {key_mapping[name]: t for name, t in clips.items()}
    keep = None
    if plan is not None:
        keep = plan.T
        # frame t keeps the angle radians(env_spin) * t / T of the clip as handed in; padded frames turn on and are cut away
        env_spin = env_spin * plan.T_out / plan.T
    B, _, T, H, W = data_batch["depth"].shape
    data_batch["video"] = data_batch["depth"]
    # env-map conditions (env_ldr / env_log / env_nrm): preprocessing outside the denoise loop (reference :283-304); env_spin
    # degrees turn the light about +Y over the clip (every frame projected on the GPU by drn_env_project), 0 = static.
    # Built for the WHOLE clip and the WHOLE picture also when it is rendered in windows or tiles: the pipeline cuts them per
    # window and crops them per tile like the G-buffers (they are per-pixel view-direction images).  A light sequence is checked
    # against the clip's own frame count; over frames the fit padded, its last light repeats and is cut away with them
    from . import preprocess_envmap as pe
    env = pe.envmap_conditions(env_map, (H, W), T, env_format, env_brightness, env_flip_horizontal, env_rotation,
                               device=getattr(pipeline, "device", "cuda"), env_spin=env_spin, env_sequence=env_sequence,
                               clip_frames=T if keep is None else keep)
    data_batch["env_ldr"] = env["env_ldr"].expand(B, -1, -1, -1, -1)
    data_batch["env_log"] = env["env_log"].expand(B, -1, -1, -1, -1)
    data_batch["env_nrm"] = env["env_nrm"].expand(B, -1, T, -1, -1)
    out = pipeline.generate_video(data_batch=data_batch, seed=seed)
    return torch.from_numpy(out[:, :keep]).float() / 255.0


class LoadDiffusionRendererModel:
    @classmethod
    def INPUT_TYPES(s):
        import folder_paths
        return {"required": {"model": (folder_paths.get_filename_list("diffusion_models"),
                                       {"tooltip": "Models are loaded from 'ComfyUI/models/diffusion_models'"})},
                "optional": {"dit_precision": (["bf16", "mxfp8"],
                                               {"default": "bf16",
                                                "tooltip": "mxfp8: opt-in MXFP8 block linears (faster, ~4x the bf16 error)"}),
                             "attention_precision": (["bf16", "mxfp8"],
                                                     {"default": "bf16",
                                                      "tooltip": "mxfp8: opt-in MXFP8 self-attention (Q, K, V and P as e4m3; "
                                                                 "costs accuracy, see DESIGN 4c)"})}}

    RETURN_TYPES = ("DIFFUSION_RENDERER_PIPELINE",)
    FUNCTION = "load_pipeline"
    CATEGORY = "Cosmos1"

    def load_pipeline(self, model, dit_precision="bf16", attention_precision="bf16"):
        import folder_paths
        import comfy.model_management as mm
        import comfy.utils
        from .CleanVAE import CleanVAE

        device = mm.get_torch_device()
        dtype = torch.bfloat16
        vae_dir = os.path.join(folder_paths.models_dir, "vae", "Cosmos-1.0-Tokenizer-CV8x8x8", "vae")
        if not os.path.isdir(vae_dir):
            raise FileNotFoundError(f"Image VAE subfolder not found at: {vae_dir}")
        vae_instance = CleanVAE(model_path=vae_dir)
        vae_instance.to(device)
        vae_instance.reset_dtype(dtype)

        checkpoint_path = folder_paths.get_full_path("diffusion_models", model)
        state_dict = comfy.utils.load_torch_file(checkpoint_path, safe_load=True)
        if "model" in state_dict:
            state_dict = state_dict["model"]
        model_instance = CleanDiffusionRendererModel(dict(get_inverse_renderer_config(), dit_precision=dit_precision,
                                                              dit_attention_precision=attention_precision), device=device)
        model_instance.load_state_dict(state_dict, strict=True)     # repack to the HIP layouts, weights stay on GPU
        del state_dict
        mm.soft_empty_cache()
        pipeline = CleanDiffusionRendererPipeline(
            checkpoint_dir=os.path.dirname(checkpoint_path), checkpoint_name=os.path.basename(checkpoint_path),
            model_type=None, vae_instance=vae_instance, model_instance=model_instance,
            guidance=0.0, num_steps=15, seed=42)
        return (pipeline,)


class Cosmos1InverseRenderer:
    @classmethod
    def INPUT_TYPES(s):
        return {
            "required": {"pipeline": ("DIFFUSION_RENDERER_PIPELINE",), "image": ("IMAGE",)},
            "optional": {"guidance": ("FLOAT", {"default": 0.0, "min": 0.0, "max": 10.0, "step": 0.1}),
                         "seed": ("INT", {"default": 42, "min": 0, "max": 0xffffffffffffffff}),
                         **_window_inputs(), **_fit_inputs(), **_tile_inputs(), **_guide_inputs(), **_sampler_inputs(),
                         **_ensemble_inputs()},
        }

    RETURN_TYPES = ("IMAGE", "IMAGE", "IMAGE", "IMAGE", "IMAGE")
    RETURN_NAMES = ("base_color", "metallic", "roughness", "normal", "depth")
    FUNCTION = "run_inverse_pass"
    CATEGORY = "Cosmos1"

    def run_inverse_pass(self, pipeline, image, guidance=0.0, seed=42, window_frames=0, window_overlap=8,
                         fit="off", fit_height=0, fit_width=0, fit_restore=False, tile_height=0, tile_width=0, tile_overlap=64,
                         tile_join="pixel", restore_guide="off", restore_sigma=12.0, window_align=False, sampler="euler", steps=0,
                         ensemble=1, ensemble_reduce="median", step_cache=0.0, ensemble_align=False):
        outs, keep, _ = _inverse_passes(pipeline, image, guidance, seed, window_frames, window_overlap, fit, fit_height, fit_width,
                                        fit_restore, tiles=(tile_height, tile_width, tile_overlap), tile_join=tile_join,
                                        restore_guide=restore_guide, restore_sigma=restore_sigma, window_align=window_align,
                                        sampler=sampler, steps=steps, ensemble=ensemble, ensemble_reduce=ensemble_reduce,
                                        step_cache=step_cache, ensemble_align=ensemble_align)
        images = []
        pbar = _progress_bar(len(INVERSE_PASSES))
        for out in outs:                                                      # in INVERSE_PASSES order = RETURN_NAMES order
            t = torch.from_numpy(out[:, :keep]).float() / 255.0               # a clip padded in time comes back at its own length
            b, tt, h, w, c = t.shape
            images.append(t.reshape(b * tt, h, w, c))
            pbar.update(1)
        return tuple(images)


_ENV_SEQUENCE_TOOLTIP = ("env_map is a light that changes over the clip: frame t is lit by frame t of env_map, which must hold "
                         "one frame per frame of the clip (or a single one). Off: only its first frame is used")


class Cosmos1ForwardRenderer:
    @classmethod
    def INPUT_TYPES(s):
        return {
            "required": {"pipeline": ("DIFFUSION_RENDERER_PIPELINE",), "depth": ("IMAGE",), "normal": ("IMAGE",),
                         "roughness": ("IMAGE",), "metallic": ("IMAGE",), "base_color": ("IMAGE",), "env_map": ("IMAGE",)},
            "optional": {"guidance": ("FLOAT", {"default": 0.0, "min": 0.0, "max": 2.0, "step": 0.1}),
                         "seed": ("INT", {"default": 42, "min": 0, "max": 0xffffffffffffffff}),
                         "env_format": (["proj", "ball"], {"default": "proj"}),
                         "env_brightness": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 2.0, "step": 0.1}),
                         "env_flip_horizontal": ("BOOLEAN", {"default": False}),
                         "env_rotation": ("FLOAT", {"default": 180.0, "min": 0, "max": 360, "step": 1.0}),
                         "env_spin": ("FLOAT", {"default": 0.0, "min": -720.0, "max": 720.0, "step": 1.0}),
                         "env_sequence": ("BOOLEAN", {"default": False, "tooltip": _ENV_SEQUENCE_TOOLTIP}),
                         **_window_inputs(), **_fit_inputs(), **_tile_inputs(), **_sampler_inputs()},
        }

    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "run_forward_pass"
    CATEGORY = "Cosmos1"

    def run_forward_pass(self, pipeline, depth, normal, roughness, metallic, base_color, env_map, guidance=0.0, seed=42,
                         env_format="proj", env_brightness=1.0, env_flip_horizontal=False, env_rotation=0.0,
                         env_spin=0.0, window_frames=0, window_overlap=8, fit="off", fit_height=0, fit_width=0,
                         fit_restore=False, tile_height=0, tile_width=0, tile_overlap=64, tile_join="pixel", env_sequence=False,
                         window_align=False, sampler="euler", steps=0, step_cache=0.0):
        inputs = {"depth": depth, "normal": normal, "roughness": roughness, "metallic": metallic, "base_color": base_color}
        return (_forward_pass(pipeline, inputs, env_map, guidance, seed, env_format, env_brightness, env_flip_horizontal,
                              env_rotation, env_spin, window_frames, window_overlap, fit, fit_height, fit_width, fit_restore,
                              tiles=(tile_height, tile_width, tile_overlap), tile_join=tile_join, env_sequence=env_sequence,
                              window_align=window_align, sampler=sampler, steps=steps, step_cache=step_cache),)


class LoadHDRImage:
    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"path": ("STRING", {"tooltip": "Path to HDR image (.hdr, .exr)"})}}

    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "load_hdr"
    CATEGORY = "Cosmos1"

    def load_hdr(self, path):
        import imageio
        img = imageio.imread(path, format="HDR-FI")
        if img.ndim == 2:
            img = np.stack([img] * 3, axis=-1)
        elif img.ndim == 3 and img.shape[2] == 1:
            img = np.repeat(img, 3, axis=2)
        return (torch.from_numpy(img).float().unsqueeze(0),)


class Cosmos1Relight:
    """Video -> G-buffers -> the same video under a new environment light, in one call: the inverse renderer, then the forward
    renderer on its G-buffers, which stay on the device as the bytes the post-process wrote (drn_fit_frames_u8 ingests them).
    The bits are those of the two nodes chained through the host.  Not one of the reference's nodes: registered only with
    DRN_EXTRA_NODES=1 (below)."""

    @classmethod
    def INPUT_TYPES(s):
        return {
            "required": {"inverse_pipeline": ("DIFFUSION_RENDERER_PIPELINE",), "forward_pipeline": ("DIFFUSION_RENDERER_PIPELINE",),
                         "image": ("IMAGE",), "env_map": ("IMAGE",)},
            "optional": {"guidance": ("FLOAT", {"default": 0.0, "min": 0.0, "max": 10.0, "step": 0.1,
                                                "tooltip": "guidance of the inverse stage"}),
                         "forward_guidance": ("FLOAT", {"default": 0.0, "min": 0.0, "max": 2.0, "step": 0.1}),
                         "seed": ("INT", {"default": 42, "min": 0, "max": 0xffffffffffffffff}),
                         "env_format": (["proj", "ball"], {"default": "proj"}),
                         "env_brightness": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 2.0, "step": 0.1}),
                         "env_flip_horizontal": ("BOOLEAN", {"default": False}),
                         "env_rotation": ("FLOAT", {"default": 180.0, "min": 0, "max": 360, "step": 1.0}),
                         "env_spin": ("FLOAT", {"default": 0.0, "min": -720.0, "max": 720.0, "step": 1.0}),
                         "env_sequence": ("BOOLEAN", {"default": False, "tooltip": _ENV_SEQUENCE_TOOLTIP}),
                         **_window_inputs(), **_fit_inputs(), **_tile_inputs(), **_guide_inputs(), **_sampler_inputs(),
                         **_ensemble_inputs(), **_edit_inputs()},
        }

    RETURN_TYPES = ("IMAGE", "IMAGE", "IMAGE", "IMAGE", "IMAGE", "IMAGE")
    RETURN_NAMES = ("image", "base_color", "metallic", "roughness", "normal", "depth")
    FUNCTION = "run_relight"
    CATEGORY = "Cosmos1"

    def run_relight(self, inverse_pipeline, forward_pipeline, image, env_map, guidance=0.0, forward_guidance=0.0, seed=42,
                    env_format="proj", env_brightness=1.0, env_flip_horizontal=False, env_rotation=0.0, env_spin=0.0,
                    window_frames=0, window_overlap=8, fit="off", fit_height=0, fit_width=0, fit_restore=False,
                    tile_height=0, tile_width=0, tile_overlap=64, tile_join="pixel", restore_guide="off", restore_sigma=12.0,
                    env_sequence=False, window_align=False, sampler="euler", steps=0, ensemble=1, ensemble_reduce="median",
                    step_cache=0.0, ensemble_align=False, edit_mask=None, edit_base_color_tint=0xFFFFFF, edit_base_color_gain=1.0,
                    edit_roughness_gain=1.0, edit_metallic_gain=1.0, edit_base_color_offset=0.0, edit_roughness_offset=0.0,
                    edit_metallic_offset=0.0, insert_mask=None, insert_base_color=None, insert_metallic=None,
                    insert_roughness=None, insert_normal=None, insert_depth=None):
        """Tiles, and the way they are joined, window_align, the sampler, its steps and step_cache apply to both stages; ensemble,
        ensemble_reduce and ensemble_align to the inverse stage only (the forward stage always renders one sample: averaged renders blur).  The two pipelines may be one object that holds both checkpoints (model_instance = {"inverse": ..., "forward": ...}).
        restore_guide = 'source': the input picture guides the way back of all six outputs.
        edit_* / insert_*: the G-buffers are edited on the device between the two stages (gbuffer_edit.py: a gain and offset per
        material map under edit_mask, the inserted object's layers under insert_mask), on the joined full clip and picture, so
        windows, tiles, ensembles, samplers and the step cache compose untouched.  The G-buffers returned are the EDITED ones:
        what the image was rendered from.  With every edit input at its default nothing is built and the call is the one it was."""
        from .fit import plan_fit, plan_restore, restore_frames, restore_frames_guided
        from .gbuffer_edit import build_edit, check_edit, edit_gbuffers, fit_edit
        tiles = (tile_height, tile_width, tile_overlap)
        edit = build_edit(standardize_to_5d, edit_mask, edit_base_color_tint, edit_base_color_gain, edit_roughness_gain,
                          edit_metallic_gain, edit_base_color_offset, edit_roughness_offset, edit_metallic_offset, insert_mask,
                          insert_base_color, insert_metallic, insert_roughness, insert_normal, insert_depth,
                          clips=standardize_to_5d(image).shape[0])
        eplan = None
        if edit is not None:                    # refused from the settings and shapes alone, before any pipeline or GPU call
            B, T, H, W = standardize_to_5d(image).shape[:4]
            if fit != "off":
                eplan = plan_fit(T, H, W, fit, fit_height, fit_width, windowed=window_frames > 0 and T > window_frames)
            check_edit(edit, (B, T) + ((H, W) if eplan is None else (eplan.H_out, eplan.W_out)), source_hw=(H, W))
        rplan = None
        if fit != "off" and fit_restore:        # a crop that cut is refused before any GPU work, as the two nodes refuse it
            T, H, W = standardize_to_5d(image).shape[1:4]
            rplan = plan_restore(plan_fit(T, H, W, fit, fit_height, fit_width, windowed=window_frames > 0 and T > window_frames))
        guide = _source_guide(forward_pipeline, image, fit, fit_height, fit_width, fit_restore, window_frames, restore_guide,
                              restore_sigma)
        # 1. the inverse stage as the inverse node runs it, its outputs left at the model's size on the device, cut to the clip's T
        outs, keep, _ = _inverse_passes(inverse_pipeline, image, guidance, seed, window_frames, window_overlap, fit, fit_height,
                                        fit_width, False, to_host=False, tiles=tiles, tile_join=tile_join,
                                        window_align=window_align, sampler=sampler, steps=steps, ensemble=ensemble,
                                        ensemble_reduce=ensemble_reduce, step_cache=step_cache, ensemble_align=ensemble_align)
        gbuffers = [torch.as_tensor(o)[:, :keep] for o in outs]                # in INVERSE_PASSES order
        if edit is not None:                    # one pass over bytes that are already on the device
            gbuffers = edit_gbuffers(gbuffers, fit_edit(edit, eplan, gbuffers[0].device))
        # 2. + 3. the forward node on those bytes: fit 'crop' with no target is the identity in space (they are on the grid) and
        # pads time as the forward node would; the way back is the inverse fit's
        names = {"basecolor": "base_color"}
        inputs = {names.get(p, p): g for p, g in zip(INVERSE_PASSES, gbuffers)}
        inputs = {k: inputs[k] for k in ("depth", "normal", "roughness", "metallic", "base_color")}
        relit = _forward_pass(forward_pipeline, inputs, env_map, forward_guidance, seed, env_format, env_brightness,
                              env_flip_horizontal, env_rotation, env_spin, window_frames, window_overlap, "crop", 0, 0, False,
                              restore_plan=rplan, tiles=tiles, tile_join=tile_join, restore_guide=guide,
                              env_sequence=env_sequence, window_align=window_align, sampler=sampler, steps=steps,
                              step_cache=step_cache)
        # 4. the G-buffers as the inverse node returns them
        images = []
        for g in gbuffers:
            if guide is not None:
                g = restore_frames_guided(g, guide.plan, guide.hi.to(g.device), guide.lo.to(g.device))
            elif rplan is not None:
                g = restore_frames(g, rplan)
            t = g.cpu().float() / 255.0
            b, tt, h, w, c = t.shape
            images.append(t.reshape(b * tt, h, w, c))
        return (relit, *images)


NODE_CLASS_MAPPINGS = {
    "LoadDiffusionRendererModel": LoadDiffusionRendererModel,
    "Cosmos1InverseRenderer": Cosmos1InverseRenderer,
    "Cosmos1ForwardRenderer": Cosmos1ForwardRenderer,
    "LoadHDRImage": LoadHDRImage,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "LoadDiffusionRendererModel": "Load Diffusion Renderer Model",
    "Cosmos1InverseRenderer": "Cosmos1 Inverse Renderer",
    "Cosmos1ForwardRenderer": "Cosmos1 Forward Renderer",
    "LoadHDRImage": "Load HDR Image",
}

# nodes the reference does not have.  NODE_CLASS_MAPPINGS stays the reference's four entries (the drop-in surface); these join the
# exported mappings only when DRN_EXTRA_NODES=1 is set when this module is imported
EXTRA_NODE_CLASS_MAPPINGS = {"Cosmos1Relight": Cosmos1Relight}
EXTRA_NODE_DISPLAY_NAME_MAPPINGS = {"Cosmos1Relight": "Cosmos1 Relight"}

if os.environ.get("DRN_EXTRA_NODES") == "1":
    NODE_CLASS_MAPPINGS.update(EXTRA_NODE_CLASS_MAPPINGS)
    NODE_DISPLAY_NAME_MAPPINGS.update(EXTRA_NODE_DISPLAY_NAME_MAPPINGS)
