#!/usr/bin/env python3
"""Spatial tiles (tiles.py) at the headline size: what joining a tile costs, and what a tiled render costs, measured in one
process with the arms alternating.  57 x 1072 x 1920 in tiles of 576 x 1024 at overlap 64: 2 x 2 tiles.

    python tools/tilebench.py [--parity] [--kernels-only] [--steps K] [--out FILE]

(a) Blend leg (device events, median of `--reps` runs after a warm-up, arms alternating inside every repetition): the last tile of
    the plan (rows from 16, columns from 64, both ramps) blended into the full canvas - tiles.blend_tile's torch path on the
    device against drn_tile_blend_u8.  Per arm: time, peak device memory above what is resident, and the bytes the join needs
    (the written rectangle read from the tile and written to the canvas, the ramp strips read from the canvas) over the time.
(b) Pipeline leg (host clock around calls that end in the D2H copy, `--rounds` rounds, arms alternating): one tiled
    generate_video of the clip against the four crops run as separate generate_video calls (tiles off, results left on the
    device) and joined by the torch path - the full 28-block network with synthetic weights, the HIP tokenizer, `--steps` steps.
(c) For scale: the same clip through fit = stretch to 576 x 1024 with the way back (fit_restore), one render.
--parity: only the checks that the arms agree byte for byte, at the same sizes, no timing.
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
tiles = importlib.import_module(pkg.__name__ + ".tiles")
fit = importlib.import_module(pkg.__name__ + ".fit")
dev = torch.device("cuda")
BF = torch.bfloat16
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def blend_leg(T, H, W, th, tw, Ov, reps, parity):
    plan = tiles.plan_tiles(H, W, th, tw, Ov)
    t = plan[-1]
    gen = torch.Generator(device="cuda").manual_seed(3)
    canvas0 = torch.randint(0, 256, (1, T, H, W, 3), generator=gen, device=dev, dtype=torch.uint8)
    tile = torch.randint(0, 256, (1, T, t.h, t.w, 3), generator=gen, device=dev, dtype=torch.uint8)
    work = {"torch": canvas0.clone(), "hip": canvas0.clone()}
    # same bytes first: faster and different is not faster.  Every tile of the plan, in order, into one canvas per arm
    for q in plan:
        for name, c in work.items():
            tiles.blend_tile(c, tile, q, backend=name)
    torch.cuda.synchronize()
    assert torch.equal(work["torch"], work["hip"]), "the kernel and the torch path disagree"
    say(f"blend leg: canvas [1,{T},{H},{W},3] uint8 ({canvas0.numel() / 2**20:.0f} MiB), tile [1,{T},{t.h},{t.w},3] "
        f"({tile.numel() / 2**20:.0f} MiB), plan {len(plan)} tiles; all tiles blended by both arms: canvases identical (checked)")
    if parity:
        return None
    hh, ww = t.h - t.ry, t.w - t.rx
    ramp = t.Oy * ww + (hh - t.Oy) * t.Ox
    need = T * 3 * (2 * hh * ww + ramp)
    say(f"  timed: tile {tuple(t)} - written {hh} x {ww}, ramp strips {ramp} px per frame; the join needs {need / 2**20:.0f} MiB "
        f"of traffic; device events, median of {reps}, arms alternating")
    res = {}
    for name, c in work.items():
        tiles.blend_tile(c, tile, t, backend=name)
    torch.cuda.synchronize()
    ms = {k: [] for k in work}
    peak = {}
    for _ in range(reps):
        for name, c in work.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tiles.blend_tile(c, tile, t, backend=name)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base)
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = med
        say(f"  {'tiles.blend_tile, torch path on the device' if name == 'torch' else 'drn_tile_blend_u8':44s} median {med:8.3f} ms   "
            f"min {min(v):8.3f}  max {max(v):8.3f}   peak memory above resident {peak[name] / 2**20:7.0f} MiB   "
            f"{need / med / 1e9:6.3f} TB/s of the bytes the join needs")
    say("  (for scale: the streaming kernels of this project reach 6.3 TB/s; the blend is a strided walk over 960-pixel row pieces "
        "of a 1920-pixel canvas)")
    return res


def pipeline_leg(T, H, W, th, tw, Ov, steps, rounds, parity):
    sw, cfgm = pkg.synthetic_weights, pkg.diffusion_renderer_config
    cfg = cfgm.get_inverse_renderer_config(th, tw, T)
    model = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=dev)
    model.load_state_dict(sw.synth_state_dict(dict(cfg["net"]), BF, device=dev), strict=True)
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=dev), device=dev)
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=vae, model_instance=model, guidance=0.0, num_steps=steps,
        height=th, width=tw, num_video_frames=T)
    p.set_model_type("inverse")
    image = torch.rand((1, T, H, W, 3), generator=torch.Generator().manual_seed(5))
    clip = image.permute(0, 4, 1, 2, 3) * 2.0 - 1.0
    ci = torch.full((1, 1), 3, dtype=torch.long)
    plan = tiles.plan_tiles(H, W, th, tw, Ov)

    def tiled():
        p.tile_height, p.tile_width, p.tile_overlap = th, tw, Ov
        return p.generate_video({"rgb": clip, "video": clip, "context_index": ci}, normalize_normal=True, seed=7)

    def separate():                 # what a user without tiles does by hand: crop, one call per crop, join with torch
        p.tile_height = p.tile_width = 0
        canvas = None
        for q in plan:
            c = clip[..., q.y:q.y + q.h, q.x:q.x + q.w].contiguous()
            o = p.generate_video({"rgb": c, "video": c, "context_index": ci}, normalize_normal=True, seed=7, to_host=False)
            if canvas is None:
                canvas = torch.empty((1, o.shape[1], H, W, 3), dtype=torch.uint8, device=o.device)
            tiles.blend_tile(canvas, o, q, backend="torch")
        return canvas.cpu().numpy()

    def stretched():                # for scale: shrink to the model's size, render once, stretch the bytes back
        p.tile_height = p.tile_width = 0
        fplan = fit.plan_fit(T, H, W, "stretch", th, tw)
        small = fit.fit_frames(image, fplan, device=dev)
        p.restore_plan = fit.plan_restore(fplan)
        try:
            return p.generate_video({"rgb": small, "video": small, "context_index": ci}, normalize_normal=True, seed=7)
        finally:
            p.restore_plan = None

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    first = clip[..., :th, :tw].contiguous()
    p.generate_video({"rgb": first, "video": first, "context_index": ci}, normalize_normal=True, seed=7)   # warm-up: one tile's shapes
    del first
    say(f"pipeline leg: inverse renderer, normal pass, {T} x {H} x {W} in tiles of {th} x {tw}, overlap {Ov} -> {len(plan)} tiles "
        f"(corners {[(q.y, q.x) for q in plan]}, written from {[(q.ry, q.rx) for q in plan]}); 28-block network, synthetic "
        f"weights, HIP tokenizer, {steps} Euler steps; host clock, D2H included, one warm-up tile, rounds alternate")
    names = ("(b) tiled generate_video", "(b) the crops as separate calls, joined by the torch path",
             "(c) fit = stretch to the tile size, one render, fit_restore")
    ts = {n: [] for n in names}
    for r in range(1 if parity else rounds):
        t, joined = wall(tiled)
        ts[names[0]].append(t)
        t, by_hand = wall(separate)
        ts[names[1]].append(t)
        if r == 0:
            assert joined.shape == by_hand.shape == (1, T, H, W, 3)
            assert (joined == by_hand).all(), "the tiled call is not the crops joined by hand"
            say("  the tiled call and the crops joined by hand: identical bytes (checked)")
        del by_hand
        if not parity:
            t, small = wall(stretched)
            ts[names[2]].append(t)
            assert small.shape == (1, T, H, W, 3)
            del small
    if parity:
        return
    for name, v in ts.items():
        say(f"  {name:62s} median {statistics.median(v):7.3f} s   runs {' '.join(f'{x:.3f}' for x in v)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parity", action="store_true", help="only check that the arms agree byte for byte; no timing")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--frames", type=int, default=57)
    ap.add_argument("--height", type=int, default=1072)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--tile-height", type=int, default=576)
    ap.add_argument("--tile-width", type=int, default=1024)
    ap.add_argument("--tile-overlap", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tilebench needs the GPU: nothing here can be measured on a CPU")
    if a.rounds < 3 or a.reps < 3:
        sys.exit("medians of at least three rounds")
    say(f"# tools/tilebench.py on {torch.cuda.get_device_name(0)}" + (" (--parity)" if a.parity else ""))
    blend_leg(a.frames, a.height, a.width, a.tile_height, a.tile_width, a.tile_overlap, a.reps, a.parity)
    if not a.kernels_only:
        pipeline_leg(a.frames, a.height, a.width, a.tile_height, a.tile_width, a.tile_overlap, a.steps, a.rounds, a.parity)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
