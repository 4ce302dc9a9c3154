#!/usr/bin/env python3
"""Spatial tiles (tiles.py) at the headline size: what joining a tile costs, and what a tiled render costs, measured in one
process with the arms alternating.  57 x 1072 x 1920 in tiles of 576 x 1024 at overlap 64: 2 x 2 tiles.

    python tools/tilebench.py [--parity] [--kernels-only] [--steps K] [--out FILE]
    python tools/tilebench.py --join latent [--kernels-only] [--steps K] [--out profiles/latent_tiles.txt]

(a) Blend leg (device events, median of `--reps` runs after a warm-up, arms alternating inside every repetition): the last tile of
    the plan (rows from 16, columns from 64, both ramps) blended into the full canvas - tiles.blend_tile's torch path on the
    device against drn_tile_blend_u8.  Per arm: time, peak device memory above what is resident, and the bytes the join needs
    (the written rectangle read from the tile and written to the canvas, the ramp strips read from the canvas) over the time.
(b) Pipeline leg (host clock around calls that end in the D2H copy, `--rounds` rounds, arms alternating): one tiled
    generate_video of the clip against the four crops run as separate generate_video calls (tiles off, results left on the
    device) and joined by the torch path - the full 28-block network with synthetic weights, the HIP tokenizer, `--steps` steps.
(c) For scale: the same clip through fit = stretch to 576 x 1024 with the way back (fit_restore), one render.
--parity: only the checks that the arms agree byte for byte, at the same sizes, no timing.

--join latent replaces the legs above by those of the latent-space join, at the same sizes:
(d) Kernel leg: one tile's gather + step-join of one Euler step on the five-pass canvas - the torch device ops they replace
    (slice + contiguous + edm_scale_input + cat; cfg_combine + edm_step on contiguous crops + the blend on slices) against
    drn_latent_tile_gather + drn_latent_tile_step_join.  Per arm: time, aten ops / launches, peak memory above resident.
(e) Pipeline leg: the tiled generate_video with tile_join = "latent" against "pixel", rounds alternating; and one figure,
    recorded and not judged (synthetic weights cannot judge pictures): the mean absolute byte difference between two
    neighbouring tiles' own decoded results over the pixels they share, before the pixel join, for either setting.
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch
import torch.utils._python_dispatch

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


class _OpCount(torch.utils._python_dispatch.TorchDispatchMode):
    """Counts the aten ops issued under it: on device tensors each is at least one launch (views are none)."""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if not any(k in str(func) for k in ("view", "slice", "alias", "expand", "empty", "unsqueeze", "detach")):
            self.n += 1
        return func(*args, **(kwargs or {}))


def latent_kernel_leg(T, H, W, th, tw, Ov, reps, P=5, guidance=1.5):
    N = pkg.native
    plan = tiles.plan_tiles(H, W, th, tw, Ov)
    t = tiles.latent_tile(plan[-1], 8)
    F, Hc, Wc = (T - 1) // 8 + 1, H // 8, W // 8
    gen = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *shape: torch.randn(shape, generator=gen, device=dev, dtype=torch.float32).to(BF)
    cur, nxt0 = rnd(P, 16, F, Hc, Wc) * 3.0, rnd(P, 16, F, Hc, Wc) * 3.0
    out = rnd(2 * P, 16, F, t.h, t.w)
    c_in, c_skip, c_out, sigma, dt = 0.33, 0.027, 0.49, 3.0, -1.2
    wy, wx = (torch.from_numpy(pkg.windows.ramp_weights(O)).to(dev) for O in (t.Oy, t.Ox))

    def torch_arm(nxt):
        crop = cur[..., t.y:t.y + t.h, t.x:t.x + t.w].contiguous()
        xs = N.edm_scale_input(crop, c_in)
        both = torch.cat([xs, xs], 0)
        m = N.cfg_combine(out[:P].contiguous(), out[P:].contiguous(), guidance)
        b = N.edm_step(m, crop, c_skip, c_out, sigma, dt)
        dst = nxt[..., t.y + t.ry:t.y + t.h, t.x + t.rx:t.x + t.w]
        src = b[..., t.ry:, t.rx:].float()
        fy = torch.ones(t.h - t.ry, device=dev)
        fx = torch.ones(t.w - t.rx, device=dev)
        fy[:t.Oy], fx[:t.Ox] = wy, wx
        wgt = fy[:, None] * fx[None, :]
        a = dst.float()
        d = src - a
        dst.copy_(torch.where(wgt == 1.0, src, a + wgt * d).to(BF))
        return both

    def hip_arm(nxt):
        both = N.latent_tile_gather(cur, t.h, t.w, t.y, t.x, c_in, 2)
        N.latent_tile_step_join(out[:P], out[P:], guidance, cur, nxt, wy, wx, t.y, t.x, t.ry, t.rx, c_skip, c_out, sigma, dt)
        return both
    arms = {"torch": torch_arm, "hip": hip_arm}
    work = {k: nxt0.clone() for k in arms}
    ins = {k: fn(work[k]) for k, fn in arms.items()}
    torch.cuda.synchronize()
    assert torch.equal(ins["torch"].view(torch.int16), ins["hip"].view(torch.int16)), "the gather and the torch ops disagree"
    assert torch.equal(work["torch"].view(torch.int16), work["hip"].view(torch.int16)), "the step-join and the torch ops disagree"
    hh, ww = t.h - t.ry, t.w - t.rx
    planes = P * 16 * F
    need = 2 * planes * (3 * t.h * t.w + 4 * hh * ww + (t.Oy * ww + (hh - t.Oy) * t.Ox))
    say(f"kernel leg: canvas [{P},16,{F},{Hc},{Wc}] bf16 ({cur.numel() * 2 / 2**20:.0f} MiB), tile {tuple(t)}, CFG on: gather (2 copies) + "
        f"step-join; both arms leave identical DiT inputs and identical next canvases (checked); the two kernels need "
        f"{need / 2**20:.0f} MiB of traffic; device events, median of {reps}, arms alternating")
    ms, peak, ops = {k: [] for k in arms}, {}, {}
    for name, fn in arms.items():
        with _OpCount() as oc:
            fn(work[name])
        ops[name] = oc.n
    for _ in range(reps):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            both = fn(work[name])
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base - both.numel() * 2)
            del both
    for name, v in ms.items():
        label = "torch device ops + the three EDM kernels" if name == "torch" else "drn_latent_tile_gather + drn_latent_tile_step_join"
        say(f"  {label:52s} median {statistics.median(v):8.3f} ms   min {min(v):8.3f}  max {max(v):8.3f}   "
            f"{'aten ops and library launches' if name == 'torch' else 'launches'} {ops[name] if name == 'torch' else 2:3d}   "
            f"temporaries (peak above resident and the DiT input) {peak[name] / 2**20:6.0f} MiB")
    say("  (aten ops counted by a dispatch mode around the torch arm, views left out; its three library launches appear as none, "
        "so add 3)")


def latent_pipeline_leg(T, H, W, th, tw, Ov, steps, rounds):
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
    p.tile_height, p.tile_width, p.tile_overlap = th, tw, Ov
    mod = pkg.diffusion_renderer_pipeline
    real = mod.blend_tile
    seen = []

    def render(join, record=False):
        p.tile_join = join
        del seen[:]
        mod.blend_tile = (lambda c, o, q: (seen.append(o.clone()), real(c, o, q))[1]) if record else real
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = p.generate_video({"rgb": clip, "video": clip, "context_index": ci}, normalize_normal=True, seed=7)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out
        finally:
            mod.blend_tile = real

    def disagreement():
        """Mean absolute byte difference of horizontally and vertically neighbouring tiles over the pixels both decoded."""
        tot, n = 0.0, 0
        for i, a in enumerate(plan):
            for j, b in enumerate(plan):
                if j <= i or not ((a.y == b.y) != (a.x == b.x)):
                    continue
                y0, y1 = max(a.y, b.y), min(a.y + a.h, b.y + b.h)
                x0, x1 = max(a.x, b.x), min(a.x + a.w, b.x + b.w)
                if y1 <= y0 or x1 <= x0:
                    continue
                pa = seen[i][:, :, y0 - a.y:y1 - a.y, x0 - a.x:x1 - a.x].float()
                pb = seen[j][:, :, y0 - b.y:y1 - b.y, x0 - b.x:x1 - b.x].float()
                tot += float((pa - pb).abs().sum())
                n += pa.numel()
        return tot / n, n
    say(f"pipeline leg: inverse renderer, normal pass, {T} x {H} x {W} in tiles of {th} x {tw}, overlap {Ov} -> {len(plan)} tiles; "
        f"28-block network, synthetic weights, HIP tokenizer, {steps} Euler steps; host clock, D2H included; one warm-up render per "
        f"setting (the figure below is taken there), then {rounds} rounds alternating")
    figure = {}
    for join in ("pixel", "latent"):
        _, out = render(join, record=True)
        figure[join] = disagreement()
        assert out.shape == (1, T, H, W, 3)
        del out
    ts = {"pixel": [], "latent": []}
    for _ in range(rounds):
        for join in ts:
            t, out = render(join)
            ts[join].append(t)
            del out
    for join, v in ts.items():
        say(f"  tiled generate_video, tile_join = {join!r:9s} median {statistics.median(v):7.3f} s   runs {' '.join(f'{x:.3f}' for x in v)}")
    for join, (mad, n) in figure.items():
        say(f"  neighbouring tiles' own decoded results over their {n} shared bytes, before the pixel join, tile_join = {join!r:9s} "
            f"mean |difference| {mad:7.3f} of 255")
    say("  (recorded, not judged: with synthetic weights the network's output is not a picture; what the figure shows is whether "
        "the tiles' latents were pulled together, not whether a G-buffer looks right)")


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
    ap.add_argument("--join", choices=("pixel", "latent"), default="pixel", help="latent: the legs of the latent-space join")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tilebench needs the GPU: nothing here can be measured on a CPU")
    if a.rounds < 3 or a.reps < 3:
        sys.exit("medians of at least three rounds")
    say(f"# tools/tilebench.py on {torch.cuda.get_device_name(0)}" + (" (--parity)" if a.parity else ""))
    if a.join == "latent":
        say("# --join latent")
        latent_kernel_leg(a.frames, a.height, a.width, a.tile_height, a.tile_width, a.tile_overlap, a.reps)
        if not a.kernels_only:
            latent_pipeline_leg(a.frames, a.height, a.width, a.tile_height, a.tile_width, a.tile_overlap, a.steps, a.rounds)
    else:
        blend_leg(a.frames, a.height, a.width, a.tile_height, a.tile_width, a.tile_overlap, a.reps, a.parity)
    if a.join != "latent" and not a.kernels_only:
        pipeline_leg(a.frames, a.height, a.width, a.tile_height, a.tile_width, a.tile_overlap, a.steps, a.rounds, a.parity)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
