#!/usr/bin/env python3
"""Long clips (windows.py) at the headline size: what joining two windows costs, measured in one process with the variants
interleaved.  113 x 576 x 1024, windows of 57 frames, overlap 8, normal pass.

    python tools/winbench.py [--kernels-only] [--steps K] [--frames T] [--out FILE]

Kernel legs (device events, median of `--reps` runs after a warm-up, variants alternating inside every repetition), on a decoded
57-frame window in bf16 and the 8-frame carry of its predecessor:
  (a)  torch: the overlap cross-faded in place (fp32 a + w * (b - a), cast to bf16, copied into the window), then
       drn_postprocess_u8 over the window
  (b)  drn_postprocess_window_u8 on the same window - once writing all 57 frames (the last window of a clip: the same frames as
       (a)), once writing 49 (a middle window, whose last 8 frames are the carry and are not written)
  (c)  drn_postprocess_window_u8 without a ramp, all 57 frames: what drn_postprocess_u8 launches (one kernel serves both)
Pipeline leg (host clock around calls that end in the D2H copy): one windowed generate_video of the clip against the windows of
its plan cut from the clip and run as separate generate_video calls (windows off; the cuts are inside the timed region on both
sides) - the full 28-block network with synthetic weights, the HIP tokenizer, `--steps` Euler steps.  The separate calls produce
no joined clip; the difference is what the join costs or saves.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
N = pkg.native
dev = torch.device("cuda")
BF = torch.bfloat16
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def interleaved(variants, reps):
    """{name: fn} -> {name: (median ms, [ms])}; one warm-up of each, then `reps` rounds in which every variant runs once."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), v) for k, v in ms.items()}


def kernel_legs(H, W, Wf, Ov, reps):
    gen = torch.Generator(device="cuda").manual_seed(3)
    video = (torch.randn((1, 3, Wf, H, W), generator=gen, device=dev) * 0.6).to(BF)
    prev = (torch.randn((1, 3, Ov, H, W), generator=gen, device=dev) * 0.6).to(BF)
    w = torch.from_numpy(pkg.windows.ramp_weights(Ov)).to(dev)
    w5 = w.view(1, 1, Ov, 1, 1)
    work = video.clone()
    out_full = torch.empty((1, Wf, H, W, 3), dtype=torch.uint8, device=dev)
    out_mid = torch.empty((1, Wf - Ov, H, W, 3), dtype=torch.uint8, device=dev)

    def torch_lerp_then_old():
        a, b = prev.float(), video[:, :, :Ov].float()
        work[:, :, :Ov] = (a + w5 * (b - a)).to(BF)
        return N.postprocess_u8(work, True)

    variants = {
        "(a) torch lerp + drn_postprocess_u8, 57 frames": torch_lerp_then_old,
        "(b) drn_postprocess_window_u8, ramp, 57 frames written": lambda: N.postprocess_window_u8(video, prev, w, 0, 0, Wf, True, out=out_full),
        "(b) drn_postprocess_window_u8, ramp, 49 frames written": lambda: N.postprocess_window_u8(video, prev, w, 0, 0, Wf - Ov, True, out=out_mid),
        "(c) drn_postprocess_window_u8, no ramp, 57 frames": lambda: N.postprocess_window_u8(video, None, None, 0, 0, Wf, True, out=out_full),
        "(c) drn_postprocess_window_u8, no ramp, no normal blend": lambda: N.postprocess_window_u8(video, None, None, 0, 0, Wf, False, out=out_full),
    }
    # same bytes first: faster and different is not faster
    ref = torch_lerp_then_old()
    assert torch.equal(N.postprocess_window_u8(video, prev, w, 0, 0, Wf, True), ref)
    del ref
    px = Wf * H * W
    say(f"kernel legs: window [1,3,{Wf},{H},{W}] bf16 ({px * 6 / 2**20:.0f} MiB in, {px * 3 / 2**20:.0f} MiB out), carry {Ov} frames, "
        f"normal pass unless noted; device events, median of {reps}, variants alternating; outputs identical (checked)")
    for name, (med, runs) in interleaved(variants, reps).items():
        frames = Wf - Ov if "49" in name else Wf
        traffic = frames * H * W * 9 + (Ov * H * W * 6 if "ramp," in name or name.startswith("(a)") else 0)
        say(f"  {name:58s} median {med:7.3f} ms   min {min(runs):7.3f}  max {max(runs):7.3f}   "
            f"{traffic / med / 1e6:7.1f} GB/s of the bytes the join needs")


def pipeline_leg(T, H, W, Wf, Ov, steps, rounds):
    sw, cfgm = pkg.synthetic_weights, pkg.diffusion_renderer_config
    cfg = cfgm.get_inverse_renderer_config(H, W, Wf)
    model = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=dev)
    model.load_state_dict(sw.synth_state_dict(dict(cfg["net"]), BF, device=dev), strict=True)
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=dev), device=dev)
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=vae, model_instance=model, guidance=0.0, num_steps=steps,
        height=H, width=W, num_video_frames=Wf)
    p.set_model_type("inverse")
    clip = torch.rand((1, 3, T, H, W), generator=torch.Generator().manual_seed(5)) * 2.0 - 1.0
    ci = torch.full((1, 1), 3, dtype=torch.long)
    plan = pkg.windows.plan_windows(T, Wf, Ov)

    def windowed():
        p.window_frames, p.window_overlap = Wf, Ov
        return p.generate_video({"rgb": clip, "video": clip, "context_index": ci}, normalize_normal=True, seed=7)

    def separate():                 # what a user without windows does by hand: cut the clip, one call per piece, no join
        p.window_frames = 0
        outs = []
        for q in plan:
            c = clip[:, :, q.start:q.start + Wf].contiguous()
            outs.append(p.generate_video({"rgb": c, "video": c, "context_index": ci}, normalize_normal=True, seed=7))
        return outs

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    first = clip[:, :, :Wf].contiguous()
    p.generate_video({"rgb": first, "video": first, "context_index": ci}, normalize_normal=True, seed=7)   # warm-up: one window's shapes
    del first
    say(f"pipeline leg: inverse renderer, normal pass, {T} x {H} x {W}, windows of {Wf}, overlap {Ov} -> {len(plan)} windows "
        f"(starts {[q.start for q in plan]}, frames written {[q.write_hi - q.write_lo for q in plan]}); 28-block network, synthetic "
        f"weights, HIP tokenizer, {steps} Euler steps; host clock, D2H included, one warm-up window, rounds alternate")
    ts = {"windowed generate_video": [], "the windows as separate generate_video calls": []}
    for _ in range(rounds):
        t, joined = wall(windowed)
        ts["windowed generate_video"].append(t)
        t, pieces = wall(separate)
        ts["the windows as separate generate_video calls"].append(t)
    assert joined.shape == (1, T, H, W, 3)
    q0 = plan[0]
    assert (joined[:, :q0.write_hi] == pieces[0][:, :q0.write_hi]).all(), "window 0 of the joined clip is not the separate call's"
    for name, v in ts.items():
        say(f"  {name:46s} median {statistics.median(v):7.3f} s   runs {' '.join(f'{x:.3f}' for x in v)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--frames", type=int, default=113)
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--window-frames", type=int, default=57)
    ap.add_argument("--window-overlap", type=int, default=8)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("winbench needs the GPU: nothing here can be measured on a CPU")
    say(f"# tools/winbench.py on {torch.cuda.get_device_name(0)}")
    kernel_legs(a.height, a.width, a.window_frames, a.window_overlap, a.reps)
    if not a.kernels_only:
        pipeline_leg(a.frames, a.height, a.width, a.window_frames, a.window_overlap, a.steps, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
