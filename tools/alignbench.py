#!/usr/bin/env python3
"""`window_align` (windows.py, csrc/window_align.hip) at the headline size: what matching a window to its predecessor costs,
measured in one process with the variants interleaved.  57 x 576 x 1024 windows, overlap 8.

    python tools/alignbench.py [--kernels-only] [--steps K] [--frames T] [--out FILE]

Kernel legs, per pass (device events, median of `--reps` runs after a warm-up, variants alternating inside every repetition), on a
decoded 57-frame window in bf16 and the 8-frame carry of its predecessor, as a middle window (49 frames written, a carry handed on):
  (a)  the parent's calls: drn_postprocess_window_u8, then the carry copy video[:, :, 49:].contiguous()
  (b)  drn_window_align_affine alone (two launches: partials, solve)
  (c)  drn_postprocess_window_align_u8 alone, with the affine and the carry written by the same launch
  (d)  (b) + (c): what window_align runs per pass
  (e)  (c) with affine = NULL: the parent's bytes and the raw carry from the new kernel
Bytes needed over time stand beside the 6.3 TB/s the project's streaming kernels reach.
Pipeline leg (host clock around calls that end in the D2H copy): a windowed generate_video of 113 frames with window_align on
against off, medians of `--rounds` alternated rounds - the full 28-block network with synthetic weights, the HIP tokenizer,
`--steps` Euler steps, a base-colour pass (a normal pass is never aligned).
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
STREAM_TBS = 6.3


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
    prev = (video[:, :, :Ov].float() * 1.2 + 0.05 + 0.05 * torch.randn((1, 3, Ov, H, W), generator=gen, device=dev)).to(BF)
    w = torch.from_numpy(pkg.windows.ramp_weights(Ov)).to(dev)
    out = torch.empty((1, Wf - Ov, H, W, 3), dtype=torch.uint8, device=dev)
    carry = torch.empty((1, 3, Ov, H, W), dtype=BF, device=dev)
    affine = N.window_align_affine(video, prev, 0)

    def parent():
        N.postprocess_window_u8(video, prev, w, 0, 0, Wf - Ov, False, out=out)
        return video[:, :, Wf - Ov:].contiguous()

    def both():
        a = N.window_align_affine(video, prev, 0)
        N.postprocess_window_align_u8(video, prev, w, a, 0, 0, Wf - Ov, False, out=out, carry_out=carry)

    variants = {
        "(a) drn_postprocess_window_u8 + carry copy (the parent)": parent,
        "(b) drn_window_align_affine": lambda: N.window_align_affine(video, prev, 0),
        "(c) drn_postprocess_window_align_u8, affine, carry_out": lambda: N.postprocess_window_align_u8(
            video, prev, w, affine, 0, 0, Wf - Ov, False, out=out, carry_out=carry),
        "(d) (b) + (c): window_align per pass": both,
        "(e) drn_postprocess_window_align_u8, affine NULL, carry_out": lambda: N.postprocess_window_align_u8(
            video, prev, w, None, 0, 0, Wf - Ov, False, out=out, carry_out=carry),
    }
    # the same bytes first: (e) is the parent's output and the raw tail; the device's affine is the specification's
    ref = N.postprocess_window_u8(video, prev, w, 0, 0, Wf - Ov, False)
    got, tail = N.postprocess_window_align_u8(video, prev, w, None, 0, 0, Wf - Ov, False, carry_frames=Ov)
    assert torch.equal(got, ref) and torch.equal(tail, video[:, :, Wf - Ov:])
    del ref, got, tail
    say(f"the affine of this window: g = {float(affine[0, 0]):.6f}, o = {float(affine[0, 1]):.6f} (inputs: 1.2 x + 0.05 + noise)")
    px, ov = (Wf - Ov) * H * W, Ov * H * W
    read_overlap = 2 * ov * 6
    traffic = {"(a)": px * 9 + ov * 6 + 2 * ov * 6, "(b)": read_overlap, "(c)": px * 9 + ov * 6 + 2 * ov * 6,
               "(d)": read_overlap + px * 9 + ov * 6 + 2 * ov * 6, "(e)": px * 9 + ov * 6 + 2 * ov * 6}
    say(f"kernel legs: window [1,3,{Wf},{H},{W}] bf16, carry {Ov} frames, {Wf - Ov} frames written, no normal blend; the overlap read "
        f"is {read_overlap / 1e6:.1f} MB per pass; device events, median of {reps}, variants alternating")
    for name, (med, runs) in interleaved(variants, reps).items():
        need = traffic[name[:3]]
        say(f"  {name:62s} median {med * 1e3:8.1f} us   min {min(runs) * 1e3:8.1f}  max {max(runs) * 1e3:8.1f}   "
            f"{need / 1e6:7.1f} MB needed, {need / med / 1e9:5.2f} TB/s (streaming kernels: {STREAM_TBS} TB/s = "
            f"{need / STREAM_TBS / 1e6:6.1f} us)")


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
    p.window_frames, p.window_overlap = Wf, Ov
    clip = torch.rand((1, 3, T, H, W), generator=torch.Generator().manual_seed(5)) * 2.0 - 1.0
    ci = torch.full((1, 1), 0, dtype=torch.long)
    plan = pkg.windows.plan_windows(T, Wf, Ov)

    def run(align):
        p.window_align = align
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = p.generate_video({"rgb": clip, "video": clip, "context_index": ci}, normalize_normal=False, seed=7)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    first = clip[:, :, :Wf].contiguous()
    p.generate_video({"rgb": first, "video": first, "context_index": ci}, normalize_normal=False, seed=7)   # warm-up: one window
    del first
    say(f"pipeline leg: inverse renderer, base-colour pass, {T} x {H} x {W}, windows of {Wf}, overlap {Ov} -> {len(plan)} windows; "
        f"28-block network, synthetic weights, HIP tokenizer, {steps} Euler steps; host clock, D2H included, one warm-up window, "
        f"rounds alternate")
    ts = {"window_align off": [], "window_align on": []}
    for _ in range(rounds):
        t, off = run(False)
        ts["window_align off"].append(t)
        t, on = run(True)
        ts["window_align on"].append(t)
    q1 = plan[1]
    assert (on[:, :q1.out_at] == off[:, :q1.out_at]).all(), "window 0 is nobody's follower"
    for name, v in ts.items():
        say(f"  {name:20s} median {statistics.median(v):7.3f} s   runs {' '.join(f'{x:.3f}' for x in v)}")
    say(f"  bytes moved by the alignment: {int((on != off).sum())} of {on.size}")


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
        sys.exit("alignbench needs the GPU: nothing here can be measured on a CPU")
    say(f"# tools/alignbench.py on {torch.cuda.get_device_name(0)}")
    kernel_legs(a.height, a.width, a.window_frames, a.window_overlap, a.reps)
    if not a.kernels_only:
        pipeline_leg(a.frames, a.height, a.width, a.window_frames, a.window_overlap, a.steps, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
