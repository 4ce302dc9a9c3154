#!/usr/bin/env python3
"""Seed ensembles (ensemble.py) at the headline size: what the per-pixel reduce costs, and what an ensemble render
costs, measured in one process with the arms alternating.  Nothing was set in advance: the figures are recorded as they come.

    python tools/ensemblebench.py [--kernels-only] [--steps K] [--out profiles/ensemble.txt]
    python tools/ensemblebench.py --parity [--out profiles/ensemble_parity.txt]          (CPU: needs no GPU)

(a) Reduce leg (device events around the wrappers, median of `--reps` runs after a warm-up, arms alternating inside every
    repetition): one pass's reduce at uint8 57 x 576 x 1024 x 3 with N = 3, 5, 8 members, in every mode, without and with the
    spread - ensemble.reduce_members' torch path on the device (stack + sort, or the fp32 normal chain) against
    drn_ensemble_reduce_u8.  Per arm: time, peak device memory above the members, and the bytes the algorithm needs (N reads and
    one write per byte; two writes with the spread) over the kernel's time.
(b) Pipeline leg (host clock around calls that end in the D2H copy, `--rounds` rounds, arms alternating): generate_video_passes of
    the five inverse passes at ensemble = 3 against three separate calls (results left on the device) reduced by the torch path
    - the full 28-block network with synthetic weights, the HIP tokenizer, `--steps` steps.
--parity: the robustness figures of tests/ensemble_refs.py's synthetic scene (numpy reference, no GPU) and the count of bytes by
    which every wrong stand-in differs from the reference at its named case.
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
E = importlib.import_module(pkg.__name__ + ".ensemble")
BF = torch.bfloat16
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def parity():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ensemble_refs as R
    say("# tools/ensemblebench.py --parity (numpy reference of tests/ensemble_refs.py, CPU)")
    f = R.robustness_figures(5)
    say("robustness: synthetic scene 48 x 64, N = 5 members = truth + Gaussian noise (sigma 6 of 255) with 20 % salt outliers each")
    say("  colour, mean |byte error| against the truth: members " + ", ".join(f"{v:.3f}" for v in f["member_mae"])
        + f"; median {f['median_mae']:.3f}; mean {f['mean_mae']:.3f}")
    say("  normals, mean angular error against the truth: members " + ", ".join(f"{v:.3f}" for v in f["member_deg"])
        + f" deg; renormalised vector sum {f['normal_deg']:.3f} deg")
    say(f"  the median is below every member: {f['median_mae'] < min(f['member_mae'])}; the normal reduce is below every member: "
        f"{f['normal_deg'] < min(f['member_deg'])}  (the tests assert the inequalities and fix no number)")
    named = {name: (mode, mem) for name, mode, mem in R.cases(big=False) if name in set(R.WRONG.values())}
    say("wrong stand-ins against the reference at their named case of the grid (result bytes / spread bytes that differ):")
    for kind, case in R.WRONG.items():
        mode, mem = named[case]
        wr, wsp = R.reduce_ref(list(mem), mode, True)
        gr, gsp = R.wrong(kind, list(mem), mode, True)
        say(f"  {kind:28s} {case:18s} {int((gr != wr).sum()):6d} / {int((gsp != wsp).sum()):6d} of {wr.size}")
    n = sum(1 for _ in R.cases())
    say(f"grid: {n} cases; the torch specification equals the numpy reference on all of them (tests/test_ensemble_cpu.py)")


def reduce_leg(T, H, W, reps):
    dev = torch.device("cuda")
    gen = torch.Generator(device="cuda").manual_seed(3)
    shape = (1, T, H, W, 3)
    n = T * H * W * 3
    pool = [torch.randint(0, 256, shape, generator=gen, device=dev, dtype=torch.uint8) for _ in range(8)]
    say(f"reduce leg: members [1,{T},{H},{W},3] uint8 ({n / 2**20:.0f} MiB each); device events around reduce_members, median of "
        f"{reps} after a warm-up, arms alternating; peak = device memory above the members (result and spread included)")
    res = {}
    for N in (3, 5, 8):
        members = pool[:N]
        for mode in E.MODES:
            for spread in (False, True):
                outs = {b: E.reduce_members(members, mode, spread=spread, backend=b) for b in ("torch", "hip")}
                torch.cuda.synchronize()
                same = torch.equal(outs["torch"][0], outs["hip"][0]) and (not spread or torch.equal(outs["torch"][1], outs["hip"][1]))
                del outs
                ms, peak = {"torch": [], "hip": []}, {}
                for _ in range(reps):
                    for b in ms:
                        torch.cuda.synchronize()
                        base = torch.cuda.memory_allocated()
                        torch.cuda.reset_peak_memory_stats()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        out = E.reduce_members(members, mode, spread=spread, backend=b)
                        e1.record()
                        e1.synchronize()
                        ms[b].append(e0.elapsed_time(e1))
                        peak[b] = max(peak.get(b, 0), torch.cuda.max_memory_allocated() - base)
                        del out
                need = n * (N + (2 if spread else 1))
                mt, mh = statistics.median(ms["torch"]), statistics.median(ms["hip"])
                res[(N, mode, spread)] = (mt, mh)
                say(f"  N = {N}  {mode:6s} {'+ spread' if spread else '        '}  torch path {mt:8.3f} ms (min {min(ms['torch']):8.3f})  "
                    f"peak {peak['torch'] / 2**20:6.0f} MiB | kernel {mh:7.3f} ms (min {min(ms['hip']):7.3f})  peak "
                    f"{peak['hip'] / 2**20:5.0f} MiB  {need / mh / 1e9:5.2f} TB/s of the {need / 2**20:.0f} MiB it needs | "
                    f"{mt / mh:5.1f}x | same bytes: {same}")
    say("  (for scale: the streaming kernels of this project reach 6.3 TB/s; a yardstick, not a criterion.  The torch path's normal "
        "chain takes its square root in float64, which the specification needs on the CPU)")
    return res


def pipeline_leg(T, H, W, steps, rounds, N=3):
    dev = torch.device("cuda")
    sw, cfgm = pkg.synthetic_weights, pkg.diffusion_renderer_config
    cfg = cfgm.get_inverse_renderer_config(H, W, T)
    model = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=dev)
    model.load_state_dict(sw.synth_state_dict(dict(cfg["net"]), BF, device=dev), strict=True)
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=dev), device=dev)
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=vae, model_instance=model, guidance=0.0, num_steps=steps,
        height=H, width=W, num_video_frames=T)
    p.set_model_type("inverse")
    clip = torch.rand((1, 3, T, H, W), generator=torch.Generator().manual_seed(5)) * 2.0 - 1.0
    passes = ("basecolor", "metallic", "roughness", "normal", "depth")
    idx = {"basecolor": 0, "metallic": 1, "roughness": 2, "normal": 3, "depth": 4}
    batch = {"rgb": clip, "video": clip, "context_index": torch.tensor([[idx[k]] for k in passes], dtype=torch.long)}
    flags = [k == "normal" for k in passes]

    def ensemble():
        p.ensemble = N
        return p.generate_video_passes(batch, flags, seed=7)

    def separate():                 # what a user without `ensemble` does by hand: N calls, the results reduced with torch
        p.ensemble = 1
        members = [p.generate_video_passes(batch, flags, seed=7 + k, to_host=False) for k in range(N)]
        out = []
        for i, flag in enumerate(flags):
            r, _ = E.reduce_members([m[i] for m in members], "normal" if flag else "median", backend="torch")
            for m in members:
                m[i] = None
            out.append(r.cpu().numpy())
        return out

    def wall(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, torch.cuda.max_memory_allocated(), out

    p.ensemble = 1
    p.generate_video_passes(batch, flags, seed=7)                                  # warm-up: one member
    resident = torch.cuda.memory_allocated()
    say(f"pipeline leg: inverse renderer, five passes stepped together, {T} x {H} x {W}; 28-block network, synthetic weights, HIP "
        f"tokenizer, {steps} Euler steps; ensemble = {N}; host clock, D2H included, one warm-up member, rounds alternate")
    names = (f"generate_video_passes at ensemble = {N}", f"{N} separate calls, reduced by the torch path")
    ts, peaks = {k: [] for k in names}, {k: 0 for k in names}
    for r in range(rounds):
        t, pk, a = wall(ensemble)
        ts[names[0]].append(t)
        peaks[names[0]] = max(peaks[names[0]], pk - resident)
        t, pk, b = wall(separate)
        ts[names[1]].append(t)
        peaks[names[1]] = max(peaks[names[1]], pk - resident)
        if r == 0:
            assert all((x == y).all() for x, y in zip(a, b)), "the ensemble call is not the separate calls reduced by hand"
            say("  the ensemble call and the separate calls reduced by hand: identical bytes in all five passes (checked)")
        del a, b
        print(f"  (round {r + 1} of {rounds} done)", flush=True)
    for name, v in ts.items():
        say(f"  {name:52s} median {statistics.median(v):7.3f} s   runs {' '.join(f'{x:.3f}' for x in v)}   peak device memory above "
            f"what is resident {peaks[name] / 2**20:6.0f} MiB")
    one = T * H * W * 3
    say(f"  (one uint8 result is {one / 2**20:.0f} MiB; {N} members x 5 passes = {N * 5 * one / 2**20:.0f} MiB held while the members render)")
    p.ensemble = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parity", action="store_true", help="the robustness figures and the stand-in counts on the CPU; no timing")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--frames", type=int, default=57)
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.parity:
        parity()
    else:
        if not torch.cuda.is_available():
            sys.exit("ensemblebench needs the GPU for its timings (--parity runs on the CPU)")
        if a.rounds < 3 or a.reps < 3:
            sys.exit("medians of at least three rounds")
        say(f"# tools/ensemblebench.py on {torch.cuda.get_device_name(0)}; nothing was set in advance")
        reduce_leg(a.frames, a.height, a.width, a.reps)
        if not a.kernels_only:
            pipeline_leg(a.frames, a.height, a.width, a.steps, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
