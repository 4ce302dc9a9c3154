#!/usr/bin/env python3
"""Seed ensembles (ensemble.py) at the headline size: what the per-pixel reduce costs, and what an ensemble render
costs, measured in one process with the arms alternating.  Nothing was set in advance: the figures are recorded as they come.

    python tools/ensemblebench.py [--kernels-only] [--steps K] [--out profiles/ensemble.txt]
    python tools/ensemblebench.py --parity [--out profiles/ensemble_parity.txt]          (CPU: needs no GPU)
    python tools/ensemblebench.py --align [--out profiles/ensemble_align.txt]
    python tools/ensemblebench.py --align --parity [--out profiles/ensemble_align_parity.txt]   (CPU: needs no GPU)

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
--align: ensembles that agree at the same size with N = 3, 5, 8 members that differ in gain and offset: the solve
    (drn_ensemble_align_affine, its two launches together) against ensemble.align_members' torch path on the device, and the
    reduce through the affines (drn_ensemble_reduce_affine_u8) against today's reduce (drn_ensemble_reduce_u8, the parent's cost)
    and against the torch path with the affines.  With --parity: the robustness figures of tests/ensemble_align_refs.py's scene
    and the stand-in counts, on the CPU.
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


def align_parity():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ensemble_align_refs as A
    import numpy as np
    fmt = lambda v: ", ".join(f"{x:.3f}" for x in v)
    say("# tools/ensemblebench.py --align --parity (numpy reference of tests/ensemble_align_refs.py, CPU)")
    say("robustness: one picture with structure, 96 x 128 x 3, N = 5, member k = g_k truth + o_k + Gaussian noise (sigma 6 of 255) "
        "with 20 % of its bytes replaced by salt; mean |byte error| of the per-byte median against member 0's space")
    for title, kw in (("members at gains 1 / 0.7 / 1.3 / 0.85 / 1.15", {}), ("all gains 1 (nothing to align)",
                                                                            dict(gains=(1.0,) * 5, offsets=(0.0,) * 5))):
        f = A.robustness_figures(**kw)
        say(f"  {title}: today's median {f['unaligned']:.3f}; aligned by moment matching alone {f['moment']:.3f}; aligned by the "
            f"cross rule {f['cross']:.3f}")
        say(f"    gains: true {fmt(f['true_gains'])}; moment matching {fmt(f['moment_gains'])}; cross rule {fmt(f['cross_gains'])}")
    f = A.robustness_figures()
    say(f"  cross rule < moment matching < unaligned on the scene with gains: {f['cross'] < f['moment'] < f['unaligned']}  (the test "
        "asserts this inequality and fixes no number; the scene with all gains 1 is recorded, not judged)")
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    cases = {name: mem for name, mem in A.solve_cases()}
    say("wrong stand-ins of the solve against the reference at their named case (affine values / moments that differ):")
    for kind, case in A.SOLVE_WRONG.items():
        wa, ws = A.align_ref(cases[case])
        ga, gs = A.align_ref(cases[case], kind)
        say(f"  {kind:30s} {case:18s} {int((bits(ga) != bits(wa)).sum()):5d} / {int((gs != ws).sum()):5d}")
    rcases = {name: (mode, mem, aff) for name, mode, mem, aff in A.reduce_cases(big=False)}
    say("wrong stand-ins of the reduce behind an affine at their named case (result bytes / spread bytes that differ):")
    for kind, case in A.REDUCE_WRONG.items():
        mode, mem, aff = rcases[case]
        wr, wsp = A.reduce_affine_ref(mem, aff, mode, True)
        gr, gsp = A.reduce_affine_ref(mem, aff, mode, True, wrong=kind)
        say(f"  {kind:30s} {case:18s} {int((gr != wr).sum()):5d} / {int((gsp != wsp).sum()):5d} of {wr.size}")
    say(f"grids: {len(cases)} solve cases, {len(rcases) + 2} reduce cases; the specification equals the numpy reference on all of "
        "them (tests/test_ensemble_align_cpu.py)")


def align_leg(T, H, W, reps):
    dev = torch.device("cuda")
    gen = torch.Generator(device="cuda").manual_seed(4)
    shape = (1, T, H, W, 3)
    n = T * H * W * 3
    truth = torch.randint(40, 180, shape, generator=gen, device=dev, dtype=torch.uint8).float()
    pool = []
    for k in range(8):
        g, o = 1.0 + 0.08 * ((k * 5) % 7 - 3) * (k > 0), 6.0 * ((k * 3) % 5 - 2) * (k > 0)
        m = truth * g + o + 4.0 * torch.randn(shape, generator=gen, device=dev)
        pool.append(m.round().clamp(0, 255).to(torch.uint8))
        del m
    del truth
    say(f"align leg: members [1,{T},{H},{W},3] uint8 ({n / 2**20:.0f} MiB each) at gains and offsets of their own; device events "
        f"around the calls, median of {reps} after a warm-up, arms alternating; peak = device memory above the members")

    def timed(arms):
        ms, peak = {k: [] for k in arms}, {}
        for fn in arms.values():
            fn()
        for _ in range(reps):
            for k, fn in arms.items():
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
                peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated() - base)
                del out
        return {k: (statistics.median(v), min(v), peak[k]) for k, v in ms.items()}

    res = {}
    for N in (3, 5, 8):
        members = pool[:N]
        a_hip, a_torch = E.align_members(members, backend="hip"), E.align_members(members, backend="torch")
        same = torch.equal(a_hip, a_torch)
        t = timed({"hip": lambda: E.align_members(members, backend="hip"), "torch": lambda: E.align_members(members, backend="torch")})
        need = n * N
        (mh, lh, ph), (mt, lt, pt) = t["hip"], t["torch"]
        res[(N, "solve")] = (mh, mt)
        say(f"  N = {N}  solve (two launches)     kernels {mh:7.3f} ms (min {lh:7.3f})  peak {ph / 2**20:6.1f} MiB  "
            f"{need / mh / 1e9:5.2f} TB/s of the {need / 2**20:.0f} MiB it reads | torch path {mt:9.3f} ms (min {lt:9.3f})  peak "
            f"{pt / 2**20:6.0f} MiB | {mt / mh:6.1f}x | same bits: {same}; gains {[round(float(x), 3) for x in a_hip[:, 0, 0]]}")
        for mode in ("median", "mean"):
            for spread in (False, True):
                outs = [E.reduce_members(members, mode, spread=spread, backend=b, affine=a_hip) for b in ("torch", "hip")]
                same = torch.equal(outs[0][0], outs[1][0]) and (not spread or torch.equal(outs[0][1], outs[1][1]))
                del outs
                t = timed({"plain": lambda: E.reduce_members(members, mode, spread=spread, backend="hip"),
                           "affine": lambda: E.reduce_members(members, mode, spread=spread, backend="hip", affine=a_hip),
                           "torch": lambda: E.reduce_members(members, mode, spread=spread, backend="torch", affine=a_hip)})
                need = n * (N + (2 if spread else 1))
                (mp, lp, _), (ma, la, pa), (mt, lt, pt) = t["plain"], t["affine"], t["torch"]
                res[(N, mode, spread)] = (mp, ma, mt)
                say(f"  N = {N}  {mode:6s} {'+ spread' if spread else '        '}  today's reduce {mp:7.3f} ms (min {lp:7.3f}) | through "
                    f"the affines {ma:7.3f} ms (min {la:7.3f})  peak {pa / 2**20:5.0f} MiB  {need / ma / 1e9:5.2f} TB/s of the "
                    f"{need / 2**20:.0f} MiB it needs  {ma / mp:5.2f}x today's | torch path {mt:9.3f} ms  peak {pt / 2**20:6.0f} MiB  "
                    f"{mt / ma:6.1f}x | same bytes: {same}")
    say("  (an aligned pass costs the solve plus the reduce through the affines; today's reduce is what the same pass costs with "
        "the switch off)")
    for N in (3, 5, 8):
        mp, ma, _ = res[(N, "median", False)]
        say(f"  N = {N}: aligned median pass {res[(N, 'solve')][0] + ma:7.3f} ms against {mp:7.3f} ms unaligned")
    return res


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
    ap.add_argument("--align", action="store_true", help="ensembles that agree: the solve and the reduce through the affines")
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
        align_parity() if a.align else parity()
    elif a.align:
        if not torch.cuda.is_available():
            sys.exit("ensemblebench needs the GPU for its timings (--align --parity runs on the CPU)")
        if a.reps < 3:
            sys.exit("medians of at least three runs")
        say(f"# tools/ensemblebench.py --align on {torch.cuda.get_device_name(0)}; nothing was set in advance")
        align_leg(a.frames, a.height, a.width, a.reps)
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
