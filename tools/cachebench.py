#!/usr/bin/env python3
"""The step cache (step_cache.py): what a computed step costs with the cache on, what a skipped step costs, and -
recorded, not judged - how many steps a threshold computes on synthetic weights.  On a GPU; nothing is set in advance.

    python tools/cachebench.py [--steps K] [--rounds R] [--reps N] [--out profiles/step_cache.txt]
    python tools/cachebench.py --sweep [--sweep-shape T H W] [--out ...]

(a) Pass leg (device events, median of `--reps`, arms alternating): the three streaming kernels and the copy of `ref` on the
    residual stream of 57 x 576 x 1024, [B x 18 432, 4096] bf16, B = 1 and 2.
(b) Step leg (host clock around K forwards of the 28-block engine that end in a synchronise, `--rounds` rounds, arms alternating,
    as tools/samplerbench.py measures): ms per step of the plain forward (the parent loop's), of a computed candidate step with the
    cache on (head, probe + one synchronisation, copy, tail, residual, final) and of a skipped step (head, probe + synchronisation,
    apply, final), at 57 x 576 x 1024 with B = 1 and B = 2 (the CFG batch) and at 1 x 256 x 256.  The cached arms run inside one
    cache_begin(.., K + 2) loop whose forced first and last step are not timed, so every timed step is a candidate; computed:
    threshold 1e-30 on an input that alternates between two latents; skipped: threshold 1.0 on an input that does not move
    (delta = 0), max_run = K + 2.
--sweep: threshold -> steps computed and the rel-L2 of the final latent against the uncached loop, under "euler" at 35 steps and
    "dpmpp_2m" at 8, synthetic weights, guidance 0.  Random weights say nothing about which threshold keeps a picture intact.
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
BF = torch.bfloat16
LINES = []
THRESHOLDS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.5)


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


# ----------------------------------------------------------------------------------------------- the pass leg
def pass_leg(reps):
    N = pkg.native
    dev = torch.device("cuda")
    S, D = 18432, 4096
    say(f"pass leg: the residual stream of 57 x 576 x 1024, [B x {S}, {D}] bf16; device events, median of {reps}, arms alternating")
    gen = torch.Generator(device="cuda").manual_seed(5)
    for B in (1, 2):
        x = torch.randn((B * S, D), generator=gen, device=dev, dtype=torch.float32).to(BF)
        ref = (x.float() * 1.01).to(BF)
        r = torch.empty_like(x)
        keep = torch.empty_like(x)
        stats = torch.empty((B, 2), dtype=torch.float64, device=dev)
        ws = torch.empty(N.load_library().drn_step_cache_workspace_bytes(B, S * D) // 8, dtype=torch.float64, device=dev)
        mib = x.numel() * 2 / 2 ** 20
        arms = {"drn_step_cache_probe (2 launches)": (lambda: N.step_cache_probe(x.view(B, -1), ref.view(B, -1), stats, ws), 2),
                "drn_step_cache_residual": (lambda: N.step_cache_residual(x, ref, out=r), 3),
                "drn_step_cache_apply": (lambda: N.step_cache_apply(x, r), 3),
                "ref <- X1 (torch copy_)": (lambda: keep.copy_(x), 2)}
        for fn, _ in arms.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(reps):
            for name, (fn, _) in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        for name, v in ms.items():
            med, streams = statistics.median(v), arms[name][1]
            say(f"  B = {B}: {name:34s} median {med * 1e3:8.1f} us   min {min(v) * 1e3:8.1f}  max {max(v) * 1e3:8.1f}   "
                f"{streams * mib * 2 ** 20 / med / 1e6:7.1f} GB/s of the {streams} x {mib:.0f} MiB it moves")


# ----------------------------------------------------------------------------------------------- the step leg
def _engine(dev):
    sw, cfgm = pkg.synthetic_weights, pkg.diffusion_renderer_config
    net = dict(cfgm.get_inverse_renderer_config(576, 1024, 57)["net"])
    eng = pkg.dit_engine.HipDiT(net, sw.synth_state_dict(net, BF, device=dev), device=dev)
    torch.cuda.empty_cache()
    return eng


def step_leg(eng, steps, rounds):
    dev = torch.device("cuda")
    sw = pkg.synthetic_weights
    say(f"step leg: 28-block engine, synthetic weights; host clock around {steps} forwards ending in a synchronise, over those steps; "
        f"one warm-up loop per arm, {rounds} rounds, arms alternating; the cached arms inside one cache_begin(.., {steps + 2}) loop whose "
        "forced first and last step are not timed")
    sigma = torch.tensor(1.7)
    eng.prepare_timesteps([1.7])
    for name, (T, H, W), B in (("57 x 576 x 1024, B = 1", (57, 576, 1024), 1), ("57 x 576 x 1024, B = 2 (CFG)", (57, 576, 1024), 2),
                               ("1 x 256 x 256, B = 1", (1, 256, 256), 1), ("1 x 256 x 256, B = 2 (CFG)", (1, 256, 256), 2)):
        shape = (B, 16, (T - 1) // 8 + 1, H // 8, W // 8)
        x = sw.synth_tensor("cachebench.x", shape, torch.float32, device=dev, scale=1.0).to(BF)
        cond = sw.synth_tensor("cachebench.cond", shape, torch.float32, device=dev, scale=1.0).to(BF)
        ci = [3, 0][:B]

        x2 = (x.float() * 1.02).to(BF)
        turn = [0]

        def forward(moving):
            turn[0] += 1
            return eng(x2 if moving and turn[0] % 2 else x, sigma, cond, ci)

        def timed(moving=False):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                y = forward(moving)
            torch.cuda.synchronize()
            assert torch.isfinite(y.float()).all(), "non-finite output"
            return (time.perf_counter() - t0) / steps * 1e3

        def cached(thr, want_computed):
            # computed: the input alternates between two latents, so every probe finds a distance; skipped: it stands still
            eng.cache_begin(thr, steps + 2, steps + 2)
            try:
                forward(want_computed)
                ms = timed(want_computed)
                forward(want_computed)
            finally:
                eng.cache_end()
            middle = [c for c, _ in eng.step_cache_log[1:-1]]
            assert middle == [want_computed] * steps, eng.step_cache_log
            return ms
        arms = {"plain forward (the parent's loop)": timed, "computed step, cache on": lambda: cached(1e-30, True),
                "skipped step": lambda: cached(1.0, False)}
        for fn in arms.values():
            fn()
        ms = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                ms[k].append(fn())
        plain = statistics.median(ms["plain forward (the parent's loop)"])
        for k, v in ms.items():
            med = statistics.median(v)
            say(f"  {name:30s} {k:34s} median {med:8.3f} ms per step  ({med / plain:5.3f} x plain)   runs {' '.join(f'{t:.3f}' for t in v)}")


# ----------------------------------------------------------------------------------------------- --sweep
def sweep(eng, shape_thw):
    dev = torch.device("cuda")
    sw, cfgm = pkg.synthetic_weights, pkg.diffusion_renderer_config
    T, H, W = shape_thw
    cfg = cfgm.get_inverse_renderer_config(H, W, T)
    model = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=dev)
    model.net = eng
    model._get_conditions = lambda batch, **kw: model.conditioner.get_condition_uncondition(batch)      # latents handed over ready
    shape = (16, (T - 1) // 8 + 1, H // 8, W // 8)
    noise = (sw.synth_tensor("cachebench.noise", (1, *shape), torch.float32, device=dev, scale=1.0) * 80.0).to(BF)
    cond = sw.synth_tensor("cachebench.cond", (1, *shape), torch.float32, device=dev, scale=1.0).to(BF)
    batch = lambda: {"latent_condition": cond, "context_index": torch.full((1, 1), 3, dtype=torch.long)}
    say(f"sweep: {T} x {H} x {W}, 28 blocks, SYNTHETIC weights, guidance 0, max_run 3; recorded, not judged: random weights say nothing "
        "about which threshold keeps a picture intact")
    say("| sampler | steps | threshold | steps computed | rel-L2 of the final latent against the uncached loop | largest delta skipped |")
    say("|---|---|---|---|---|---|")
    for sampler, steps in (("euler", 35), ("dpmpp_2m", 8)):
        kw = dict(guidance=0.0, seed=7, state_shape=list(shape), num_steps=steps, init_noise=noise, sampler=sampler)
        base = model.generate_samples_from_batch(batch(), **kw).float()
        for thr in THRESHOLDS:
            out = model.generate_samples_from_batch(batch(), step_cache=thr, **kw).float()
            log = eng.step_cache_log
            rel = float((out - base).norm() / base.norm())
            skipped = [d for c, d in log if not c]
            say(f"| {sampler} | {steps} | {thr} | {sum(1 for c, _ in log if c)} | {rel:.3e} | "
                f"{max(skipped) if skipped else float('nan'):.4f} |")
        deltas = [d for _, d in eng.step_cache_log if d is not None]
        say(f"  ({sampler}: the deltas the last loop logged range {min(deltas):.4f} .. {max(deltas):.4f})" if deltas else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true", help="the threshold table alone")
    ap.add_argument("--sweep-shape", type=int, nargs=3, default=(57, 576, 1024), metavar=("T", "H", "W"))
    ap.add_argument("--passes-only", action="store_true", help="the pass leg alone (no network is built)")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cachebench needs the GPU: nothing here can be measured on a CPU")
    if a.rounds < 3 or a.reps < 3 or a.steps < 2:
        sys.exit("medians of at least three rounds, at least two steps")
    say(f"# tools/cachebench.py{' --sweep' if a.sweep else ''} on {torch.cuda.get_device_name(0)}")
    if a.sweep:
        sweep(_engine(torch.device("cuda")), tuple(a.sweep_shape))
    else:
        pass_leg(a.reps)
        if not a.passes_only:
            step_leg(_engine(torch.device("cuda")), a.steps, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
