#!/usr/bin/env python3
"""The samplers of the denoising loop (sampler.py): what the second-order sampler buys in steps, and what its
fused step costs, each measured where it can be.

    python tools/samplerbench.py --order [--out profiles/sampler_order.txt]          (CPU: no GPU needed)
    python tools/samplerbench.py [--steps K] [--rounds R] [--reps N] [--out profiles/sampler.txt]

--order: the convergence table, on the CPU, from sampler.step_reference alone.  The reference's schedule (logspace 80 -> 0.02 plus
    the trailing 0), an analytic Gaussian denoiser with 16 data scales, the exact solution of the ODE as the truth; "euler" against
    "dpmpp_2m" with a float64 state (the samplers' own error) and with the bf16 state the loop keeps (network output rounded to
    bf16 too).  It says nothing about pictures: synthetic weights cannot judge them.
default: on a GPU, interleaved rounds in one process.
(a) Launch leg (device events, median of `--reps`, arms alternating inside every repetition), at the headline latent
    [P,16,8,72,128], P = 1 and 5, CFG on and off: the launches the Euler loop spends between two DiT calls - drn_cfg_combine (CFG),
    drn_edm_step, the next step's drn_edm_scale_input, torch.cat([xs, xs]) (CFG) - against the one drn_sampler_step_2m.
(b) Step leg (host clock around a whole generate_samples_from_batch that ends in a synchronise, over its steps; `--rounds`
    rounds, samplers alternating): ms per step under "euler" and "dpmpp_2m" at 1 x 256 x 256 and 57 x 576 x 1024, the 28-block
    network with synthetic weights, guidance 0, condition latents handed over ready.
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
S = pkg.sampler
BF = torch.bfloat16
LINES = []
SIGMA_MAX, SIGMA_MIN, SIGMA_DATA = 80.0, 0.02, 0.5


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


# ----------------------------------------------------------------------------------------------- --order
def solve(kind, steps, state, x0, std):
    sched = pkg.model_diffusion_renderer.CleanEDMEulerScheduler(sigma_max=SIGMA_MAX, sigma_min=SIGMA_MIN, sigma_data=SIGMA_DATA)
    sched.set_timesteps(steps)
    x, hist = x0.to(state), None
    for sigma, coef in zip(sched.timesteps, S.plan_steps(sched.sigmas, SIGMA_DATA, kind)):
        xd = x.to(torch.float64)
        denoised = xd * (std ** 2 / (std ** 2 + float(sigma) ** 2))
        m = ((denoised - coef.c_skip * xd) / coef.c_out).to(state)            # what the network would answer
        x, hist, _ = S.step_reference(m, None, 0.0, x, hist, coef, state_dtype=state)
    truth = x0 * ((std ** 2 + SIGMA_MIN ** 2) / (std ** 2 + SIGMA_MAX ** 2)).sqrt()
    truth = truth * (std ** 2 / (std ** 2 + SIGMA_MIN ** 2))
    return float((x.to(torch.float64) - truth).pow(2).mean().sqrt())


def order_table():
    x0 = torch.randn(16, 4096, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * SIGMA_MAX
    std = torch.linspace(0.2, 1.0, 16, dtype=torch.float64)[:, None]
    say("# tools/samplerbench.py --order (CPU): RMS distance to the exact ODE solution; Gaussian denoiser, data std 0.2 .. 1.0 in 16 "
        "rows of 4096, x0 = randn * 80 (seed 0), schedule logspace(80 -> 0.02) + 0")
    say("| steps | Euler, fp64 state | 2M, fp64 state | Euler, bf16 state | 2M, bf16 state |")
    say("|---|---|---|---|---|")
    err = {}
    for n in (8, 15, 32, 35, 64):
        row = [solve(k, n, st, x0, std) for st in (torch.float64, BF) for k in ("euler", "dpmpp_2m")]
        err[n] = row
        say(f"| {n} | {row[0]:.2e} | {row[1]:.2e} | {row[2]:.2e} | {row[3]:.2e} |")
    say(f"32 -> 64 steps, fp64 state: 2M's error falls by {err[32][1] / err[64][1]:.2f} (second order), Euler's by "
        f"{err[32][0] / err[64][0]:.2f} (first order)")
    say(f"2M at 8 steps against Euler at 64, fp64 state: {err[8][1]:.2e} against {err[64][0]:.2e}")
    say(f"2M at 8 steps against Euler at 35, bf16 state: {err[8][3]:.2e} against {err[35][2]:.2e} ({err[35][2] / err[8][3]:.1f}x); "
        f"the bf16 state's rounding floor shows in 2M's last rows")
    say("(synthetic: an analytic denoiser, no network; nothing here judges pictures)")


# ----------------------------------------------------------------------------------------------- the launch leg
def launch_leg(reps):
    N = pkg.native
    dev = torch.device("cuda")
    sched = pkg.model_diffusion_renderer.CleanEDMEulerScheduler(sigma_max=SIGMA_MAX, sigma_min=SIGMA_MIN, sigma_data=SIGMA_DATA)
    sched.set_timesteps(15)
    coef = S.plan_steps(sched.sigmas, SIGMA_DATA)[7]
    sched.current_step = 7
    _, c_skip, c_out, sigma, dt = sched.step_scalars(sched.timesteps[7])
    gen = torch.Generator(device="cuda").manual_seed(3)
    say(f"launch leg: latent [P,16,8,72,128] bf16, step 7 of 15; device events, median of {reps}, arms alternating; the Euler arm is "
        "drn_cfg_combine (CFG) + drn_edm_step + the next drn_edm_scale_input + torch.cat (CFG), the fused arm one drn_sampler_step_2m "
        "with its fp32 history read and written")
    for P in (1, 5):
        for cfg in (False, True):
            rnd = lambda: torch.randn((P, 16, 8, 72, 128), generator=gen, device=dev, dtype=torch.float32).to(BF)
            c, u, x = rnd(), (rnd() if cfg else None), rnd() * 3.0
            hist = torch.randn((P, 16, 8, 72, 128), generator=gen, device=dev, dtype=torch.float32)
            copies = 2 if cfg else 1

            def euler():
                m = N.cfg_combine(c, u, 2.0) if cfg else c
                xn = N.edm_step(m, x, c_skip, c_out, sigma, dt)
                xs = N.edm_scale_input(xn, coef.c_in_next)
                return torch.cat([xs, xs], 0) if cfg else xs

            def fused():
                return S.step_reference(c, u, 2.0, x, hist, coef, copies, backend="hip", hist_out=hist)[2]
            arms = {"euler": euler, "fused": fused}
            for fn in arms.values():
                fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in arms}
            for _ in range(reps):
                for name, fn in arms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = fn()
                    e1.record()
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1))
                    del out
            n = x.numel()
            need = n * ((4 if cfg else 2) + 2 + 4 + 4 + 2 + 2 * copies)          # the fused launch: inputs, history in and out, outputs
            for name, v in ms.items():
                med = statistics.median(v)
                label = f"{(4 if cfg else 2)} launches of the Euler loop" if name == "euler" else "drn_sampler_step_2m"
                extra = f"   {need / med / 1e6:7.1f} GB/s of the {need / 2**20:.0f} MiB it needs" if name == "fused" else ""
                say(f"  P = {P}, CFG {'on ' if cfg else 'off'}: {label:32s} median {med * 1e3:8.1f} us   min {min(v) * 1e3:8.1f}  "
                    f"max {max(v) * 1e3:8.1f}{extra}")


# ----------------------------------------------------------------------------------------------- the step leg
def step_leg(steps, rounds):
    dev = torch.device("cuda")
    sw, cfgm = pkg.synthetic_weights, pkg.diffusion_renderer_config
    say(f"step leg: 28-block network, synthetic weights, guidance 0, {steps} steps per call; host clock around "
        f"generate_samples_from_batch ending in a synchronise, over its steps; one warm-up call per sampler, {rounds} rounds, samplers "
        "alternating")
    model = None
    for name, (T, H, W) in (("1 x 256 x 256", (1, 256, 256)), ("57 x 576 x 1024", (57, 576, 1024))):
        cfg = cfgm.get_inverse_renderer_config(H, W, T)
        if model is None:
            model = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=dev)
            model.load_state_dict(sw.synth_state_dict(dict(cfg["net"]), BF, device=dev), strict=True)
            torch.cuda.empty_cache()
            # the condition latents are handed over ready: no tokenizer in this leg
            model._get_conditions = lambda batch, **kw: model.conditioner.get_condition_uncondition(batch)
        shape = (16, (T - 1) // 8 + 1, H // 8, W // 8)
        noise = (sw.synth_tensor("samplerbench.noise", (1, *shape), torch.float32, device=dev, scale=1.0) * SIGMA_MAX).to(BF)
        cond = sw.synth_tensor("samplerbench.cond", (1, *shape), torch.float32, device=dev, scale=1.0).to(BF)
        batch = lambda: {"latent_condition": cond, "context_index": torch.full((1, 1), 3, dtype=torch.long)}

        def run(kind):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate_samples_from_batch(batch(), guidance=0.0, seed=7, state_shape=list(shape), num_steps=steps,
                                                    init_noise=noise, sampler=kind)
            torch.cuda.synchronize()
            assert torch.isfinite(out.float()).all(), "non-finite latent"
            return (time.perf_counter() - t0) / steps * 1e3
        for kind in S.SAMPLERS:
            run(kind)
        ms = {k: [] for k in S.SAMPLERS}
        for _ in range(rounds):
            for kind in S.SAMPLERS:
                ms[kind].append(run(kind))
        for kind, v in ms.items():
            say(f"  {name:16s} sampler = {kind!r:11s} median {statistics.median(v):8.3f} ms per step   runs {' '.join(f'{x:.3f}' for x in v)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--order", action="store_true", help="the convergence table, on the CPU; nothing else")
    ap.add_argument("--launches-only", action="store_true", help="the launch leg alone (no network is built)")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.order:
        order_table()
    else:
        if not torch.cuda.is_available():
            sys.exit("samplerbench needs the GPU for everything but --order: nothing else here can be measured on a CPU")
        if a.rounds < 3 or a.reps < 3 or a.steps < 2:
            sys.exit("medians of at least three rounds, at least two steps")
        say(f"# tools/samplerbench.py on {torch.cuda.get_device_name(0)}")
        launch_leg(a.reps)
        if not a.launches_only:
            step_leg(a.steps, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
