#!/usr/bin/env python3
"""A light per frame (env_sequence) at the headline clip (T = 57, 576 x 1024, 57 panoramas of 1024 x 2048, cube maps of 512^2, spin 0
and 360): the torch per-frame loop on the device against the two kernels (drn_env_cubes + drn_env_project_seq, chunks of 16
frames) in one process - medians of alternated, synchronised rounds after a warm-up of each, the peak device memory each path adds
above its inputs, and per kernel the bytes it must move over its time.

    python tools/envseqbench.py [T H W He We]      (--rounds N, default 5)
    python tools/envseqbench.py --parity           (per case |hip - float64| / s over E_ref at the cases of tests/envseq_refs.py)
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
import envmap_refs as ER  # noqa: E402
import envseq_refs as SR  # noqa: E402

pe = ER.pe_module(pkg)
dev = torch.device("cuda")
R = pe.SEQ_CUBE_RES


def parity():
    worst = 0.0
    for i, cid in enumerate(SR.CUBE_CASE_IDS):
        c = SR.cube_case(pkg, i)
        out = pkg.native.env_cubes(c["latlong"].to(dev), c["grid"].to(dev), c["n0"], c["n"], c["brightness"], c["flip"], c["roll"])
        torch.cuda.synchronize()
        err = SR.cube_err(out, c)
        worst = max(worst, err / c["e_ref"])
        print(f"{cid}: E_ref {c['e_ref']:.3e}  max|hip - ref64|/s {err:.3e}  ratio {err / c['e_ref']:.3f}")
    m = 1
    while m < 2.0 * worst:
        m *= 2
    print(f"worst ratio {worst:.3f} -> smallest power of two with 2x headroom: m = {m} (limit {SR.M_MAX}); tests use M_CUBES = {SR.M_CUBES}")


def lights(N, He, We):
    """N HDR panoramas on the device, rand^4 * 50 from one seed (what tests/envmap_refs.panorama() is made of)."""
    g = torch.Generator(device=dev).manual_seed(20250311)
    return torch.rand(N, He, We, 3, generator=g, device=dev).pow(4) * 50.0


def run(frames, H, W, T, spin, backend):
    d = pe._projection_sequence(frames, (H, W), 1.0, False, 180.0, dev, T, False, spin, backend)
    if "cond_ldr" in d:
        return d["cond_ldr"], d["cond_log"]
    return ((d["env_ldr"].permute(3, 0, 1, 2) * 2.0 - 1.0).contiguous(), (d["env_log"].permute(3, 0, 1, 2) * 2.0 - 1.0).contiguous())


def kernel_times(frames, H, W, T, spin):
    """Device-event time of every launch of one chunked build, summed per kernel -> (ms cubes, ms project, launches of each)."""
    native = pkg.native
    events = {"cubes": [], "project": []}

    def timed(name, fn):
        def inner(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            events[name].append((e0, e1))
            return out
        return inner

    real = native.env_cubes, native.env_project_seq
    native.env_cubes, native.env_project_seq = timed("cubes", real[0]), timed("project", real[1])
    try:
        run(frames, H, W, T, spin, "hip")
        torch.cuda.synchronize()
    finally:
        native.env_cubes, native.env_project_seq = real
    return {k: (sum(a.elapsed_time(b) for a, b in v), len(v)) for k, v in events.items()}


def timing(T, H, W, He, We, rounds):
    frames = lights(T, He, We)
    torch.cuda.synchronize()
    gib = 2.0 ** 30
    print(f"T={T} H={H} W={W}: {T} panoramas of {He} x {We} ({frames.numel() * 4 / gib:.2f} GiB), cube maps {R}^2 "
          f"({6 * R * R * 12 / 2**20:.1f} MiB each, {pe.SEQ_CHUNK} per chunk), outputs 2 x [3,{T},{H},{W}] fp32 = "
          f"{2 * 3 * T * H * W * 4 / 2**20:.0f} MiB")
    for spin in (0.0, 360.0):
        a, b = run(frames, H, W, T, spin, "torch"), run(frames, H, W, T, spin, "hip")          # warm-up of both, and their difference
        torch.cuda.synchronize()
        diff = max((x - y).abs().max().item() for x, y in zip(a, b))
        del a, b
        ms = {"torch": [], "hip": []}
        peak = {}
        for _ in range(rounds):
            for name in ("torch", "hip"):                                                        # alternated
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                out = run(frames, H, W, T, spin, name)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
                peak[name] = max(peak.get(name, 0.0), (torch.cuda.max_memory_allocated() - base) / 2**20)
                del out
        print(f"spin {spin:5.1f}: max|hip - torch(device)| {diff:.2e} (tie pixels included)")
        for name in ("torch", "hip"):
            print(f"  {name:5s}: median {statistics.median(ms[name]):10.3f} ms  rounds {' '.join(f'{v:.1f}' for v in ms[name])}  "
                  f"peak memory above the inputs {peak[name]:8.1f} MiB")
        print(f"  torch / hip = {statistics.median(ms['torch']) / statistics.median(ms['hip']):.1f}x")
        kt = kernel_times(frames, H, W, T, spin)
        # the bytes each kernel must move: cubes = every panorama once + the grid per launch + the cube maps written;
        # project = the cube maps read once + the directions per launch + both outputs written
        n_launch = kt["cubes"][1]
        by_cubes = T * He * We * 12 + n_launch * 6 * R * R * 8 + T * 6 * R * R * 12
        by_proj = T * 6 * R * R * 12 + n_launch * H * W * 12 + 2 * 3 * T * H * W * 4
        for name, by in (("cubes", by_cubes), ("project", by_proj)):
            t_ms, n = kt[name]
            print(f"  drn_env_{'cubes' if name == 'cubes' else 'project_seq'}: {n} launches, {t_ms:8.3f} ms in all (device events), "
                  f"{by / 2**20:8.1f} MiB to move -> {by / (t_ms * 1e-3) / 1e12:.2f} TB/s")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    if "--rounds" in sys.argv:
        args.remove(str(rounds))
    if "--parity" in sys.argv:
        parity()
    else:
        dims = [int(v) for v in args[:5]] if len(args) >= 5 else [57, 576, 1024, 1024, 2048]
        timing(*dims, rounds)
