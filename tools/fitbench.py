#!/usr/bin/env python3
"""The fit ingest at a 1080p clip (57 x 1080 x 1920 -> 576 x 1024, crop): the torch device path (fit.py's specification on the
GPU) against drn_fit_frames in one process - medians over three alternated rounds of synchronised runs, with the upload of the
fp32 frames inside and outside the timed region, and the peak device memory each path adds.  For scale: fit = "off" on a clip
that already is 576 x 1024, through today's host ingest (permute * 2 - 1 on the CPU, fp32 upload, bf16 cast on the device).

    python tools/fitbench.py [T Hs Ws Hd Wd]     (timing)
    python tools/fitbench.py --parity            (max((|hip - ref64| - 0.5 ulp)+ / E_ref) at the cases of tests/fit_refs.py)
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
import fit_refs as R  # noqa: E402

fit = R.fit_module(pkg)
dev = torch.device("cuda")


def parity():
    worst = 0.0
    for gi, B, T in R.grid():
        c = R.case(pkg, gi, B, T)
        got = fit.fit_frames(c["src"], c["plan"], dev, backend="hip").cpu()
        ok, ratio = R.bound_excess(got.double(), c["ref64"], c["e_ref"])
        worst = max(worst, ratio)
        print(f"{c['name']}: E_ref {c['e_ref']:.3e}  max((|hip - ref64| - 0.5 ulp_bf16)+ / E_ref) {ratio:.3f}  "
              f"{'within' if ok else 'OUTSIDE'} 0.5 ulp + {R.M_BOUND} E_ref")
    print(f"worst ratio {worst:.3f} over {len(list(R.grid()))} cases; the tests allow {R.M_BOUND}")


def timed(fn, runs=3):
    out = fn()                             # warm-up: code objects, allocator
    del out
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        del out
    return ms, (torch.cuda.max_memory_allocated() - base) / 2**20


def timing(T, Hs, Ws, Hd, Wd):
    g = torch.Generator().manual_seed(1)
    host = torch.rand(1, T, Hs, Ws, 3, generator=g)
    plan = fit.plan_fit(T, Hs, Ws, "crop", Hd, Wd)
    on_dev = host.to(dev)
    a = fit.fit_frames(on_dev, plan, dev, backend="torch").float()
    b = fit.fit_frames(on_dev, plan, dev, backend="hip").float()
    torch.cuda.synchronize()
    src_mib, dst_mib = host.numel() * 4 / 2**20, b.numel() * 2 / 2**20
    print(f"{T} x {Hs} x {Ws} -> {plan.T_out} x {plan.H_out} x {plan.W_out} crop (resized {plan.H_full} x {plan.W_full}, taps "
          f"{plan.y_w.shape[1]} x {plan.x_w.shape[1]}): source {src_mib:.0f} MiB fp32, result {dst_mib:.0f} MiB bf16; "
          f"max|hip - torch(device)| {(a - b).abs().max().item():.2e} (one bf16 ulp at 1 is 7.8e-03), "
          f"{(a != b).float().mean().item() * 100:.3f} % of the elements differ")
    del a, b
    on_grid = torch.rand(1, plan.T_out, plan.H_out, plan.W_out, 3, generator=g)
    arms = [
        ("torch(device), upload included", lambda: fit.fit_frames(host, plan, dev, backend="torch")),
        ("hip,           upload included", lambda: fit.fit_frames(host, plan, dev, backend="hip")),
        ("torch(device), frames on device", lambda: fit.fit_frames(on_dev, plan, dev, backend="torch")),
        ("hip,           frames on device", lambda: fit.fit_frames(on_dev, plan, dev, backend="hip")),
        (f"fit off, {plan.H_out} x {plan.W_out} clip, host ingest + upload + cast",
         lambda: (on_grid.permute(0, 4, 1, 2, 3) * 2.0 - 1.0).to(device=dev, dtype=torch.bfloat16)),
    ]
    runs = {name: [] for name, _ in arms}
    peaks = {}
    for _ in range(3):                     # alternated rounds
        for name, fn in arms:
            ms, peak = timed(fn)
            runs[name] += ms
            peaks[name] = max(peaks.get(name, 0.0), peak)
    for name, _ in arms:
        ms = runs[name]
        print(f"{name:48s}: median {statistics.median(ms):9.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs)  "
              f"peak memory above the resident tensors {peaks[name]:8.1f} MiB")
    # the launch alone: tables resident, 20 launches back to back between two device events
    tabs = [t.to(dev) for t in (plan.t_idx, plan.y_lo_n, plan.y_w, plan.x_lo_n, plan.x_w)]
    out = torch.empty((1, 3, plan.T_out, plan.H_out, plan.W_out), dtype=torch.bfloat16, device=dev)
    lib, stream = pkg.native.load_library(), torch.cuda.current_stream().cuda_stream

    def launch():
        rc = lib.drn_fit_frames(on_dev.data_ptr(), out.data_ptr(), 1, T, Hs, Ws, plan.T_out, plan.H_out, plan.W_out,
                                tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), plan.y_w.shape[1],
                                tabs[3].data_ptr(), tabs[4].data_ptr(), plan.x_w.shape[1], stream)
        assert rc == 0, rc
    launch()
    per = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            launch()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / 20)
    k = statistics.median(per)
    print(f"drn_fit_frames alone (device events, 20 launches, 3 rounds): {k:.3f} ms per launch "
          f"({' '.join(f'{v:.3f}' for v in per)}) = {(src_mib + dst_mib) / 1024 / (k / 1e3):.0f} GiB/s over source + result bytes")


if __name__ == "__main__":
    if "--parity" in sys.argv:
        parity()
    else:
        dims = [int(v) for v in sys.argv[1:6]] if len(sys.argv) > 5 else [57, 1080, 1920, 576, 1024]
        timing(*dims)
