#!/usr/bin/env python3
"""The fit's way back at a 1080p clip (uint8 57 x 576 x 1024 -> 1080 x 1920, on the device): the torch device path (fit.py's
specification on the GPU) against drn_restore_frames_u8 in one process - medians over three alternated rounds of synchronised
runs, once with the D2H copy of the result inside the timed region and once without, and the peak device memory each path adds.
Then the launch alone between device events, and the bytes the algorithm needs (every source and result byte once) over that time,
next to the HBM rate an MI355X reaches.

    python tools/restorebench.py [T Hm Wm H W]      (timing)
    python tools/restorebench.py --parity           (the figures of the cases of tests/restore_refs.py)
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
import restore_refs as R  # noqa: E402

fit = R.fit_module(pkg)
dev = torch.device("cuda")
HBM_ACHIEVABLE_TBS = 6.3           # what streaming kernels reach on an MI355X (8 TB/s peak)


def parity():
    worst = 0.0
    cases = list(R.grid(R.GEOMETRIES + R.EXTRA))
    for g, B, Ts, Td in cases:
        c = R.case(pkg, g, B, Ts, Td)
        got = fit.restore_frames(c["src"].to(dev), c["rplan"], backend="hip").cpu()
        ok, ratio = R.bound_excess(got, c["ref64"], c["e_ref"])
        worst = max(worst, ratio)
        print(f"restore-frame {c['name']}: E_ref {c['e_ref']:.3e}  max((|hip - ref64| - 0.5)+ / E_ref) {ratio:.3f}  "
              f"{int((got != c['spec']).sum())} of {got.numel()} bytes differ from the specification  "
              f"{'within' if ok else 'OUTSIDE'} 0.5 + {R.M_BOUND} E_ref")
    print(f"worst ratio {worst:.3f} over {len(cases)} cases; the tests allow {R.M_BOUND}")


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


def timing(T, Hm, Wm, H, W):
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (1, T, Hm, Wm, 3), generator=g, dtype=torch.int32).to(torch.uint8).to(dev)
    rplan = fit.plan_restore(fit.plan_fit(T, H, W, "stretch", Hm, Wm, windowed=True))
    a = fit.restore_frames(u8, rplan, backend="torch")
    b = fit.restore_frames(u8, rplan, backend="hip")
    torch.cuda.synchronize()
    need = T * 3 * (Hm * Wm + H * W)
    print(f"uint8 {T} x {Hm} x {Wm} -> {H} x {W} (taps {rplan.y_w.shape[1]} x {rplan.x_w.shape[1]}): source {u8.numel() / 2**20:.0f} MiB, "
          f"result {b.numel() / 2**20:.0f} MiB; {int((a != b).sum())} of {b.numel()} bytes differ between hip and torch(device), "
          f"max difference {int((a.int() - b.int()).abs().max())}")
    del a, b
    arms = [
        ("torch(device), D2H copy included", lambda: fit.restore_frames(u8, rplan, backend="torch").cpu()),
        ("hip,           D2H copy included", lambda: fit.restore_frames(u8, rplan, backend="hip").cpu()),
        ("torch(device), result on device", lambda: fit.restore_frames(u8, rplan, backend="torch")),
        ("hip,           result on device", lambda: fit.restore_frames(u8, rplan, backend="hip")),
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
        print(f"{name:34s}: median {statistics.median(ms):9.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs)  "
              f"peak memory above the resident tensors {peaks[name]:8.1f} MiB")
    # the launch alone: tables resident, 20 launches back to back between two device events
    tabs = [t.to(dev) for t in (rplan.y_lo_n, rplan.y_w, rplan.x_lo_n, rplan.x_w)]
    out = torch.empty((1, T, H, W, 3), dtype=torch.uint8, device=dev)
    lib, stream = pkg.native.load_library(), torch.cuda.current_stream().cuda_stream

    def launch():
        rc = lib.drn_restore_frames_u8(u8.data_ptr(), out.data_ptr(), 1, T, Hm, Wm, T, H, W, tabs[0].data_ptr(), tabs[1].data_ptr(),
                                       rplan.y_w.shape[1], tabs[2].data_ptr(), tabs[3].data_ptr(), rplan.x_w.shape[1], stream)
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
    rate = need / (k / 1e3) / 1e12
    print(f"drn_restore_frames_u8 alone (device events, 20 launches, 3 rounds): {k:.3f} ms per launch "
          f"({' '.join(f'{v:.3f}' for v in per)}); the algorithm needs {need / 1e6:.0f} MB (every source and result byte once) = "
          f"{rate:.2f} TB/s, {rate / HBM_ACHIEVABLE_TBS * 100:.0f} % of the {HBM_ACHIEVABLE_TBS} TB/s a streaming kernel reaches from "
          f"HBM (the least time at that rate: {need / (HBM_ACHIEVABLE_TBS * 1e12) * 1e3:.3f} ms)")


if __name__ == "__main__":
    if "--parity" in sys.argv:
        parity()
    else:
        dims = [int(v) for v in sys.argv[1:6]] if len(sys.argv) > 5 else [57, 576, 1024, 1080, 1920]
        timing(*dims)
