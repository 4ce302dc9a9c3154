#!/usr/bin/env python3
"""The guided way back at a 1080p clip (uint8 57 x 576 x 1024 -> 1080 x 1920, on the device): the torch device path (fit.py's
specification on the GPU) against drn_restore_guided_u8 and, as the yardstick of what guiding costs, the plain way back
(drn_restore_frames_u8), in one process - medians over three alternated rounds of synchronised runs with the result left on the
device, and the peak device memory each path adds.  Then each launch alone between device events, and the bytes the algorithm
needs (every source, guide and result byte once) over that time, next to the HBM rate an MI355X reaches.  The picture is a scene
of palette regions +- 3 levels, so that the range term is at work as it would be on a real picture.

    python tools/guidedbench.py [T Hm Wm H W]
"""
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
fit = importlib.import_module(pkg.__name__ + ".fit")
dev = torch.device("cuda")
HBM_ACHIEVABLE_TBS = 6.3           # what streaming kernels reach on an MI355X (8 TB/s peak)
SIGMA = 12.0


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


def scene(plan, T):
    """-> guide_hi, guide_lo, src on the device: two palettes on the same drifting blocks, the guide's +- 3 levels, both taken to
    the model's size by the fit's own tables."""
    g = torch.Generator(device="cpu").manual_seed(1)
    pal = torch.randint(0, 256, (2, 7, 3), generator=g, dtype=torch.int32).to(dev)
    y = torch.arange(plan.H, device=dev).view(1, -1, 1)
    x = torch.arange(plan.W, device=dev).view(1, 1, -1)
    t = torch.arange(T, device=dev).view(-1, 1, 1)
    reg = ((y + 3 * t) // 97 * 3 + (x + 5 * t) // 131) % 7
    noise = torch.randint(-3, 4, (T, plan.H, plan.W, 3), generator=torch.Generator(device=dev).manual_seed(2), dtype=torch.int32,
                          device=dev)
    hi = (pal[0][reg] + noise).clamp(0, 255).to(torch.uint8).unsqueeze(0).contiguous()
    truth = pal[1][reg].to(torch.uint8).unsqueeze(0).contiguous()
    down = fit.plan_guide_lo(plan)
    return hi, fit.restore_frames(hi, down), fit.restore_frames(truth, down), truth


def events(launch, n=20):
    launch()
    per = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            launch()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / n)
    return statistics.median(per), per


def timing(T, Hm, Wm, H, W):
    plan = fit.plan_fit(T, H, W, "stretch", Hm, Wm, windowed=True)
    gplan, rplan = fit.plan_restore_guided(plan, SIGMA), fit.plan_restore(plan)
    hi, lo, u8, truth = scene(plan, T)
    a = fit.restore_frames_guided(u8, gplan, hi, lo, backend="torch")
    b = fit.restore_frames_guided(u8, gplan, hi, lo, backend="hip")
    c = fit.restore_frames(u8, rplan, backend="hip")
    torch.cuda.synchronize()

    def mae(v):
        return float((v.float() - truth.float()).abs().mean())
    print(f"uint8 {T} x {Hm} x {Wm} -> {H} x {W} (taps {gplan.y_w.shape[1]} x {gplan.x_w.shape[1]}, sigma {SIGMA}): source "
          f"{u8.numel() / 2**20:.0f} MiB, guides {hi.numel() / 2**20:.0f} + {lo.numel() / 2**20:.0f} MiB, result {b.numel() / 2**20:.0f} "
          f"MiB; {int((a != b).sum())} of {b.numel()} bytes differ between hip and torch(device), max difference "
          f"{int((a.int() - b.int()).abs().max())}")
    print(f"on this scene of palette blocks: MAE against the full-size truth {mae(b):.2f} of 255 guided, {mae(c):.2f} plain")
    del a, b, c, truth
    arms = [
        ("torch(device) guided", lambda: fit.restore_frames_guided(u8, gplan, hi, lo, backend="torch")),
        ("hip guided", lambda: fit.restore_frames_guided(u8, gplan, hi, lo, backend="hip")),
        ("hip plain (drn_restore_frames_u8)", lambda: fit.restore_frames(u8, rplan, backend="hip")),
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
    # the launches alone: tables resident, 20 launches back to back between two device events
    lib, stream = pkg.native.load_library(), torch.cuda.current_stream().cuda_stream
    out = torch.empty((1, T, H, W, 3), dtype=torch.uint8, device=dev)
    gt = [t.to(dev) for t in (gplan.y_lo_n, gplan.y_w, gplan.x_lo_n, gplan.x_w, gplan.tab)]
    rt = [t.to(dev) for t in (rplan.y_lo_n, rplan.y_w, rplan.x_lo_n, rplan.x_w)]

    def guided():
        rc = lib.drn_restore_guided_u8(u8.data_ptr(), lo.data_ptr(), hi.data_ptr(), out.data_ptr(), 1, 1, T, Hm, Wm, T, 0, T, H, W,
                                       gt[0].data_ptr(), gt[1].data_ptr(), gplan.y_w.shape[1], gt[2].data_ptr(), gt[3].data_ptr(),
                                       gplan.x_w.shape[1], gt[4].data_ptr(), gplan.eps, stream)
        assert rc == 0, rc

    def plain():
        rc = lib.drn_restore_frames_u8(u8.data_ptr(), out.data_ptr(), 1, T, Hm, Wm, T, H, W, rt[0].data_ptr(), rt[1].data_ptr(),
                                       rplan.y_w.shape[1], rt[2].data_ptr(), rt[3].data_ptr(), rplan.x_w.shape[1], stream)
        assert rc == 0, rc
    for name, fn, need, what in (("drn_restore_guided_u8", guided, T * 3 * (2 * Hm * Wm + 2 * H * W), "source, guide and result"),
                                 ("drn_restore_frames_u8", plain, T * 3 * (Hm * Wm + H * W), "source and result")):
        k, per = events(fn)
        rate = need / (k / 1e3) / 1e12
        print(f"{name} alone (device events, 20 launches, 3 rounds): {k:.3f} ms per launch ({' '.join(f'{v:.3f}' for v in per)}); the "
              f"algorithm needs {need / 1e6:.0f} MB (every {what} byte once) = {rate:.2f} TB/s, "
              f"{rate / HBM_ACHIEVABLE_TBS * 100:.0f} % of the {HBM_ACHIEVABLE_TBS} TB/s a streaming kernel reaches from HBM (the least "
              f"time at that rate: {need / (HBM_ACHIEVABLE_TBS * 1e12) * 1e3:.3f} ms)")


if __name__ == "__main__":
    dims = [int(v) for v in sys.argv[1:6]] if len(sys.argv) > 5 else [57, 576, 1024, 1080, 1920]
    timing(*dims)
