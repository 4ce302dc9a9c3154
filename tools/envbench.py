#!/usr/bin/env python3
"""The rotating environment light at the headline clip (T = 57, 576 x 1024, spin 360): the torch path against drn_env_project in
one process - median of 5 synchronised runs after a warm-up each, and the peak device memory each path adds.

    python tools/envbench.py [T H W]          (timing; the cube map is built once, outside the timed region, as per clip)
    python tools/envbench.py --parity         (max|hip - float64| / E_ref at the cases of tests/envmap_refs.py, and the two device
                                               paths of envmap_conditions against each other in the same unit)
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

pe = ER.pe_module(pkg)
dev = torch.device("cuda")


def parity():
    worst = 0.0
    for i, cid in list(enumerate(ER.CASE_IDS)) + [("node", ER.NODE_CASE_ID)]:
        c = ER.case(pkg, i)
        out = pkg.native.env_project(c["cube"].to(dev), c["vec"].to(dev), c["rot"].to(dev), ER.LOG_SCALE)
        torch.cuda.synchronize()
        err = ER.max_err(out, c["ref"], c["mask"])
        worst = max(worst, err / c["e_ref"])
        print(f"{cid}: E_ref {c['e_ref']:.3e}  max|hip - ref64| {err:.3e}  ratio {err / c['e_ref']:.3f}  "
              f"tie share {c['mask'].float().mean().item():.4f}")
    # the same bound is asked of envmap_conditions' two device paths against each other (tests/test_envmap_gpu.py)
    c = ER.node_case_on(pe, dev)              # references from the cube map / directions built on the device, as both paths use
    H, W, T, spin, _ = ER.NODE_CASE
    got = []
    for backend in ("hip", "torch"):
        pe.clear_environment_cache()
        d = pe.envmap_conditions(ER.panorama(), (H, W), T, "proj", 1.0, False, 0.0, device=dev, env_spin=spin, backend=backend)
        got.append((d["env_ldr"][0].double().cpu(), d["env_log"][0].double().cpu()))
    pe.clear_environment_cache()
    diff = ER.max_err(got[0], got[1], c["mask"])
    worst = max(worst, diff / c["e_ref"])
    for name, g in zip(("hip", "torch(device)"), got):
        err = ER.max_err(g, c["ref"], c["mask"])
        worst = max(worst, err / c["e_ref"]) if name == "hip" else worst
        print(f"{ER.NODE_CASE_ID} through envmap_conditions: E_ref {c['e_ref']:.3e}  max|{name} - ref64| {err:.3e}  ratio {err / c['e_ref']:.3f}")
    print(f"{ER.NODE_CASE_ID} through envmap_conditions: max|hip - torch(device)| {diff:.3e}  ratio {diff / c['e_ref']:.3f}")
    m = 1
    while m < 2.0 * worst:
        m *= 2
    print(f"worst ratio {worst:.3f} -> smallest power of two with 2x headroom: m = {m} (limit {ER.M_MAX}); tests use M_BOUND = {ER.M_BOUND}")


def timed(fn, runs=5):
    fn()                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
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
    return statistics.median(ms), ms, (torch.cuda.max_memory_allocated() - base) / 2**20


def timing(T, H, W, spin=360.0):
    latlong = pe.apply_hdr_preprocessing(ER.panorama(), 1.0, False, 0.0, dev)
    cube = pe.latlong_to_cubemap_official(latlong, [512, 512]).contiguous()
    vec = pe.latlong_vec((H, W), device=dev).contiguous()
    rot = pe.spin_table(spin, T)
    rot_dev = rot.to(dev)
    mats = [pe.rotate_y(a, device=dev) for a in pe.spin_angles(spin, T)]

    def torch_path():
        ms = [pe.project_frame(cube, vec, m) for m in mats]
        ldr, log = torch.stack([m["env_ev0"] for m in ms]), torch.stack([m["env_log"] for m in ms])
        return (ldr.permute(3, 0, 1, 2) * 2.0 - 1.0).contiguous(), (log.permute(3, 0, 1, 2) * 2.0 - 1.0).contiguous()

    def hip_path():
        return pkg.native.env_project(cube, vec, rot_dev, ER.LOG_SCALE)

    a, b = torch_path(), hip_path()
    torch.cuda.synchronize()
    diff = max((x - y).abs().max().item() for x, y in zip(a, b))
    del a, b
    out_mib = 2 * 3 * T * H * W * 4 / 2**20
    print(f"T={T} H={H} W={W} spin={spin}: cube 512^2, outputs 2 x [3,{T},{H},{W}] fp32 = {out_mib:.0f} MiB; "
          f"max|hip - torch(device)| {diff:.2e} (tie pixels included)")
    for name, fn in (("torch", torch_path), ("hip", hip_path), ("torch", torch_path), ("hip", hip_path)):
        med, ms, peak = timed(fn)
        print(f"{name:5s}: median {med:9.3f} ms  runs {' '.join(f'{v:.3f}' for v in ms)}  peak memory above the inputs {peak:8.1f} MiB")


if __name__ == "__main__":
    if "--parity" in sys.argv:
        parity()
    else:
        dims = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else [57, 576, 1024]
        timing(*dims)
