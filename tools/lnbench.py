#!/usr/bin/env python3
"""The HBM-bound passes of a DiT block alone, at the cfg-3 shape (18 432 rows, D = 4096, 32 heads), against a plain copy of the
same byte count on the same device:
    python tools/lnbench.py [--lib path/to/libdrn_variant.so ...] [--rounds 15]
ln_modulate without and with the pending add (the launcher's own kernel choice, and both kernels forced), q/k norm + RoPE.
Several --lib arguments are timed interleaved in ONE process; the gate (abgate.py) compares every later library with the first."""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from tools.abgate import gate, quartiles  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[])
    ap.add_argument("--rows", type=int, default=18432)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10, help="launches per timing")
    ap.add_argument("--cold", type=int, default=4, help="rotate over this many copies of the activations, so that a launch finds its "
                    "input where the model's does - written by another kernel a while ago - and not left in the 256 MB Infinity "
                    "Cache by its own previous launch (1: one copy, which flatters whatever keeps that copy cached)")
    args = ap.parse_args()
    pkg = load_package()
    N = pkg.native
    libs = args.lib or [N.library_path()]
    handles = []
    for path in libs:
        lib = ctypes.CDLL(os.path.abspath(path))
        for name, at in N.SIGNATURES.items():
            if hasattr(lib, name):
                getattr(lib, name).argtypes = at
        handles.append(lib)
    dev = torch.device("cuda")
    rows, D, H = args.rows, 4096, 32
    g = torch.Generator(device="cpu").manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)

    st = torch.cuda.current_stream().cuda_stream
    x0, qkv0 = rnd(rows, D), rnd(rows, 3 * D)
    xs, hs = [x0.clone() for _ in range(args.cold)], [torch.empty_like(x0) for _ in range(args.cold)]
    qkvs = [qkv0.clone() for _ in range(args.cold)]
    sh, sc, ad = rnd(1, D), rnd(1, D), rnd(1, D) * 1e-3
    turn = [0]
    wq, wk = rnd(128), rnd(128)
    cs, sn = rnd(rows, 128), rnd(rows, 128)
    row_bytes = rows * D * 2

    def ln(lib, add, force):
        turn[0] = (turn[0] + 1) % args.cold
        x, h = xs[turn[0]], hs[turn[0]]
        lib.drn_ln_force_kernel(force)
        rc = lib.drn_ln_modulate(x.data_ptr(), add.data_ptr() if add is not None else None, sh.data_ptr(), sc.data_ptr(), h.data_ptr(),
                                 rows, D, rows, 1e-6, st)
        lib.drn_ln_force_kernel(-1)
        assert rc == 0, rc

    def qk(lib):
        turn[0] = (turn[0] + 1) % args.cold
        qkv = qkvs[turn[0]]
        rc = lib.drn_qk_norm_rope(qkv.data_ptr(), qkv.data_ptr() + 2 * D, wq.data_ptr(), wk.data_ptr(), cs.data_ptr(), sn.data_ptr(),
                                  rows, H, 3 * D, 3 * D, rows, 0, 1e-6, st)
        assert rc == 0, rc

    cases = [("ln_modulate          (launcher's choice)", lambda lib: ln(lib, None, -1), 2 * row_bytes),
             ("ln_modulate          1 wave/row", lambda lib: ln(lib, None, 0), 2 * row_bytes),
             ("ln_modulate          4 waves/row", lambda lib: ln(lib, None, 1), 2 * row_bytes),
             ("ln_modulate + add    (launcher's choice)", lambda lib: ln(lib, ad, -1), 3 * row_bytes),
             ("ln_modulate + add    1 wave/row", lambda lib: ln(lib, ad, 0), 3 * row_bytes),
             ("ln_modulate + add    4 waves/row", lambda lib: ln(lib, ad, 1), 3 * row_bytes),
             ("qk_norm_rope", qk, 4 * row_bytes)]
    for name, fn, nbytes in cases:
        # the yardstick: a device copy that moves the same bytes (half read, half written), timed in the same rounds
        srcs = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(args.cold)]
        dsts = [torch.empty_like(t) for t in srcs]

        def copy():
            turn[0] = (turn[0] + 1) % args.cold
            dsts[turn[0]].copy_(srcs[turn[0]])
        runs = [(os.path.basename(p), (lambda lib=lib: fn(lib))) for p, lib in zip(libs, handles)] + [("copy", copy)]
        times = [[] for _ in runs]
        for _, run in runs:
            for _ in range(3):
                run()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for i, (_, run) in enumerate(runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    run()
                e1.record()
                torch.cuda.synchronize()
                times[i].append(e0.elapsed_time(e1) / args.reps * 1e3)
        for i, (label, _) in enumerate(runs):
            q1, med, q3 = quartiles(times[i])
            print(f"{name:42s} {label:24s} median {med:7.1f} us  {nbytes / med / 1e6:6.2f} TB/s   q1 {q1:7.1f}  q3 {q3:7.1f}  "
                  f"min {min(times[i]):7.1f}  max {max(times[i]):7.1f}", flush=True)
        for i in range(1, len(libs)):
            print(f"    {os.path.basename(libs[i])} vs {os.path.basename(libs[0])} (us): {gate(times[0], times[i])[1]}", flush=True)
        del srcs, dsts


if __name__ == "__main__":
    main()
