"""Per-rank compute of the sequence-parallel DiT forward, measured on ONE GPU: the exchanges are replaced by no-ops, so the
kernels run on rank 0's shapes (token band of S/world rows, heads/world heads after the all-to-all); the peers' data is
faked by device copies of this rank's own slabs (same value distribution; the copies cost ~0.02 ms per exchange).
What it shows: the compute floor of `bench.py --gpus N` and which kernels lose efficiency at the per-rank shapes.

    python tools/rankbench.py --world 8 [--exchange a2a|gather] [--steps 4]
    python tools/rankbench.py --world 8 --precision mxfp8 [--attention-precision mxfp8] --compare 3
        (--compare n: a bf16 engine is built beside the chosen one and the two are timed alternately, n rounds, in this process)
"""
import argparse
import os
import sys
import tempfile
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402


def tokenizer_band(pkg, args, dev):
    """One rank's row band of the tokenizer (rank 1: both neighbours exist); gathers are faked by device copies."""
    world = args.world
    sw = pkg.synthetic_weights
    pkg.parallel.allgather_stack = lambda local, group=None: local.unsqueeze(0).expand(world, *local.shape).contiguous()
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=dev), device=dev)
    clip = sw.synth_tensor("rb.rgb", (1, 3, args.frames, args.height, args.width), torch.float32, device=dev).to(torch.bfloat16)
    res = {}
    for w_ in (1, world):
        vae.model.rank, vae.model.world, vae.model.pg = (min(1, w_ - 1), w_, None)
        z = vae.encode(clip)
        vae.decode(z)
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        z = vae.encode(clip)
        e[1].record()
        vae.decode(z)
        e[2].record()
        torch.cuda.synchronize()
        res[w_] = (e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]))
    print(f"tokenizer {args.frames}f x {args.height} x {args.width}: one GPU encode {res[1][0]:.2f} ms decode {res[1][1]:.2f} ms; "
          f"one band of {world}: encode {res[world][0]:.2f} ms decode {res[world][1]:.2f} ms (exchanges faked by device copies)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--exchange", default="a2a")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=57)
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=28)
    ap.add_argument("--tokenizer", action="store_true", help="time this rank's band of the tokenizer instead of the DiT")
    ap.add_argument("--clips", type=int, default=1, help="clips stepped as one sharded batch (the node's 5 G-buffer passes)")
    ap.add_argument("--precision", choices=("bf16", "mxfp8"), default="bf16", help="block linears (HipDiT precision)")
    ap.add_argument("--attention-precision", choices=("bf16", "mxfp8"), default="bf16", help="self-attention (HipDiT attention_precision)")
    ap.add_argument("--compare", type=int, default=0, metavar="ROUNDS",
                    help="also build the bf16 / bf16 engine and time the two alternately for this many rounds")
    ap.add_argument("--checksum", action="store_true", help="print the int16 sum of the last forward's output (A/B runs of two trees)")
    args = ap.parse_args()
    os.environ["DRN_SP_EXCHANGE"] = args.exchange
    pkg = load_package()
    eng, N = pkg.dit_engine, pkg.native
    world = args.world
    eng.group_info = lambda pg=None: (0, world)

    def fake_alltoall(send, recv, pg=None, async_op=False):
        if isinstance(send, (tuple, list)):                      # MXFP8: elements and scales
            for s_, r_ in zip(send, recv):
                r_.copy_(s_)
            return
        recv.copy_(send)

    def fake_allgather(full, plan, pg=None, async_op=False):
        if full.shape[0] == plan.S and plan.world > 1:
            full.view(plan.world, plan.rows, -1)[1:].copy_(plan.band(full).unsqueeze(0).expand(plan.world - 1, -1, -1))

    def fake_bands(send, recv, lo, hi, pg=None, async_op=False):
        if isinstance(send, (tuple, list)):
            for s_, r_ in zip(send, recv):
                fake_bands(s_, r_, lo, hi)
            return
        if hi > lo:
            recv[lo:hi].copy_(send[lo:hi])

    eng.alltoall_rows_ = fake_alltoall
    eng.alltoall_bands_ = fake_bands
    eng.allgather_rows_ = fake_allgather
    dev = torch.device("cuda", 0)
    if args.tokenizer:
        return tokenizer_band(pkg, args, dev)
    cfg = pkg.diffusion_renderer_config.get_inverse_renderer_config(args.height, args.width, args.frames)
    net = dict(cfg["net"], num_blocks=args.blocks)
    sw = pkg.synthetic_weights
    sd = sw.synth_state_dict(net, torch.bfloat16, device=dev)
    # the engine wants a torch.distributed group for the MXFP8 modes: a 1-rank gloo group is the handle, no collective runs on it
    rdv = tempfile.NamedTemporaryFile(prefix="rankbench_", delete=False)
    rdv.close()
    os.unlink(rdv.name)
    dist.init_process_group("gloo", init_method=f"file://{rdv.name}", rank=0, world_size=1)
    pg = dist.group.WORLD
    dit = eng.HipDiT(net, sd, device=dev, process_group=pg, precision=args.precision,
                     attention_precision=args.attention_precision)
    base = None
    if args.compare and (args.precision, args.attention_precision) != ("bf16", "bf16"):
        base = eng.HipDiT(net, sd, device=dev, process_group=pg, precision="bf16", attention_precision="bf16")
    del sd
    torch.cuda.empty_cache()
    F_, h, w = (args.frames - 1) // 8 + 1, args.height // 8, args.width // 8
    x = sw.synth_tensor("rb.x", (args.clips, 16, F_, h, w), torch.float32, device=dev, scale=2.0).to(torch.bfloat16)
    cond = sw.synth_tensor("rb.c", (args.clips, 16, F_, h, w), torch.float32, device=dev, scale=1.0).to(torch.bfloat16)
    sig = [80.0 * 0.8 ** i for i in range(args.steps + 1)]
    tag = f"linears {args.precision} attention {args.attention_precision}"

    def timed(d):
        """(ms per forward, host enqueue ms per forward) over --steps forwards after one warm-up."""
        d.prepare_timesteps(sig)
        d(x, sig[0], cond, 3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s_ in sig[1:]:
            d(x, s_, cond, 3)
        host = (time.perf_counter() - t0) / args.steps * 1e3     # host time to ENQUEUE a forward (must stay below the GPU time)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, host

    ms, host_ms = timed(dit)
    if base is not None:
        rows = {"bf16": [], tag: []}
        for _ in range(args.compare):                            # alternated: drift of the box hits both alike
            rows["bf16"].append(timed(base)[0])
            rows[tag].append(timed(dit)[0])
        for name, v in rows.items():
            print(f"  {name:40s} ms per forward, per round: {' '.join(f'{t:8.2f}' for t in v)}   median {sorted(v)[len(v) // 2]:8.2f}")
        del base
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dit(x, sig[1], cond, 3)
    one_ms = (time.perf_counter() - t0) * 1e3                      # empty queue: pure host cost of one forward
    torch.cuda.synchronize()
    print(f"host cost of one forward on an empty queue: {one_ms:.2f} ms")
    timer = N.KernelTimer(sample_every=3)
    N.set_timer(timer)
    y = dit(x, sig[1], cond, 3)
    torch.cuda.synchronize()
    N.set_timer(None)
    if args.checksum:
        print(f"checksum {int(y.view(torch.int16).sum(dtype=torch.int64))}")
    print(f"world={world} exchange={dit.exchange} clips={args.clips} {tag} path={dit.sp_path}: {ms:.2f} ms per forward on this rank's "
          f"shapes (no communication); host enqueue {host_ms:.2f} ms per forward")
    for name, d in timer.summary().items():
        n = d["launches_seen"]
        print(f"  {name:10s} {n:4d} launches  avg {d['ms_avg']:.3f} ms  -> {d['ms_avg'] * n:7.2f} ms per forward, "
              f"{d['flops'] / d['ms_total'] / 1e9:7.1f} TF/s")
    # bytes that leave this rank per self-attention layer (to the world - 1 peers), before (bf16) and with the chosen precisions
    S, D = F_ * (h // 2) * (w // 2), net["model_channels"]
    out = (world - 1) * (S // world) // world if dit.exchange == "a2a" else (world - 1) * (S // world)     # rows sent x columns / D
    mxb = 1 + 1 / 32                                             # e4m3 element + its share of the E8M0 scale byte
    if dit.exchange == "a2a":
        ex = {"k|v out": (4 * D, 4 * D), "q out": (2 * D, 2 * D),
              "o return": (2 * D, mxb * D if (dit.sp_path or {}).get("return") == "e4m3" else 2 * D)}
    else:
        amx = (dit.sp_path or {}).get("attention") == "mxfp8"
        ex = {"k gather": (2 * D, mxb * D if amx else 2 * D), "v gather": (2 * D, 2 * D)}
    for name, (b0, b1) in ex.items():
        print(f"  exchange {name:9s}: {out * b0 / 1e6:8.2f} MB per layer and rank in bf16 -> {out * b1 / 1e6:8.2f} MB here")
    print(f"  exchange total    : {out * sum(b for b, _ in ex.values()) / 1e6:8.2f} MB -> {out * sum(b for _, b in ex.values()) / 1e6:8.2f} MB")
    dist.destroy_process_group()

if __name__ == "__main__":
    main()
