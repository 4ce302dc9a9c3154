#!/usr/bin/env python3
"""MXFP8 against bf16 on one box, interleaved in ONE process (CDNA guide rule 24), random data.
    python tools/mxbench.py [gemm] [model] [attn] [--M ROWS] [--rounds R] [--cold C] [--sweep]
gemm:  the four block linears at M rows (default 18 432 = cfg 3): what native.gemm runs in bf16 against drn_mx_quant_bf16 of the
       activation + drn_gemm_mxfp8 (and each of the two alone); the quantiser in GB/s against the HBM peak.
       --M 256 / --M 1024 (few tokens): also quantise + what native.gemm_mxfp8 picks (the few-token kernel of gemm_mx_tall.hip,
       its reduce launch included where it slices K) against quantise + drn_gemm_mxfp8 (the small-M path off); the weight copies
       are rotated over more than the 256 MB Infinity Cache.  --sweep adds both tile shapes at every power-of-two slice count.
       Then, per producer that can write MXFP8 itself (LayerNorm + modulate -> q|k|v, attention -> out-proj, MLP-up's GELU ->
       MLP-down): "producer + quantise launch + GEMM" against "fused producer + GEMM" (the same bits; drn.h).
model: ms per step (DiT forward + Euler step) of the 28-block model at cfg 3 (57 x 576 x 1024, S = 18 432) and cfg 1 (256 x 256,
       S = 256) with precision bf16, mxfp8, and mxfp8 built under DRN_PER_LAUNCH=1 (one ctypes call per kernel; at cfg 1 also
       with the small-M path off: the path of an mxfp8 engine before gemm_mx_tall.hip), and mxfp8 built under DRN_MX_FUSED=0 (a
       quantise launch in front of every block linear: the launches of an mxfp8 engine before the fused producers), synthetic
       weights; and both precisions of the block linears with attention_precision="mxfp8" (the MXFP8 self-attention).
attn:  one self-attention site of the 32-head model at S = 256, 1024, 2048 and 18 432 tokens: qk_norm_rope + attention on the bf16
       16x16x32 body (the yardstick) against qk_norm_rope_mx + mx_quant_vt + attention_mxfp8 (the two producer launches counted),
       each under the attention plan of its shape, interleaved; every run is printed, then median and max - min spread."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

HBM_PEAK_GBS = 8000.0
SHAPES = [("qkv", 12288, 4096, 0), ("out-proj", 4096, 4096, 2), ("mlp-up", 16384, 4096, 1), ("mlp-down", 4096, 16384, 2)]


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def bench_gemm(pkg, args):
    N = pkg.native
    dev = torch.device("cuda")
    M = args.M
    g = torch.Generator(device="cpu").manual_seed(0)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)

    lib = N.load_library()
    few = M <= 1024 and M % 256 == 0
    print(f"# GEMM, M = {M}, {args.rounds} interleaved rounds x {args.reps} launches, weights rotated over >= {args.cold} copies")
    for name, n, k, epi in SHAPES:
        a = rnd(M, k)
        # few tokens: the product is a weight stream, so the fp8 copies together must not fit the 256 MB Infinity Cache
        cold = max(args.cold, -(-600_000_000 // (n * k))) if few else args.cold
        w0 = rnd(n, k, scale=k ** -0.5)
        ws = [w0] + [w0.clone() for _ in range(cold - 1)]
        wqs = [N.mx_quant(w) for w in ws]
        out = torch.empty(M, n, dtype=torch.bfloat16, device=dev)
        gate = rnd(1, n, scale=0.5) if epi == 2 else None
        res = rnd(M, n) if epi == 2 else None
        aq = N.mx_quant(a)
        it = {"i": 0}

        def nxt():
            it["i"] = (it["i"] + 1) % cold
            return it["i"]

        def run_bf16():
            N.gemm(a, ws[nxt()], out=out, epilogue=epi, gate=gate, residual=res)

        def run_quant():
            N.mx_quant(a, out=aq)

        def run_mx():
            N.gemm_mxfp8(aq, wqs[nxt()], out=out, epilogue=epi, gate=gate, residual=res, splitk=0)

        def run_both():
            N.mx_quant(a, out=aq)
            N.gemm_mxfp8(aq, wqs[nxt()], out=out, epilogue=epi, gate=gate, residual=res, splitk=0)

        def small(shape, splits):
            def run():
                lib.drn_gemm_mxfp8_tall_force_shape(shape)
                N.mx_quant(a, out=aq)
                N.gemm_mxfp8(aq, wqs[nxt()], out=out, epilogue=epi, gate=gate, residual=res, splitk=splits)
            return run

        cases = [("bf16", run_bf16), ("quant", run_quant), ("mxfp8", run_mx), ("quant+mxfp8", run_both)]
        plan = N.mx_gemm_plan(M, n, k) if few else 0
        if plan:
            cases.append(("quant+small-M", small(-1, None)))
            if args.sweep:
                for shape in (0, 1):
                    cases += [(f"shape{shape} s={sp}", small(shape, sp)) for sp in (1, 2, 4, 8, 16) if (k // 128) % sp == 0]
        for _, f in cases:
            timed(f, 3)
        t = {c: [] for c, _ in cases}
        for _ in range(args.rounds):
            for c, f in cases:
                t[c].append(timed(f, args.reps))
        med = {c: sorted(v)[len(v) // 2] for c, v in t.items()}
        fl = 2.0 * M * n * k
        qbytes = M * k * 2 + M * k + M * k / 32
        print(f"{name:9s} N={n:5d} K={k:5d}: bf16 {med['bf16']:.3f} ms ({fl / med['bf16'] / 1e9:.0f} TF) | "
              f"mxfp8 {med['mxfp8']:.3f} ms ({fl / med['mxfp8'] / 1e9:.0f} TF) | quant {med['quant']:.3f} ms "
              f"({qbytes / med['quant'] / 1e6:.0f} GB/s = {qbytes / med['quant'] / 1e6 / HBM_PEAK_GBS:.2f} of HBM peak) | "
              f"quant+mxfp8 {med['quant+mxfp8']:.3f} ms = {med['quant+mxfp8'] / med['bf16']:.3f} x bf16")
        if plan:
            sm = med["quant+small-M"]
            print(f"          few-token path ({plan} slice{'s' if plan > 1 else ''}{', reduce launch included' if plan > 1 else ''}, {cold} weight "
                  f"copies): quant+small-M {sm * 1e3:.1f} us = {sm / med['bf16']:.3f} x bf16 ({med['bf16'] * 1e3:.1f} us) = "
                  f"{sm / med['quant+mxfp8']:.3f} x quant+drn_gemm_mxfp8 ({med['quant+mxfp8'] * 1e3:.1f} us); quant alone "
                  f"{med['quant'] * 1e3:.1f} us")
            if args.sweep:
                print("          sweep (quant + kernel [+ reduce], us): "
                      + "  ".join(f"{c} {med[c] * 1e3:.1f}" for c, _ in cases if c.startswith("shape")))
            lib.drn_gemm_mxfp8_tall_force_shape(-1)
        del ws, wqs, a, aq, out, gate, res
        torch.cuda.empty_cache()


def bench_producers(pkg, args):
    """producer + drn_mx_quant_bf16 + consumer GEMM against fused producer + consumer GEMM, at M rows of the D = 4096 model."""
    N = pkg.native
    dev = torch.device("cuda")
    M, D, Hd, heads = args.M, 4096, 16384, 32
    g = torch.Generator(device="cpu").manual_seed(1)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)

    cold = max(args.cold, 3)
    wq = {n: [N.mx_quant(rnd(nn, kk, scale=kk ** -0.5)) for _ in range(cold)]
          for n, nn, kk in (("qkv", 3 * D, D), ("out", D, D), ("up", Hd, D), ("down", D, Hd))}
    it = {"i": 0}

    def nxt():
        it["i"] = (it["i"] + 1) % cold
        return it["i"]

    x, shift, scale = rnd(M, D), rnd(1, D, scale=0.3), rnd(1, D, scale=0.3)
    h, hmx = torch.empty_like(x), N.mx_empty(M, D, dev)
    qkv = rnd(1, M, 3 * D)
    q, k, v = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
    o, omx = torch.empty(1, M, D, dtype=torch.bfloat16, device=dev), N.mx_empty(M, D, dev)
    u, umx = torch.empty(M, Hd, dtype=torch.bfloat16, device=dev), N.mx_empty(M, Hd, dev)
    qkv_out = torch.empty(M, 3 * D, dtype=torch.bfloat16, device=dev)
    gate, res = rnd(1, D, scale=0.5), rnd(M, D)
    xo = torch.empty_like(res)                           # gated-residual output (not `res`: it would grow with every repetition)
    aq = N.mx_quant(x)
    up_fusable = N.mx_gemm_plan(M, Hd, D) <= 1

    def ln_sep():
        N.ln_modulate(x, shift, scale, out=h)
        N.mx_quant(h, out=hmx)
        N.gemm_mxfp8(hmx, wq["qkv"][nxt()], out=qkv_out)

    def ln_fused():
        N.ln_modulate(x, shift, scale, out_mx=hmx)
        N.gemm_mxfp8(hmx, wq["qkv"][nxt()], out=qkv_out)

    def at_sep():
        N.attention(q, k, v, out=o, heads=heads)
        N.mx_quant(o.view(M, D), out=omx)
        N.gemm_mxfp8(omx, wq["out"][nxt()], out=xo, epilogue=N.EPI_GATE_RES, gate=gate, residual=res)

    def at_fused():
        N.attention(q, k, v, heads=heads, out_mx=omx)
        N.gemm_mxfp8(omx, wq["out"][nxt()], out=xo, epilogue=N.EPI_GATE_RES, gate=gate, residual=res)

    def up_sep():
        N.gemm_mxfp8(aq, wq["up"][nxt()], out=u, epilogue=N.EPI_GELU)
        N.mx_quant(u, out=umx)
        N.gemm_mxfp8(umx, wq["down"][nxt()], out=xo, epilogue=N.EPI_GATE_RES, gate=gate, residual=res)

    def up_fused():
        N.gemm_mxfp8(aq, wq["up"][nxt()], epilogue=N.EPI_GELU, out_mx=umx)
        N.gemm_mxfp8(umx, wq["down"][nxt()], out=xo, epilogue=N.EPI_GATE_RES, gate=gate, residual=res)

    cases = [("LayerNorm -> q|k|v", ln_sep, ln_fused)]
    if N.attention_mx_available():
        cases.append(("attention -> out-proj", at_sep, at_fused))
    if up_fusable:
        cases.append(("MLP-up GELU -> MLP-down", up_sep, up_fused))
    print(f"# producers, M = {M}: producer + quantise launch + GEMM | fused producer + GEMM, medians of {args.rounds} interleaved rounds")
    for name, sep, fused in cases:
        for f in (sep, fused):
            timed(f, 3)
        t = {"sep": [], "fused": []}
        for _ in range(args.rounds):
            t["sep"].append(timed(sep, args.reps))
            t["fused"].append(timed(fused, args.reps))
        ms, mf = sorted(t["sep"])[args.rounds // 2], sorted(t["fused"])[args.rounds // 2]
        print(f"{name:24s}: {ms * 1e3:8.1f} us | {mf * 1e3:8.1f} us ({(mf - ms) * 1e3:+.1f} us, {mf / ms:.3f} x); "
              f"spread {min(t['sep']) * 1e3:.1f}..{max(t['sep']) * 1e3:.1f} | {min(t['fused']) * 1e3:.1f}..{max(t['fused']) * 1e3:.1f}")


def bench_attn(pkg, args):
    N = pkg.native
    dev = torch.device("cuda")
    heads, D = 32, 4096
    g = torch.Generator(device="cpu").manual_seed(2)
    wq = torch.randn(128, generator=g).to(torch.bfloat16).to(dev)
    wk = torch.randn(128, generator=g).to(torch.bfloat16).to(dev)
    kt, thr, pexp = N.attention_mxfp8_params()
    print(f"# attention, heads {heads}: bf16 = qk_norm_rope + attention (16x16x32 body) | mxfp8 = qk_norm_rope_mx + mx_quant_vt + "
          f"attention_mxfp8 (key tile {kt}, rescale threshold {thr:g}, pexp {pexp}); {args.rounds} interleaved rounds")
    for S in (256, 1024, 2048, 18432):
        src = (torch.randn(S, 3 * D, generator=g)).to(torch.bfloat16).to(dev)
        qkv = src.clone()
        ang = torch.rand(S, 128, generator=g) * 6.28
        cos, sin = ang.cos().to(torch.bfloat16).to(dev), ang.sin().to(torch.bfloat16).to(dev)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        o = torch.empty(1, S, D, dtype=torch.bfloat16, device=dev)
        qm, km = N.mx_empty(S, D, dev), N.mx_empty(S, D, dev)
        vtvs = N.mx_quant_vt(v.unsqueeze(0), heads)

        def run_bf16():
            N.qk_norm_rope(q, k, wq, wk, cos, sin, heads)            # (in place: the values drift towards the norm's fixed point;
            N.attention(q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), out=o, heads=heads)     #  the time does not depend on them)

        def run_mx():
            N.qk_norm_rope_mx(q, k, wq, wk, cos, sin, heads, out_q=qm, out_k=km)
            N.mx_quant_vt(v.unsqueeze(0), heads, out=vtvs)
            N.attention_mxfp8(qm, km, vtvs[0], vtvs[1], 1, S, S, out=o)

        def run_mx_kernel():
            N.attention_mxfp8(qm, km, vtvs[0], vtvs[1], 1, S, S, out=o)

        def run_bf16_kernel():
            N.attention(q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), out=o, heads=heads)

        cases = [("bf16", run_bf16), ("mxfp8", run_mx), ("bf16 kernel alone", run_bf16_kernel), ("mxfp8 kernel alone", run_mx_kernel)]
        reps = args.reps if S >= 18432 else 5 * args.reps
        for _, f in cases:
            timed(f, 3)
        t = {c: [] for c, _ in cases}
        for _ in range(args.rounds):
            for c, f in cases:
                qkv.copy_(src)
                t[c].append(timed(f, reps))
        med = {c: sorted(v)[len(v) // 2] for c, v in t.items()}
        spread = max(t["bf16"]) - min(t["bf16"])
        print(f"S={S:5d} plan {N.attention_plan(1, heads, S, S)}")
        for c, _ in cases:
            print(f"    {c:18s}: runs " + " ".join(f"{x:.4f}" for x in t[c]) + f" ms | median {med[c]:.4f} ms")
        fl = 4.0 * heads * S * S * 128
        print(f"    median mxfp8 - bf16 = {med['mxfp8'] - med['bf16']:+.4f} ms ({med['mxfp8'] / med['bf16']:.3f} x); bf16 spread (max - min) "
              f"{spread:.4f} ms; kernels alone: bf16 {fl / med['bf16 kernel alone'] / 1e9:.0f} TF, mxfp8 {fl / med['mxfp8 kernel alone'] / 1e9:.0f} TF; "
              f"faster by more than the spread: {'yes' if med['bf16'] - med['mxfp8'] > spread else 'no'}")
        del src, qkv, o, qm, km, vtvs
        torch.cuda.empty_cache()


def bench_model(pkg, args):
    N = pkg.native
    dev = torch.device("cuda")
    sw = pkg.synthetic_weights
    net = dict(pkg.diffusion_renderer_config.get_inverse_renderer_config()["net"], model_channels=4096, num_blocks=28, num_heads=32)
    sd = sw.synth_state_dict(net, torch.bfloat16, device=dev)
    dits = {}
    for prec in ("bf16", "mxfp8"):
        dits[prec] = pkg.dit_engine.HipDiT(net, sd, device=dev, precision=prec)
    os.environ["DRN_PER_LAUNCH"] = "1"                   # read at construction
    dits["mxfp8 per-launch"] = pkg.dit_engine.HipDiT(net, sd, device=dev, precision="mxfp8")
    del os.environ["DRN_PER_LAUNCH"]
    os.environ["DRN_MX_FUSED"] = "0"                     # read at construction: a quantise launch per block linear
    dits["mxfp8 DRN_MX_FUSED=0"] = pkg.dit_engine.HipDiT(net, sd, device=dev, precision="mxfp8")
    del os.environ["DRN_MX_FUSED"]
    lib0 = N.load_library()
    lib0.drn_attention_mxfp8_force(1)                    # every site on the MXFP8 kernels (the engine's own rule keeps bf16 below 2048 tokens)
    for prec in ("bf16", "mxfp8"):                       # the MXFP8 self-attention switch, under both precisions of the block linears
        dits[f"{prec} + attention mxfp8"] = pkg.dit_engine.HipDiT(net, sd, device=dev, precision=prec, attention_precision="mxfp8")
    lib = N.load_library()
    del sd
    torch.cuda.empty_cache()
    for cfg, (F_, h, w) in (("cfg3", (8, 72, 128)), ("cfg1", (1, 32, 32))):
        x = sw.synth_tensor("mxb.x", (1, 16, F_, h, w), torch.float32, scale=2.0).to(torch.bfloat16).to(dev)
        cond = sw.synth_tensor("mxb.c", (1, 16, F_, h, w), torch.float32).to(torch.bfloat16).to(dev)
        xs = x.clone()
        for d in dits.values():
            d.prepare_timesteps([1.5])

        def step(d, small_m=1):
            lib.drn_gemm_mxfp8_force_small_m(small_m)
            y = d(xs, 1.5, cond, 0)
            N.edm_step(y, xs, 0.9, 0.1, 1.5, -0.05)
            lib.drn_gemm_mxfp8_force_small_m(1)

        runs = {p: (lambda d=d: step(d)) for p, d in dits.items()}
        if cfg == "cfg1":
            runs["mxfp8 per-launch, small-M off"] = lambda: step(dits["mxfp8 per-launch"], 0)
        for f in runs.values():
            f()
        torch.cuda.synchronize()
        reps = args.model_reps if cfg == "cfg3" else 5 * args.model_reps
        t = {p: [] for p in runs}
        for _ in range(args.rounds):
            for p, f in runs.items():
                t[p].append(timed(f, reps))
        med = {p: sorted(v)[len(v) // 2] for p, v in t.items()}
        print(f"# model {cfg} (latent {F_}x{h}x{w}): bf16 {med['bf16']:.2f} ms/step | mxfp8 {med['mxfp8']:.3f} ms/step "
              f"({100 * (1 - med['mxfp8'] / med['bf16']):+.1f} % lower) | "
              + " | ".join(f"{p} {v:.3f}" for p, v in med.items() if p not in ("bf16", "mxfp8"))
              + " | spread (min..max) " + ", ".join(f"{p} {min(v):.3f}..{max(v):.3f}" for p, v in t.items()))
        for base in ("bf16", "mxfp8"):
            on, off = f"{base} + attention mxfp8", base
            spread = max(t[off]) - min(t[off])
            print(f"#   attention mxfp8 under {base} linears: runs " + " ".join(f"{v:.3f}" for v in t[on]) + f" | switch off runs "
                  + " ".join(f"{v:.3f}" for v in t[off]) + f" | median {med[on]:.3f} vs {med[off]:.3f} ms/step, spread of the switch-off "
                  f"runs {spread:.3f}: faster by more than the spread: {'yes' if med[off] - med[on] > spread else 'no'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["gemm", "model"])
    ap.add_argument("--M", type=int, default=18432)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--model-reps", type=int, default=3)
    ap.add_argument("--cold", type=int, default=3, help="gemm: rotate over this many weight copies (HBM, not Infinity Cache)")
    ap.add_argument("--sweep", action="store_true", help="gemm at few tokens: both tile shapes x slice counts of the few-token kernel")
    args = ap.parse_args()
    pkg = load_package()
    pkg.native.load_library()
    print(f"# device {torch.cuda.get_device_name()}")
    if "gemm" in args.what:
        bench_gemm(pkg, args)
        bench_producers(pkg, args)
    if "attn" in args.what:
        bench_attn(pkg, args)
    if "model" in args.what:
        bench_model(pkg, args)


if __name__ == "__main__":
    main()
