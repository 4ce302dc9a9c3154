#!/usr/bin/env python3
"""What the relight path costs, measured in one process with the arms alternated (medians of three rounds, the spread beside them;
nothing is set in advance).

    python tools/relightbench.py ingest [T Hs Ws Hd Wd]
        drn_fit_frames on an fp32 clip (the yardstick: the kernel as it was) against drn_fit_frames_u8 on the same clip as bytes,
        57 x 1080 x 1920 -> 576 x 1024 crop by default: the launch alone (device events), the call (tables uploaded, result
        allocated), and the call with the upload of the host clip inside; source + result bytes over the launch time.
    python tools/relightbench.py chain [T H W steps blocks]
        Full-size synthetic-weight nets (28 blocks), `steps` steps per stage (default 2), a 57 x 576 x 1024 clip on the host: the
        inverse node followed by the forward node (G-buffers through the host) against Cosmos1Relight (G-buffers stay on the
        device as bytes); wall time to the six host tensors and peak device memory above the resident models.

Not measured here: anything under sequence parallelism, and a relight of a windowed long clip.
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
fit = pkg.fit
dev = torch.device("cuda")


def spread(ms):
    return f"median {statistics.median(ms):9.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs)"


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


def ingest(T, Hs, Ws, Hd, Wd):
    assert torch.cuda.is_available(), "relightbench needs a GPU"
    g = torch.Generator().manual_seed(1)
    host_u8 = torch.randint(0, 256, (1, T, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    host_f32 = fit.u8_unit(host_u8)        # the same clip as ComfyUI hands it over: u8 / 255 in fp32
    plan = fit.plan_fit(T, Hs, Ws, "crop", Hd, Wd)
    dev_u8, dev_f32 = host_u8.to(dev), host_f32.to(dev)
    a = fit.fit_frames(dev_f32, plan, dev, backend="hip")
    b = fit.fit_frames(dev_u8, plan, dev, backend="hip")
    torch.cuda.synchronize()
    same = torch.equal(a, b)
    f32_mib, u8_mib, dst_mib = host_f32.numel() * 4 / 2**20, host_u8.numel() / 2**20, a.numel() * 2 / 2**20
    print(f"{T} x {Hs} x {Ws} -> {plan.T_out} x {plan.H_out} x {plan.W_out} crop (resized {plan.H_full} x {plan.W_full}, taps "
          f"{plan.y_w.shape[1]} x {plan.x_w.shape[1]}): source {f32_mib:.0f} MiB fp32 / {u8_mib:.0f} MiB uint8, result {dst_mib:.0f} "
          f"MiB bf16; drn_fit_frames_u8(bytes) == drn_fit_frames(u8 / 255) bit for bit: {same}")
    assert same
    del a, b
    tabs = [t.to(dev) for t in (plan.t_idx, plan.y_lo_n, plan.y_w, plan.x_lo_n, plan.x_w)]
    out = torch.empty((1, 3, plan.T_out, plan.H_out, plan.W_out), dtype=torch.bfloat16, device=dev)
    lib, stream = pkg.native.load_library(), torch.cuda.current_stream().cuda_stream

    def launcher(fn, src):
        def launch():
            rc = fn(src.data_ptr(), out.data_ptr(), 1, T, Hs, Ws, plan.T_out, plan.H_out, plan.W_out, tabs[0].data_ptr(),
                    tabs[1].data_ptr(), tabs[2].data_ptr(), plan.y_w.shape[1], tabs[3].data_ptr(), tabs[4].data_ptr(),
                    plan.x_w.shape[1], stream)
            assert rc == 0, rc
        return launch

    def alone(launch, n=20):               # n launches back to back between two device events -> ms per launch
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                launch()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n
        return run
    launches = [("drn_fit_frames     (fp32 source), launch alone", alone(launcher(lib.drn_fit_frames, dev_f32)), f32_mib),
                ("drn_fit_frames_u8  (uint8 source), launch alone", alone(launcher(lib.drn_fit_frames_u8, dev_u8)), u8_mib)]
    calls = [("fp32, call, frames on the device", lambda: fit.fit_frames(dev_f32, plan, dev, backend="hip")),
             ("uint8, call, frames on the device", lambda: fit.fit_frames(dev_u8, plan, dev, backend="hip")),
             ("fp32, call with the upload inside", lambda: fit.fit_frames(host_f32, plan, dev, backend="hip")),
             ("uint8, call with the upload inside", lambda: fit.fit_frames(host_u8, plan, dev, backend="hip"))]
    for _, run, _ in launches:
        run()
    per = {name: [] for name, _, _ in launches}
    runs = {name: [] for name, _ in calls}
    peaks = {}
    for _ in range(3):                     # alternated rounds
        for name, run, _ in launches:
            per[name].append(run())
        for name, fn in calls:
            ms, peak = timed(fn)
            runs[name] += ms
            peaks[name] = max(peaks.get(name, 0.0), peak)
    for name, _, src_mib in launches:
        k = statistics.median(per[name])
        print(f"{name:50s}: {k:.3f} ms per launch (device events, 20 launches; rounds {' '.join(f'{v:.3f}' for v in per[name])}) = "
              f"{(src_mib + dst_mib) / 1024 / (k / 1e3):.0f} GiB/s over its {src_mib + dst_mib:.0f} MiB of source + result bytes")
    for name, _ in calls:
        print(f"{name:50s}: {spread(runs[name])}  peak memory above the resident tensors {peaks[name]:8.1f} MiB")


def chain(T, H, W, steps, blocks):
    assert torch.cuda.is_available(), "relightbench needs a GPU"
    sw, cfgm = pkg.synthetic_weights, pkg.diffusion_renderer_config
    models = {}
    for kind, cfg in (("inverse", cfgm.get_inverse_renderer_config()), ("forward", cfgm.get_forward_renderer_config())):
        net = dict(cfg["net"], num_blocks=blocks)
        m = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(dict(cfg, net=net, model_type=kind), device=dev)
        sd = sw.synth_state_dict(net, torch.bfloat16, device=dev)
        m.load_state_dict(sd, strict=True)
        del sd
        models[kind] = m
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=dev), device=dev)
    pipe = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "synthetic.pt", model_type=None, vae_instance=vae, model_instance=models, guidance=0.0, num_steps=steps)
    torch.cuda.empty_cache()
    image = sw.synth_tensor("relight.image", (1, T, H, W, 3), torch.float32).mul(0.25).add(0.5).clamp(0.0, 1.0)      # host IMAGE
    env = sw.synth_tensor("relight.env", (1, 256, 512, 3), torch.float32).abs() * 4.0
    inverse, forward = pkg.nodes.Cosmos1InverseRenderer(), pkg.nodes.Cosmos1ForwardRenderer()
    relight = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    kw = dict()                            # fit off, the nodes' default: the clip is on the grid

    def two_nodes():
        g = inverse.run_inverse_pass(pipe, image, seed=3, **kw)
        g5 = [o.reshape(1, -1, *o.shape[1:]) for o in g]           # base_color, metallic, roughness, normal, depth
        (relit,) = forward.run_forward_pass(pipe, g5[4], g5[3], g5[2], g5[1], g5[0], env, seed=3, **kw)
        return (relit, *g)

    def one_node():
        return relight.run_relight(pipe, pipe, image, env, seed=3, **kw)
    arms = [("Cosmos1InverseRenderer -> host -> Cosmos1ForwardRenderer", two_nodes), ("Cosmos1Relight", one_node)]
    a, b = two_nodes(), one_node()         # warm-up of both arms, and the bits
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    print(f"{T} x {H} x {W}, {blocks} blocks, {steps} steps per stage, fit off: six outputs bit for bit "
          f"equal: {same}")
    assert same
    del a, b
    resident = torch.cuda.memory_allocated() / 2**30
    secs = {name: [] for name, _ in arms}
    peaks = {name: 0.0 for name, _ in arms}
    for _ in range(3):                     # alternated rounds, one run each
        for name, fn in arms:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            secs[name].append(time.perf_counter() - t0)
            peaks[name] = max(peaks[name], (torch.cuda.max_memory_allocated() - base) / 2**30)
            del out
    print(f"resident on the device (two models, tokenizer): {resident:.1f} GiB")
    for name, _ in arms:
        s = secs[name]
        print(f"{name:58s}: median {statistics.median(s):7.3f} s  (min {min(s):.3f}, max {max(s):.3f}, {len(s)} runs)  "
              f"peak device memory above the resident {peaks[name]:6.2f} GiB")
    m = {name: statistics.median(secs[name]) for name, _ in arms}
    print(f"difference of the medians: {m[arms[0][0]] - m[arms[1][0]]:+.3f} s "
          f"({100 * (m[arms[0][0]] - m[arms[1][0]]) / m[arms[0][0]]:+.1f} % of the two-node chain)")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "ingest"
    nums = [int(v) for v in sys.argv[2:]]
    if mode == "ingest":
        ingest(*(nums if len(nums) == 5 else [57, 1080, 1920, 576, 1024]))
    elif mode == "chain":
        chain(*(nums if len(nums) == 5 else [57, 576, 1024, 2, 28]))
    else:
        sys.exit(__doc__)
