#!/usr/bin/env python3
"""What a relight edit costs, measured in one process with the arms alternated (nothing is set in advance).

    python tools/editbench.py kernel [T H W]
        uint8 G-buffers [1, T, H, W, 3] (57 x 576 x 1024 by default) on the device, three edits - metallic and roughness under a
        mask; all five layers under a matte; both together - each through gbuffer_edit.edit_gbuffers' torch specification on the
        device and through the one launch of drn_gbuffer_edit_u8: device events, medians of 15 after a warm-up, arms alternating;
        peak device memory above the inputs; the bytes the edit needs (masks once, every touched map read and written, every
        layer read) over the time.  Random masks: no lane finds its 16 pixels untouched.  One more line: the full edit under
        masks that cover a quarter of the picture, where in place the kernel skips what it need not store.
    python tools/editbench.py whole [T H W steps blocks]
        Full-size synthetic-weight nets, `steps` steps per stage (default 2): Cosmos1Relight with the both-together edit against
        the default call; wall time to the six host tensors and peak device memory above the resident models.

Not measured here: anything under sequence parallelism, and picture quality with real weights.
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
E = pkg.gbuffer_edit
dev = torch.device("cuda")
RUNS = 15


def inputs(T, H, W, quarter=False):
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *shape: torch.randint(0, 256, shape, generator=g, dtype=torch.uint8, device=dev)
    maps = [rnd(1, T, H, W, 3) for _ in E.MAPS]
    layers = [rnd(1, T, H, W, 3) for _ in E.MAPS]
    if quarter:         # a box over a quarter of the picture with a soft rim of 32 pixels: most lanes see both masks 0
        y = torch.arange(H, device=dev).float()[:, None]
        x = torch.arange(W, device=dev).float()[None, :]
        d = torch.minimum(torch.minimum(y - H / 4, 3 * H / 4 - y), torch.minimum(x - W / 4, 3 * W / 4 - x))
        box = ((d / 32.0).clamp(0, 1) * 255).round().to(torch.uint8)
        em = box[None, None].expand(1, T, H, W).contiguous()
        im = em.clone()
    else:
        em, im = rnd(1, T, H, W), rnd(1, T, H, W)
    return maps, layers, em, im


def edits(layers, em, im):
    gain, offset = [[1.0] * 3 for _ in E.MAPS], [[0.0] * 3 for _ in E.MAPS]
    gain[1], offset[1] = [0.0] * 3, [255.0] * 3                 # fully metallic
    gain[2], offset[2] = [1.7] * 3, [7.3] * 3                   # rougher
    ident = ([[1.0] * 3 for _ in E.MAPS], [[0.0] * 3 for _ in E.MAPS])
    # (the edit, bytes per pixel it needs: the masks once, 3 + 3 per touched map, 3 per layer)
    return [("material (metallic, roughness under a mask)", E.GBufferEdit(gain, offset, em, [None] * 5, None), 1 + 2 * 6),
            ("insert (five layers under a matte)", E.GBufferEdit(*ident, None, list(layers), im), 1 + 5 * 9),
            ("both together", E.GBufferEdit(gain, offset, em, list(layers), im), 2 + 5 * 9)]


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    p = (torch.cuda.max_memory_allocated() - base) / 2**20
    del out
    return p


def measure(name, maps, edit, bpp, pixels):
    work = [m.clone() for m in maps]                            # the kernel edits in place: on copies, again and again
    spec = E.edit_gbuffers(maps, edit, backend="torch")
    got = E.edit_gbuffers([m.clone() for m in maps], edit, backend="hip")
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(spec, got))
    del spec, got
    arms = {"hip": (lambda: E.edit_gbuffers(work, edit, backend="hip"), 10), "torch": (lambda: E.edit_gbuffers(maps, edit, backend="torch"), 1)}
    ms = {k: [] for k in arms}
    for k, (fn, n) in arms.items():
        events(fn, n)                                           # warm-up
    for _ in range(RUNS):                                       # alternated
        for k, (fn, n) in arms.items():
            ms[k].append(events(fn, n))
    pk = {k: peak(fn) for k, (fn, _) in arms.items()}
    h, t = statistics.median(ms["hip"]), statistics.median(ms["torch"])
    need = bpp * pixels
    print(f"  {name:44s} one launch {h:7.3f} ms (min {min(ms['hip']):7.3f})  peak {pk['hip']:7.1f} MiB  "
          f"{need / 1e12 / (h / 1e3):5.2f} TB/s of the {need / 2**20:.0f} MiB it needs | torch path {t:8.3f} ms (min {min(ms['torch']):8.3f})  "
          f"peak {pk['torch']:7.0f} MiB | {t / h:6.1f}x | same bytes: {same}")
    assert same
    return h, t


def kernel(T, H, W):
    assert torch.cuda.is_available(), "editbench needs a GPU"
    print(f"# tools/editbench.py kernel on {torch.cuda.get_device_name(0)}; nothing was set in advance")
    print(f"G-buffers [1,{T},{H},{W},3] uint8 ({T * H * W * 3 / 2**20:.0f} MiB each), masks [1,{T},{H},{W}]; device events around 10 "
          f"launches (torch: one call), median of {RUNS} after a warm-up, arms alternating; peak = device memory above the inputs")
    maps, layers, em, im = inputs(T, H, W)
    for name, edit, bpp in edits(layers, em, im):
        measure(name, maps, edit, bpp, T * H * W)
    del em, im
    maps, layers, em, im = inputs(T, H, W, quarter=True)
    name, edit, bpp = edits(layers, em, im)[2]
    print("  masks over a quarter of the picture (in place, a lane whose 16 pixels have both masks 0 stores nothing; the rate is "
          "still over the bytes of the whole picture):")
    measure(name, maps, edit, bpp, T * H * W)


def whole(T, H, W, steps, blocks):
    assert torch.cuda.is_available(), "editbench needs a GPU"
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
    g = torch.Generator().manual_seed(9)
    mask = lambda: torch.rand(1, T, H, W, generator=g)                                                              # host MASKs
    layer = lambda: torch.rand(1, T, H, W, 3, generator=g)                                                          # host IMAGEs
    kw = dict(edit_mask=mask(), edit_metallic_gain=0.0, edit_metallic_offset=1.0, edit_roughness_gain=1.7, edit_roughness_offset=0.03,
              insert_mask=mask(), insert_base_color=layer(), insert_metallic=layer(), insert_roughness=layer(), insert_normal=layer(),
              insert_depth=layer())
    relight = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    arms = [("Cosmos1Relight, default call", lambda: relight.run_relight(pipe, pipe, image, env, seed=3)),
            ("Cosmos1Relight, material edit + five layers", lambda: relight.run_relight(pipe, pipe, image, env, seed=3, **kw))]
    for _, fn in arms:
        fn()                                                    # warm-up
    print(f"# tools/editbench.py whole on {torch.cuda.get_device_name(0)}")
    print(f"{T} x {H} x {W}, {blocks} blocks, {steps} steps per stage, fit off; the edit's two masks and five layers are host fp32 "
          f"tensors at full size ({(2 + 15) * T * H * W * 4 / 2**30:.1f} GiB), uploaded inside the call")
    secs = {name: [] for name, _ in arms}
    peaks = {name: 0.0 for name, _ in arms}
    for _ in range(3):                                          # alternated rounds, one run each
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
    for name, _ in arms:
        s = secs[name]
        print(f"{name:46s}: median {statistics.median(s):7.3f} s  (min {min(s):.3f}, max {max(s):.3f}, {len(s)} runs)  "
              f"peak device memory above the resident {peaks[name]:6.2f} GiB")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(v) for v in sys.argv[2:]]
    if mode == "kernel":
        kernel(*(nums if len(nums) == 3 else [57, 576, 1024]))
    elif mode == "whole":
        whole(*(nums if len(nums) == 5 else [57, 576, 1024, 2, 28]))
    else:
        sys.exit(__doc__)
