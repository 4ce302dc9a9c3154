"""drn_fit_frames (the fp32 instantiation of csrc/fit.hip's kernel, on csrc/resample_core.h) on the GPU: the kernel against the
float64 reference under the bound of tests/fit_refs.py (whose wrong stand-ins tests/test_fit_cpu.py shows to miss it), bit for bit
against today's ingest at scale 1, bit for bit where a tile is cut into one chunk per row, its argument checks, and both renderer
nodes with fit against the composition done by hand."""
import importlib

import numpy as np
import pytest
import torch

import fit_refs as R
from conftest import tiny_net

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD, SENTINEL = 64, 0xA5          # 64 bytes keep the guarded output 16-byte aligned
DRN_EINVAL = -1


def _launch(pkg, gpu, src, plan):
    """The kernel into a guard-banded buffer, issued twice (a rerun over its own output changes nothing) -> the result on the CPU;
    the guard bands are checked here."""
    B = src.shape[0]
    shape = (B, 3, plan.T_out, plan.H_out, plan.W_out)
    n = 2 * int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    out = buf[GUARD:GUARD + n].view(BF).view(shape)
    for _ in range(2):
        pkg.native.fit_frames(src, plan.t_idx, plan.y_lo_n, plan.y_w, plan.x_lo_n, plan.x_w, out=out)
    host = buf.cpu()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all(), "wrote outside its output"
    return host[GUARD:GUARD + n].view(BF).view(shape)


@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=R.GEOMETRY_IDS)
def test_kernel_meets_the_bound(pkg, gpu, gi):
    fit = R.fit_module(pkg)
    worst = 0.0
    for _, B, T in R.grid([gi]):
        c = R.case(pkg, gi, B, T)
        src = c["src"].to(gpu)
        got = _launch(pkg, gpu, src, c["plan"])
        ok, ratio = R.bound_excess(got.double(), c["ref64"], c["e_ref"])
        print(f"fit parity {c['name']}: E_ref {c['e_ref']:.3e}, max((|hip - ref64| - 0.5 ulp)+ / E_ref) = {ratio:.3f}")
        assert ok, (c["name"], ratio)
        worst = max(worst, ratio)
        if gi in R.SCALE1:
            # identity and pure crop, with and without time padding: today's ingest on the cropped frames, and the torch backend
            p = c["plan"]
            frames = c["src"][:, p.t_idx.long(), p.y0:p.y0 + p.H_out, p.x0:p.x0 + p.W_out]
            assert torch.equal(got, R.todays_ingest(frames)), c["name"]
            assert torch.equal(got, fit.fit_frames(c["src"], p, gpu, backend="torch").cpu()), c["name"]
            assert torch.equal(got, fit.fit_frames(c["src"], p, gpu).cpu()), c["name"]            # auto = the kernel on a GPU
    print(f"fit parity {R.GEOMETRY_IDS[gi]}: worst ratio {worst:.3f} (bound {R.M_BOUND})")


def test_kernel_source_off_a_16_byte_boundary(pkg, gpu):
    for gi in (0, 5):
        c = R.case(pkg, gi, 2, 3)
        src = c["src"].to(gpu)
        flat = torch.empty(src.numel() + 1, dtype=torch.float32, device=gpu)
        assert flat.data_ptr() % 16 == 0
        flat[1:] = src.reshape(-1)
        shifted = flat[1:].view(src.shape)
        assert shifted.data_ptr() % 16 == 4
        assert torch.equal(_launch(pkg, gpu, shifted, c["plan"]), _launch(pkg, gpu, src, c["plan"]))


def test_scattered_row_taps_cut_a_tile_into_one_chunk_per_row(pkg, gpu):
    """No two consecutive output rows fit the stage together (fit_refs.scattered_rows), so the 16-row tile is 16 chunks.  Source
    values are multiples of 1/256 and all weights dyadic: every fp32 product and sum is exact, the only rounding on either side is
    the last one to bf16, and the float64 evaluation is the kernel's result bit for bit."""
    plan, my, mx = R.scattered_rows()
    g = torch.Generator().manual_seed(20261019)
    src = torch.randint(0, 257, (1, 2, 120, 40, 3), generator=g).float() / 256.0
    want = R.apply64(src, my, mx, plan.t_idx.long()) * 2.0 - 1.0
    assert want.shape == (1, 3, 3, 16, 32) and torch.equal(want.float().double(), want)       # exact in fp32 before the rounding
    got = _launch(pkg, gpu, src.to(gpu), plan)
    assert torch.equal(got, want.float().to(BF))


def test_kernel_argument_checks(pkg, gpu):
    lib = pkg.native.load_library()
    c = R.case(pkg, 0, 1, 3)
    p = c["plan"]
    src = c["src"].to(gpu)
    tabs = [t.to(gpu) for t in (p.t_idx, p.y_lo_n, p.y_w, p.x_lo_n, p.x_w)]
    n = 2 * 3 * p.T_out * p.H_out * p.W_out
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    out = buf[GUARD:].data_ptr()
    assert out % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    base = dict(src=src.data_ptr(), dst=out, B=1, Ts=3, Hs=p.H, Ws=p.W, Td=p.T_out, Hd=p.H_out, Wd=p.W_out,
                t_idx=tabs[0].data_ptr(), y_lo_n=tabs[1].data_ptr(), y_w=tabs[2].data_ptr(), Ky=p.y_w.shape[1],
                x_lo_n=tabs[3].data_ptr(), x_w=tabs[4].data_ptr(), Kx=p.x_w.shape[1])

    def call(**kw):
        a = dict(base, **kw)
        return lib.drn_fit_frames(a["src"], a["dst"], a["B"], a["Ts"], a["Hs"], a["Ws"], a["Td"], a["Hd"], a["Wd"], a["t_idx"],
                                  a["y_lo_n"], a["y_w"], a["Ky"], a["x_lo_n"], a["x_w"], a["Kx"], stream)
    bad = {f"null {k}": {k: None} for k in ("src", "dst", "t_idx", "y_lo_n", "y_w", "x_lo_n", "x_w")}
    bad.update({f"{k} = 0": {k: 0} for k in ("B", "Ts", "Hs", "Ws", "Td", "Hd", "Wd")})
    bad.update({"B < 0": dict(B=-1), "Ky = 0": dict(Ky=0), "Ky = 33": dict(Ky=33), "Kx = 0": dict(Kx=0), "Kx = 33": dict(Kx=33),
                "Hd = 24": dict(Hd=24), "Wd = 8": dict(Wd=8), "Hd = 17": dict(Hd=17),
                "output of 2^31 elements": dict(B=1 << 14, Td=1 << 8, Hd=16, Wd=16 * 11),            # 3 * 2^22 * 176 > 2^31
                "source of 2^31 elements": dict(B=1 << 12, Ts=1 << 8, Hs=1 << 8, Ws=1 << 4),          # 3 * 2^32
                "src 2 bytes off": dict(src=src.data_ptr() + 2), "y_w 1 byte off": dict(y_w=tabs[2].data_ptr() + 1),
                "x_w 2 bytes off": dict(x_w=tabs[4].data_ptr() + 2),
                "dst 8 bytes off": dict(dst=out + 8), "dst 2 bytes off": dict(dst=out + 2)})
    for name, kw in bad.items():
        assert call(**kw) == DRN_EINVAL, name
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all(), "a rejected call wrote"
    assert call() == 0
    torch.cuda.synchronize()
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all()
    # the wrapper reads the tables where their contents can be read
    for name, t in (("y_lo_n", p.y_lo_n.clone()), ("x_lo_n", p.x_lo_n.clone())):
        t[-1, 0] += 40
        kw = dict(t_idx=p.t_idx, y_lo_n=p.y_lo_n, y_w=p.y_w, x_lo_n=p.x_lo_n, x_w=p.x_w)
        kw[name] = t
        with pytest.raises(AssertionError, match="taps outside the source"):
            pkg.native.fit_frames(src, **kw)
    with pytest.raises(AssertionError, match="t_idx outside the clip"):
        pkg.native.fit_frames(src, p.t_idx + 1, p.y_lo_n, p.y_w, p.x_lo_n, p.x_w)


# ----------------------------------------------------------------------------------------------- nodes
def _inverse_pipeline(pkg, gpu, steps=2):
    sw = pkg.synthetic_weights
    net = tiny_net(pkg, 256, 1, 2)
    cfg = pkg.diffusion_renderer_config.get_inverse_renderer_config()
    cfg["net"] = dict(net)
    model = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=gpu)
    model.load_state_dict(sw.synth_state_dict(net, BF, device=gpu), strict=True)
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=gpu), device=gpu)
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=vae, model_instance=model, guidance=0.0, num_steps=steps)
    p.device = gpu
    p.set_model_type("inverse")
    return p


def test_inverse_node_with_fit(pkg, gpu):
    fit = R.fit_module(pkg)
    nodes = pkg.nodes
    p = _inverse_pipeline(pkg, gpu)
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    image = R.source(1, 11, 70, 75)
    outs = node.run_inverse_pass(p, image, guidance=0.0, seed=3, fit="crop")
    assert len(outs) == 5
    for o in outs:
        assert o.shape == (11, 64, 64, 3) and o.dtype == torch.float32 and 0.0 <= o.min() and o.max() <= 1.0
    # the composition by hand: the fitted tensor through the pipeline's own batched passes, cut to the clip's 11 frames
    plan = fit.plan_fit(11, 70, 75, "crop")
    assert (plan.T_out, plan.H_out, plan.W_out, plan.y0, plan.x0) == (17, 64, 64, 3, 5)
    clip = fit.fit_frames(image, plan, gpu)
    assert clip.is_cuda and clip.dtype == BF and clip.shape == (1, 3, 17, 64, 64)
    ci = torch.tensor([[nodes.GBUFFER_INDEX_MAPPING[k]] for k in nodes.INVERSE_PASSES], dtype=torch.long)
    p.window_frames = 0
    hand = p.generate_video_passes({"rgb": clip, "video": clip, "context_index": ci}, seed=3,
                                   normalize_normal=[k == "normal" for k in nodes.INVERSE_PASSES])
    for o, h in zip(outs, hand):
        assert h.shape == (1, 17, 64, 64, 3) and torch.equal(o, torch.from_numpy(h[0, :11]).float() / 255.0)
    again = node.run_inverse_pass(p, image, guidance=0.0, seed=3, fit="crop")          # reproducible from the seed
    assert all(torch.equal(a, b) for a, b in zip(outs, again))
    assert not torch.equal(outs[0], outs[3])
    for kw in (dict(fit="off"), {}):                                                  # fit off: refused as it is today
        with pytest.raises(ValueError, match="needs T = 8k\\+1 frames and H, W multiples of 8"):
            node.run_inverse_pass(p, image, guidance=0.0, seed=3, **kw)
    # windows take any T: three windows of 9 over 21 frames, nothing added in time
    long_clip = R.source(1, 21, 70, 75, seed=1)
    wins = node.run_inverse_pass(p, long_clip, guidance=0.0, seed=3, window_frames=9, window_overlap=2, fit="crop")
    assert len(pkg.windows.plan_windows(21, 9, 2)) == 3 and fit.plan_fit(21, 70, 75, "crop", windowed=True).T_out == 21
    for o in wins:
        assert o.shape == (21, 64, 64, 3)


def test_forward_node_with_fit(pkg, gpu):
    fit = R.fit_module(pkg)
    sw = pkg.synthetic_weights
    net = tiny_net(pkg, 256, 1, 2, forward=True)
    cfg = pkg.diffusion_renderer_config.get_forward_renderer_config()
    cfg["net"] = dict(net)
    cfg["model_type"] = "forward"
    model = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=gpu)
    model.load_state_dict(sw.synth_state_dict(net, BF, device=gpu), strict=True)
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=gpu), device=gpu)
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=vae, model_instance={"forward": model}, guidance=0.0, num_steps=2)
    p.device = gpu
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    names = ("depth", "normal", "roughness", "metallic", "base_color")
    g = {k: R.source(1, 10, 40, 36, seed=i) for i, k in enumerate(names)}
    env = sw.synth_tensor("fitfw.env", (1, 32, 64, 3), torch.float32).abs() * 4.0

    def run(maps, **kw):
        return node.run_forward_pass(p, *(maps[k] for k in names), env, guidance=0.0, seed=5, env_format="proj",
                                     env_rotation=180.0, **kw)[0]
    out = run(g, env_spin=90.0, fit="crop")
    assert out.shape == (1, 10, 32, 32, 3) and out.dtype == torch.float32 and 0.0 <= out.min() and out.max() <= 1.0
    # by hand: the fitted G-buffers (17 frames of 32 x 32) and the light turning 90 * 17 / 10 degrees over the 17 frames, cut to 10
    plan = fit.plan_fit(10, 40, 36, "crop")
    assert (plan.T_out, plan.H_out, plan.W_out) == (17, 32, 32)
    batch = {k.replace("base_color", "basecolor"): fit.fit_frames(v, plan, gpu) for k, v in g.items()}
    batch["video"] = batch["depth"]
    pe = importlib.import_module(pkg.__name__ + ".preprocess_envmap")
    cond = pe.envmap_conditions(env, (32, 32), 17, "proj", 1.0, False, 180.0, device=gpu, env_spin=90.0 * 17 / 10)
    batch.update(env_ldr=cond["env_ldr"], env_log=cond["env_log"], env_nrm=cond["env_nrm"].expand(1, -1, 17, -1, -1))
    p.window_frames = 0
    hand = torch.from_numpy(p.generate_video(data_batch=batch, seed=5)).float() / 255.0
    assert hand.shape == (1, 17, 32, 32, 3) and torch.equal(out, hand[:, :10])
    assert not torch.equal(out, run(g, env_spin=0.0, fit="crop"))
