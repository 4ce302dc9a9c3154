"""The relight path on the GPU with tiny nets: the pipeline's `to_host=False` outputs against the default arrays, Cosmos1Relight
against the two nodes chained through the host (or the composition by hand where fit_restore is on), and a uint8 image through
the inverse node against the fp32 image u8 / 255."""
import pytest
import torch

import fit_refs as R
import fit_u8_refs as U
from conftest import tiny_net

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAMES = ("base_color", "metallic", "roughness", "normal", "depth")          # the inverse node's order


@pytest.fixture(scope="module")
def pipe(pkg, gpu):
    """One pipeline that holds both renderers: tiny nets, the synthetic tokenizer, 2 steps."""
    sw = pkg.synthetic_weights
    models = {}
    for kind, forward in (("inverse", False), ("forward", True)):
        net = tiny_net(pkg, 256, 1, 2, forward=forward)
        cfgm = pkg.diffusion_renderer_config
        cfg = cfgm.get_forward_renderer_config() if forward else cfgm.get_inverse_renderer_config()
        cfg["net"] = dict(net)
        cfg["model_type"] = kind
        m = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=gpu)
        m.load_state_dict(sw.synth_state_dict(net, BF, device=gpu), strict=True)
        models[kind] = m
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=gpu), device=gpu)
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=vae, model_instance=models, guidance=0.0, num_steps=2)
    p.device = gpu
    return p


@pytest.fixture(scope="module")
def env(pkg):
    return pkg.synthetic_weights.synth_tensor("relight.env", (1, 32, 64, 3), torch.float32).abs() * 4.0


def _inverse_batches(pkg, clip):
    nodes = pkg.nodes
    ci = torch.tensor([[nodes.GBUFFER_INDEX_MAPPING[k]] for k in nodes.INVERSE_PASSES], dtype=torch.long)
    flags = [k == "normal" for k in nodes.INVERSE_PASSES]
    return ci, flags


@pytest.mark.parametrize("windows", (False, True), ids=("whole_clip", "windowed"))
def test_to_host_false_keeps_the_bytes_on_the_device(pkg, gpu, pipe, windows):
    fit = R.fit_module(pkg)
    T = 21 if windows else 9
    clip = fit.fit_frames(R.source(1, T, 32, 32, seed=2), fit.plan_fit(T, 32, 32, "crop", windowed=True), gpu)
    ci, flags = _inverse_batches(pkg, clip)
    pipe.set_model_type("inverse")
    pipe.guidance, pipe.restore_plan = 0.0, None
    pipe.window_frames, pipe.window_overlap = (9, 2) if windows else (0, 8)
    batch = {"rgb": clip, "video": clip, "context_index": ci}
    want = pipe.generate_video_passes(batch, seed=3, normalize_normal=flags)
    got = pipe.generate_video_passes(batch, seed=3, normalize_normal=flags, to_host=False)
    assert len(got) == len(want) == 5
    for g, w in zip(got, want):
        assert isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.uint8 and g.shape == (1, T, 32, 32, 3)
        assert torch.equal(g.cpu(), torch.from_numpy(w))
    one = {"rgb": clip, "video": clip, "context_index": ci[3:4]}
    w = pipe.generate_video(one, normalize_normal=True, seed=3)
    g = pipe.generate_video(one, normalize_normal=True, seed=3, to_host=False)
    assert g.is_cuda and torch.equal(g.cpu(), torch.from_numpy(w)) and torch.equal(g.cpu(), torch.from_numpy(want[3]))
    each = pipe.generate_video_each([one, dict(one, context_index=ci[0:1])], [True, False], seed=3, to_host=False)
    assert all(e.is_cuda for e in each) and torch.equal(each[0], g) and torch.equal(each[1].cpu(), torch.from_numpy(want[0]))
    # with a restore plan the device tensors are the restored ones
    pipe.restore_plan = fit.plan_restore(fit.plan_fit(T, 40, 36, "stretch", windowed=True))
    w = pipe.generate_video(one, normalize_normal=True, seed=3)
    g = pipe.generate_video(one, normalize_normal=True, seed=3, to_host=False)
    pipe.restore_plan = None
    assert g.is_cuda and g.shape == (1, T, 40, 36, 3) and torch.equal(g.cpu(), torch.from_numpy(w))


def _chain(pkg, pipe, image, env, inv_kw, fwd_kw):
    g = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]().run_inverse_pass(pipe, image, seed=3, **inv_kw)
    g5 = dict(zip(NAMES, (o.reshape(1, -1, *o.shape[1:]) for o in g)))
    (relit,) = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]().run_forward_pass(
        pipe, g5["depth"], g5["normal"], g5["roughness"], g5["metallic"], g5["base_color"], env, seed=3, **fwd_kw)
    return (relit, *g)


CASES = {
    "9x64x64_fit_off": ((9, 64, 64), dict()),
    "11x70x75_crop": ((11, 70, 75), dict(fit="crop")),
    "21x70x75_crop_windows_9_2": ((21, 70, 75), dict(fit="crop", window_frames=9, window_overlap=2)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_relight_equals_the_two_node_chain(pkg, gpu, pipe, env, name):
    (T, H, W), kw = CASES[name]
    image = R.source(1, T, H, W, seed=4)
    win = {k: v for k, v in kw.items() if k.startswith("window")}
    light = dict(env_spin=90.0, env_rotation=180.0)
    node = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    got = node.run_relight(pipe, pipe, image, env, seed=3, **light, **kw)
    want = _chain(pkg, pipe, image, env, kw, dict(light, fit="crop", **win))
    assert len(got) == 6 and got[0].shape == (1, T, 64, 64, 3) and all(o.shape == (T, 64, 64, 3) for o in got[1:])
    for n, a, b in zip(("image",) + NAMES, got, want):
        assert a.dtype == torch.float32 and not a.is_cuda and torch.equal(a, b), n
    assert float(got[0].std()) > 0 and not torch.equal(got[1], got[4])


def test_relight_with_stretch_and_restore_is_the_composition_by_hand(pkg, gpu, pipe, env):
    fit = R.fit_module(pkg)
    T, H, W = 10, 40, 36
    image = R.source(1, T, H, W, seed=5)
    node = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    got = node.run_relight(pipe, pipe, image, env, seed=3, env_spin=45.0, fit="stretch", fit_restore=True)
    assert got[0].shape == (1, T, H, W, 3) and all(o.shape == (T, H, W, 3) for o in got[1:]) and pipe.restore_plan is not None
    rplan = fit.plan_restore(fit.plan_fit(T, H, W, "stretch"))
    small = _chain(pkg, pipe, image, env, dict(fit="stretch"), dict(env_spin=45.0, fit="crop"))   # everything at the model's size
    assert small[0].shape == (1, T, 32, 32, 3) and pipe.restore_plan is None
    for n, a, s in zip(("image",) + NAMES, got, small):
        u8 = (s * 255.0).round().to(torch.uint8).reshape(1, T, 32, 32, 3)
        assert torch.equal(u8.float() / 255.0, s.reshape(1, T, 32, 32, 3))
        assert torch.equal(a.reshape(1, T, H, W, 3), fit.restore_frames(u8.to(gpu), rplan).cpu().float() / 255.0), n
    with pytest.raises(ValueError, match="crop cannot be undone"):
        node.run_relight(pipe, pipe, image, env, seed=3, fit="crop", fit_restore=True)


def test_inverse_node_takes_a_uint8_image(pkg, gpu, pipe):
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    for (T, H, W), kw in (((9, 32, 32), dict()), ((11, 70, 75), dict(fit="crop"))):
        u8 = U.source_u8(1, T, H, W, seed=6)
        got = node.run_inverse_pass(pipe, u8, seed=3, **kw)
        want = node.run_inverse_pass(pipe, u8.float() / 255.0, seed=3, **kw)
        assert len(got) == 5 and all(torch.equal(a, b) for a, b in zip(got, want)), (T, H, W)
