"""drn_env_project (csrc/envmap.hip) on the GPU: the rotating environment light against the float64 evaluation of the torch path,
its store geometry inside guard bands, the argument checks, the dispatch of preprocess_envmap and the forward node with env_spin.
References, cases and the bound: tests/envmap_refs.py (proved on the CPU in tests/test_envmap_spin_cpu.py)."""
import pytest
import torch

import envmap_refs as ER
from conftest import tiny_net

pytestmark = pytest.mark.gpu
PAD = 4096
EINVAL = -1


@pytest.fixture(scope="module")
def pe(pkg):
    return ER.pe_module(pkg)


def _run_guarded(pkg, c, gpu):
    n = 1
    for d in c["shape"]:
        n *= d
    bufs = [ER.guarded32(n, PAD, gpu) for _ in (0, 1)]
    out = tuple(w.view(c["shape"]) for _, w in bufs)
    pkg.native.env_project(c["cube"].to(gpu), c["vec"].to(gpu), c["rot"].to(gpu), ER.LOG_SCALE, out=out)
    torch.cuda.synchronize()
    return bufs, out


@pytest.mark.parametrize("i", range(len(ER.CASES)), ids=ER.CASE_IDS)
def test_kernel_matches_float64_inside_guard_bands(pkg, gpu, i):
    """max|hip - ref64| <= M_BOUND * E_ref outside the tie mask; nothing stored outside the two outputs, every element of them
    stored, and a second launch gives the same bits."""
    c = ER.case(pkg, i)
    bufs, out = _run_guarded(pkg, c, gpu)
    for buf, _ in bufs:
        ER.assert_guard32(buf, PAD, written=True)
    err = ER.max_err(out, c["ref"], c["mask"])
    print(f"case {ER.CASE_IDS[i]}: E_ref {c['e_ref']:.3e}  max|hip - ref64| {err:.3e}  ratio {err / c['e_ref']:.2f}  (bound {ER.M_BOUND})")
    assert err <= ER.M_BOUND * c["e_ref"]
    assert all(bool(o.abs().max() <= 1.0) for o in out)
    _, again = _run_guarded(pkg, c, gpu)
    assert torch.equal(out[0], again[0]) and torch.equal(out[1], again[1])


def test_static_light_repeats_frame_zero(pkg, gpu):
    c = ER.case(pkg, 0)
    rot = torch.tensor([[1.0, 0.0]] * 3)
    ldr, log = pkg.native.env_project(c["cube"].to(gpu), c["vec"].to(gpu), rot.to(gpu))
    one = pkg.native.env_project(c["cube"].to(gpu), c["vec"].to(gpu), rot[:1].to(gpu))
    for full, single in ((ldr, one[0]), (log, one[1])):
        assert full.shape == (3, 3, 16, 24) and single.shape == (3, 1, 16, 24)
        for t in range(3):
            assert torch.equal(full[:, t], single[:, 0])


def test_quarter_turn_rolls_the_image_on_the_device(pe, gpu):
    """The property and the bound of tests/test_envmap_spin_cpu.py::test_quarter_turn_rolls_the_image, through backend='hip'."""
    env = ER.smooth_panorama()
    kw = dict(env_brightness=1.0, env_flip=False, env_rot=0.0, device=gpu, num_frames=4, use_cache=False, backend="hip")
    s = pe.render_projection_from_panorama(env, (16, 32), env_spin=360.0, **kw)
    st = pe.render_projection_from_panorama(env, (16, 32), **kw)
    for k in ("env_ldr", "env_log"):
        assert s[k].shape == st[k].shape == (4, 16, 32, 3)
        assert torch.equal(st[k][3], st[k][0])                                        # spin 0: T = 1 launch, expanded
        right = (s[k][1] - torch.roll(st[k][0], -8, dims=1)).abs().max().item()
        wrong = (s[k][1] - torch.roll(st[k][0], 8, dims=1)).abs().max().item()
        print(f"{k}: quarter turn {right:.2e} (wrong way {wrong:.2e})")
        assert right <= 1e-5 and wrong > 0.1


def test_forced_kernel_static_cache_serves_any_frame_count(pe, gpu):
    """backend='hip' with a static light caches its ONE frame (the static key carries no T): a later call with another T gets
    its own frame count, the same frame, from the cache."""
    pe.clear_environment_cache()
    env = ER.panorama()
    a = pe.envmap_conditions(env, (8, 12), 3, "proj", 1.0, False, 0.0, device=gpu, backend="hip")
    b = pe.envmap_conditions(env, (8, 12), 5, "proj", 1.0, False, 0.0, device=gpu, backend="hip")
    assert pe.get_cache_stats()["cache_size"] == 1
    assert a["env_ldr"].shape == (1, 3, 3, 8, 12) and b["env_ldr"].shape == b["env_log"].shape == (1, 3, 5, 8, 12)
    assert b["env_ldr"].data_ptr() == a["env_ldr"].data_ptr() and torch.equal(b["env_log"][:, :, 4], a["env_log"][:, :, 0])
    pe.clear_environment_cache()


def test_invalid_arguments_launch_nothing(pkg, gpu):
    lib = pkg.native.load_library()
    c = ER.case(pkg, 0)
    _, T, H, W = c["shape"]
    R = c["cube"].shape[1]
    cube, vec, rot = c["cube"].to(gpu), c["vec"].to(gpu), c["rot"].to(gpu)
    n = 3 * T * H * W
    (b0, o0), (b1, o1) = ER.guarded32(n, PAD, gpu), ER.guarded32(n, PAD, gpu)
    stream = torch.cuda.current_stream().cuda_stream
    good = [cube.data_ptr(), R, vec.data_ptr(), rot.data_ptr(), o0.data_ptr(), o1.data_ptr(), T, H, W, ER.LOG_SCALE, stream]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():          # "a6" = argument 6
            a[int(k[1:])] = v
        return lib.drn_env_project(*a)

    for pos in (0, 2, 3, 4, 5):
        assert call(**{f"a{pos}": None}) == EINVAL, pos                              # null pointers
        assert call(**{f"a{pos}": good[pos] + 2}) == EINVAL, pos                     # not 4-byte aligned
    for pos in (1, 6, 7, 8):
        assert call(**{f"a{pos}": 0}) == EINVAL and call(**{f"a{pos}": -3}) == EINVAL, pos
    assert call(a6=2048, a7=1024, a8=1024) == EINVAL                                 # T*H*W = 2^31
    assert call(a6=1 << 30, a7=2, a8=1) == EINVAL
    torch.cuda.synchronize()
    ER.assert_guard32(b0, PAD, written=False)
    ER.assert_guard32(b1, PAD, written=False)
    assert call() == 0                                                               # the same arguments, valid: runs
    torch.cuda.synchronize()
    ER.assert_guard32(b0, PAD, written=True)
    ER.assert_guard32(b1, PAD, written=True)


def test_envmap_conditions_hip_against_torch_on_the_device(pkg, pe, gpu):
    """envmap_conditions(env_spin=120) through the kernel and through the torch path, both on the device, at the 512^2 cube map
    the node uses (ER.NODE_CASE).  Same bound as the kernel test, M_BOUND * E_ref of this case, for the difference of the two and
    for each against float64; same tie mask.  The float64 reference starts from the cube map and directions built on the device,
    the tensors both paths start from."""
    pe.clear_environment_cache()
    c = ER.node_case_on(pe, gpu)
    env, (H, W, T, spin, _) = ER.panorama(), ER.NODE_CASE
    a = pe.envmap_conditions(env, (H, W), T, "proj", 1.0, False, 0.0, device=gpu, env_spin=spin, backend="hip")
    b = pe.envmap_conditions(env, (H, W), T, "proj", 1.0, False, 0.0, device=gpu, env_spin=spin, backend="torch")
    pe.clear_environment_cache()                                                       # so that 'auto' computes, not hits
    auto = pe.envmap_conditions(env, (H, W), T, "proj", 1.0, False, 0.0, device=gpu, env_spin=spin)
    for d in (a, b, auto):
        assert d["env_ldr"].shape == d["env_log"].shape == (1, 3, T, H, W) and d["env_nrm"].shape == (1, 3, 1, H, W)
        assert d["env_ldr"].is_cuda and d["env_ldr"].dtype == torch.float32
    assert torch.equal(auto["env_ldr"], a["env_ldr"]) and torch.equal(auto["env_log"], a["env_log"])      # auto + spin = the kernel
    assert torch.equal(a["env_nrm"], b["env_nrm"])
    hip, tch = (a["env_ldr"][0], a["env_log"][0]), (b["env_ldr"][0], b["env_log"][0])
    e, bound = c["e_ref"], ER.M_BOUND * c["e_ref"]
    e_hip, e_tch = ER.max_err(hip, c["ref"], c["mask"]), ER.max_err(tch, c["ref"], c["mask"])
    diff = ER.max_err(hip, tuple(x.double().cpu() for x in tch), c["mask"])
    print(f"case {ER.NODE_CASE_ID}: E_ref {e:.3e}  max|hip - ref64| {e_hip:.3e} ratio {e_hip / e:.3f}  max|torch(device) - ref64| {e_tch:.3e} "
          f"ratio {e_tch / e:.3f}  max|hip - torch(device)| {diff:.3e} ratio {diff / e:.3f}  (bound {ER.M_BOUND})")
    assert diff <= bound and e_hip <= bound and e_tch <= bound
    # static lighting under 'auto' stays on the torch path, bit for bit what the call without the keyword gives
    s0 = pe.envmap_conditions(env, (H, W), T, "proj", 1.0, False, 0.0, device=gpu)
    pe.clear_environment_cache()
    s1 = pe.envmap_conditions(env, (H, W), T, "proj", 1.0, False, 0.0, device=gpu, env_spin=0.0, backend="torch")
    assert torch.equal(s0["env_ldr"], s1["env_ldr"]) and torch.equal(s0["env_log"], s1["env_log"])
    pe.clear_environment_cache()


def test_forward_node_with_env_spin(pkg, pe, gpu, monkeypatch):
    """The forward node on the tiny forward net of test_forward_node_end_to_end, 9 frames, 2 steps: env_spin=120 gives a finite
    picture of the right shape that differs from the static one and goes through drn_env_project (one launch of 9 frames);
    env_spin=0 launches nothing there and is the call without the argument, bit for bit."""
    launches = []
    real = pkg.native.env_project
    monkeypatch.setattr(pkg.native, "env_project", lambda cube, vec, rot, *a, **kw: (launches.append(tuple(rot.shape)), real(cube, vec, rot, *a, **kw))[1])
    pe.clear_environment_cache()
    sw = pkg.synthetic_weights
    cfgm = pkg.diffusion_renderer_config
    net = tiny_net(pkg, 256, 1, 2, forward=True)
    cfg = cfgm.get_forward_renderer_config()
    cfg["net"] = dict(net)
    cfg["model_type"] = "forward"
    model = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=gpu)
    model.load_state_dict(sw.synth_state_dict(net, torch.bfloat16, device=gpu), strict=True)
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=gpu), device=gpu)
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=vae, model_instance={"forward": model}, guidance=0.0, num_steps=2)
    p.device = gpu
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    g = {k: sw.synth_tensor("fw." + k, (1, 9, 32, 32, 3), torch.float32).abs() for k in ("depth", "normal", "roughness", "metallic", "base_color")}
    env = sw.synth_tensor("fw.env", (1, 32, 64, 3), torch.float32).abs() * 4.0

    def run(**kw):
        (out,) = node.run_forward_pass(p, g["depth"], g["normal"], g["roughness"], g["metallic"], g["base_color"], env, guidance=0.0,
                                       seed=5, env_format="proj", env_brightness=1.0, env_flip_horizontal=False, env_rotation=180.0, **kw)
        return out

    plain = run()
    pe.clear_environment_cache()
    zero = run(env_spin=0.0)
    assert launches == []
    spun = run(env_spin=120.0)
    assert launches == [(9, 2)]
    pe.clear_environment_cache()
    assert spun.shape == (1, 9, 32, 32, 3) and spun.dtype == torch.float32 and bool(torch.isfinite(spun).all())
    assert 0.0 <= spun.min() and spun.max() <= 1.0
    assert torch.equal(zero, plain)
    assert not torch.equal(spun, plain)
    with pytest.raises(ValueError, match="ball"):
        node.run_forward_pass(p, g["depth"], g["normal"], g["roughness"], g["metallic"], g["base_color"], env, env_format="ball",
                              env_spin=30.0)
