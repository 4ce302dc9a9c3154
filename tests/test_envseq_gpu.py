"""drn_env_cubes and drn_env_project_seq (csrc/envmap.hip) on the GPU: the cube maps of a light sequence against the float64
evaluation of the torch specification, element by element; the projection with a cube map per frame against drn_env_project,
bit for bit; chunks; every refusal; envmap_conditions(env_sequence=True) and the forward node.  References, cases and bounds:
tests/envseq_refs.py (proved on the CPU in tests/test_envseq_cpu.py)."""
import pytest
import torch

import envmap_refs as ER
import envseq_refs as SR
from conftest import tiny_net

pytestmark = pytest.mark.gpu
PAD = 4096
EINVAL = -1


@pytest.fixture(scope="module")
def pe(pkg):
    return ER.pe_module(pkg)


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


# ------------------------------------------------------------------------------------------------ drn_env_cubes
def _cubes_guarded(pkg, c, gpu):
    buf, win = ER.guarded32(_numel(c["shape"]), PAD, gpu)
    out = win.view(c["shape"])
    pkg.native.env_cubes(c["latlong"].to(gpu), c["grid"].to(gpu), c["n0"], c["n"], c["brightness"], c["flip"], c["roll"], out=out)
    torch.cuda.synchronize()
    return buf, out


@pytest.mark.parametrize("i", range(len(SR.CUBE_CASES)), ids=SR.CUBE_CASE_IDS)
def test_cubes_match_float64_inside_guard_bands(pkg, gpu, i):
    """|hip - ref64| / s <= M_CUBES * E_ref at EVERY element (s = the largest of its four cleaned taps; exactly 0 where s = 0);
    nothing stored outside the output, every element of it stored, and a second launch gives the same bits."""
    c = SR.cube_case(pkg, i)
    buf, out = _cubes_guarded(pkg, c, gpu)
    ER.assert_guard32(buf, PAD, written=True)
    err = SR.cube_err(out, c)
    print(f"env-seq case {SR.CUBE_CASE_IDS[i]}: E_ref {c['e_ref']:.3e}  max|hip - ref64|/s {err:.3e}  ratio {err / c['e_ref']:.2f}  (bound {SR.M_CUBES})")
    assert err <= SR.M_CUBES * c["e_ref"]
    assert bool((out >= 0).all()) and bool((out <= 65504.0).all())
    _, again = _cubes_guarded(pkg, c, gpu)
    assert torch.equal(out, again)


def test_cubes_invalid_arguments_launch_nothing(pkg, gpu):
    lib = pkg.native.load_library()
    c = SR.cube_case(pkg, 0)
    latlong, grid = c["latlong"].to(gpu), c["grid"].to(gpu)
    N, He, We = latlong.shape[:3]
    R = c["R"]
    buf, out = ER.guarded32(N * 6 * R * R * 3, PAD, gpu)
    stream = torch.cuda.current_stream().cuda_stream
    good = [latlong.data_ptr(), grid.data_ptr(), out.data_ptr(), N, He, We, R, 0, N, 1.0, 0, 0, stream]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():          # "a6" = argument 6
            a[int(k[1:])] = v
        return lib.drn_env_cubes(*a)

    for pos in (0, 1, 2):
        assert call(**{f"a{pos}": None}) == EINVAL, pos                              # null pointers
        assert call(**{f"a{pos}": good[pos] + 2}) == EINVAL, pos                     # not 4-byte aligned
    for pos in (3, 4, 5, 6):
        assert call(**{f"a{pos}": 0}) == EINVAL and call(**{f"a{pos}": -3}) == EINVAL, pos
    assert call(a7=-1) == EINVAL and call(a8=0) == EINVAL and call(a8=-1) == EINVAL          # n0 < 0, n < 1
    assert call(a7=1, a8=N) == EINVAL and call(a7=N, a8=1) == EINVAL and call(a8=N + 1) == EINVAL    # n0 + n > N
    assert call(a11=-1) == EINVAL and call(a11=We) == EINVAL                              # roll outside [0, We)
    assert call(a3=1 << 20, a4=1 << 10, a5=1 << 10) == EINVAL                             # N*He*We*3 >= 2^31
    assert call(a6=1 << 14, a8=1) == EINVAL                                               # n*6*R*R*3 >= 2^31
    torch.cuda.synchronize()
    ER.assert_guard32(buf, PAD, written=False)
    assert call() == 0                                                                    # the same arguments, valid: runs
    torch.cuda.synchronize()
    ER.assert_guard32(buf, PAD, written=True)


# ------------------------------------------------------------------------------------------------ drn_env_project_seq
def _sentinel_pair(c, gpu):
    return tuple(torch.full((3, c["T_all"], c["H"], c["W"]), SR.SENTINEL, dtype=torch.float32, device=gpu) for _ in (0, 1))


@pytest.mark.parametrize("i", range(len(SR.PROJ_CASES)), ids=SR.PROJ_CASE_IDS)
def test_project_seq_is_env_project_frame_by_frame(pkg, gpu, i):
    """Frame t == drn_env_project(cubes[cube_of[t]], rot[t:t+1]), bit for bit, written at t0 + t of outputs that hold T_all frames
    whose other frames keep the sentinel; a second launch gives the same bits."""
    c = SR.proj_case(pkg, i)
    cubes, vec, rot = c["cubes"].to(gpu), c["vec"].to(gpu), c["rot"].to(gpu)
    table = torch.tensor(c["cube_of"], dtype=torch.int32)
    out = _sentinel_pair(c, gpu)
    pkg.native.env_project_seq(cubes, table, vec, rot, ER.LOG_SCALE, out=out, t0=c["t0"])
    for t, k in enumerate(c["cube_of"]):
        one = pkg.native.env_project(cubes[k], vec, rot[t:t + 1].contiguous(), ER.LOG_SCALE)
        for o, w in zip(out, one):
            assert torch.equal(o[:, c["t0"] + t], w[:, 0]), (t, k)
    err, rest = SR.proj_err(out, c)
    assert rest, "a frame outside the chunk was written"
    again = _sentinel_pair(c, gpu)
    pkg.native.env_project_seq(cubes, table, vec, rot, ER.LOG_SCALE, out=again, t0=c["t0"])
    assert torch.equal(out[0], again[0]) and torch.equal(out[1], again[1])
    if i == 0:           # the float64 bound of envmap_refs holds by what test_envmap_gpu.py shows; asserted on one case anyway
        print(f"env-seq case {SR.PROJ_CASE_IDS[i]}: E_ref {c['e_ref']:.3e}  max|hip - ref64| {err:.3e}  ratio {err / c['e_ref']:.2f}  (bound {ER.M_BOUND})")
        assert err <= ER.M_BOUND * c["e_ref"]
    # whole clip, no offset: the same frames in an output of its own
    ldr, log = pkg.native.env_project_seq(cubes, table, vec, rot, ER.LOG_SCALE)
    assert torch.equal(ldr, out[0][:, c["t0"]:c["t0"] + c["T"]]) and torch.equal(log, out[1][:, c["t0"]:c["t0"] + c["T"]])


def test_binding_refuses_a_table_outside_the_cubes(pkg, gpu):
    c = SR.proj_case(pkg, 0)
    cubes, vec, rot = c["cubes"].to(gpu), c["vec"].to(gpu), c["rot"].to(gpu)
    for bad in ([0, 1, 3], [-1, 0, 1]):
        with pytest.raises(AssertionError, match="cube_of"):
            pkg.native.env_project_seq(cubes, torch.tensor(bad, dtype=torch.int32), vec, rot)
    with pytest.raises(AssertionError, match="cube_of"):
        pkg.native.env_project_seq(cubes, torch.tensor([0, 1, 2], dtype=torch.int32, device=gpu), vec, rot)


@pytest.mark.parametrize("T,n_lights", [(5, 5), (7, 5)], ids=["T5_N5", "T7_N5_padded"])
def test_chunked_build_equals_the_unchunked(pe, gpu, T, n_lights):
    """A clip built in chunks of 1, 2 and 16 frames == the build in one chunk, bit for bit (T = 7 over 5 lights: the last light
    repeats over the padded frames, inside a chunk and across chunks)."""
    frames = torch.cat([SR.panoramas(24, 48), SR.panoramas(24, 48).flip(2)[:2]]).to(gpu).contiguous()
    vec = pe.latlong_vec((16, 24), device=gpu).contiguous()
    rot = pe.spin_table(111.0, T).to(gpu)
    cube_of = pe.sequence_cube_of(n_lights, T)
    whole = pe.project_sequence_hip(frames, cube_of, vec, rot, 0.5, True, 4, res=32, chunk=T)
    for chunk in (1, 2, 16):
        got = pe.project_sequence_hip(frames, cube_of, vec, rot, 0.5, True, 4, res=32, chunk=chunk)
        assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1]), chunk
    assert bool(torch.isfinite(whole[0]).all()) and not torch.equal(whole[1][:, 0], whole[1][:, 1])


def test_project_seq_invalid_arguments_launch_nothing(pkg, gpu):
    lib = pkg.native.load_library()
    c = SR.proj_case(pkg, 0)
    T, H, W, R, T_all, t0 = c["T"], c["H"], c["W"], c["R"], c["T_all"], c["t0"]
    cubes, vec, rot = c["cubes"].to(gpu), c["vec"].to(gpu), c["rot"].to(gpu)
    table = torch.tensor(c["cube_of"], dtype=torch.int32, device=gpu)
    n = 3 * T_all * H * W
    (b0, o0), (b1, o1) = ER.guarded32(n, PAD, gpu), ER.guarded32(n, PAD, gpu)
    stream = torch.cuda.current_stream().cuda_stream
    good = [cubes.data_ptr(), 3, table.data_ptr(), R, vec.data_ptr(), rot.data_ptr(), o0.data_ptr(), o1.data_ptr(), T, t0, T_all, H, W,
            ER.LOG_SCALE, stream]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.drn_env_project_seq(*a)

    for pos in (0, 2, 4, 5, 6, 7):
        assert call(**{f"a{pos}": None}) == EINVAL, pos                              # null pointers, the table among them
        assert call(**{f"a{pos}": good[pos] + 2}) == EINVAL, pos                     # not 4-byte aligned, the table among them
    for pos in (1, 3, 8, 11, 12):
        assert call(**{f"a{pos}": 0}) == EINVAL and call(**{f"a{pos}": -3}) == EINVAL, pos     # n_cubes, R, T, H, W < 1
    assert call(a9=-1) == EINVAL and call(a9=T_all - T + 1) == EINVAL and call(a10=T - 1, a9=0) == EINVAL    # t0 < 0, t0 + T > T_all
    assert call(a8=2048, a9=0, a10=2048, a11=1024, a12=1024) == EINVAL               # T_all*H*W = 2^31
    assert call(a8=1, a9=0, a10=1 << 30, a11=2, a12=1) == EINVAL
    torch.cuda.synchronize()
    ER.assert_guard32(b0, PAD, written=False)
    ER.assert_guard32(b1, PAD, written=False)
    assert call(a9=0) == 0 and call(a9=T_all - T) == 0                               # valid: runs; the two chunks cover T_all
    torch.cuda.synchronize()
    ER.assert_guard32(b0, PAD, written=True)
    ER.assert_guard32(b1, PAD, written=True)


# ------------------------------------------------------------------------------------------------ end to end
def test_envmap_conditions_sequence_hip_against_torch_on_the_device(pkg, pe, gpu):
    """envmap_conditions(env_sequence=True) through the kernels and through the torch loop, both on the device, at 18 x 32, T = 3,
    the 512^2 cube maps the node uses and NODE_CASE's spin, with the bound of the existing NODE_CASE test: M_BOUND * E_ref for the
    difference of the two and for each against float64, same tie mask.  As there, E_ref is the fp32 torch path's own error on the
    inputs at hand and the float64 reference starts from the cube map and directions built on the device - here per frame, from
    frame t's own cube map (SR.sequence_references): E_ref depends on the light (1.7e-6, 1.1e-3 and 7.6e-6 for these three on the
    CPU: the second has a dark texel beside a bright one under a pixel, where env_ldr = sRGB(16 x / (1 + x)) has a slope of ~400),
    so every frame is held to its own."""
    pe.clear_environment_cache()
    H, W, T, spin, R = ER.NODE_CASE
    env = torch.stack([torch.rand(24, 48, 3, generator=torch.Generator().manual_seed(20250311 + k)).pow(4) * 50.0 for k in range(T)])
    cubes = [pe.latlong_to_cubemap_official(pe.apply_hdr_preprocessing(env[k], 1.0, False, 0.0, gpu), [R, R]).cpu() for k in range(T)]
    frames = SR.sequence_references(pe, cubes, pe.latlong_vec((H, W), device=gpu).cpu(), pe.spin_table(spin, T))
    kw = dict(device=gpu, env_spin=spin, env_sequence=True)
    a = pe.envmap_conditions(env, (H, W), T, "proj", 1.0, False, 0.0, backend="hip", **kw)
    b = pe.envmap_conditions(env, (H, W), T, "proj", 1.0, False, 0.0, backend="torch", **kw)
    pe.clear_environment_cache()                                                       # so that 'auto' computes, not hits
    auto = pe.envmap_conditions(env, (H, W), T, "proj", 1.0, False, 0.0, **kw)
    for d in (a, b, auto):
        assert d["env_ldr"].shape == d["env_log"].shape == (1, 3, T, H, W) and d["env_nrm"].shape == (1, 3, 1, H, W)
        assert d["env_ldr"].is_cuda and d["env_ldr"].dtype == torch.float32
    assert torch.equal(auto["env_ldr"], a["env_ldr"]) and torch.equal(auto["env_log"], a["env_log"])      # auto + sequence = the kernels
    assert torch.equal(a["env_nrm"], b["env_nrm"])
    assert not torch.equal(a["env_log"][:, :, 0], a["env_log"][:, :, 1])
    worst = []
    for t, f in enumerate(frames):
        hip = (a["env_ldr"][0, :, t:t + 1], a["env_log"][0, :, t:t + 1])
        tch = (b["env_ldr"][0, :, t:t + 1], b["env_log"][0, :, t:t + 1])
        e = f["e_ref"]
        e_hip, e_tch = ER.max_err(hip, f["ref"], f["mask"]), ER.max_err(tch, f["ref"], f["mask"])
        diff = ER.max_err(hip, tuple(x.double().cpu() for x in tch), f["mask"])
        print(f"env-seq case {ER.NODE_CASE_ID} through envmap_conditions, frame {t}: E_ref {e:.3e}  max|hip - ref64| {e_hip:.3e} ratio "
              f"{e_hip / e:.3f}  max|torch(device) - ref64| {e_tch:.3e} ratio {e_tch / e:.3f}  max|hip - torch(device)| {diff:.3e} "
              f"ratio {diff / e:.3f}  (bound {ER.M_BOUND})")
        worst.append(max(diff, e_hip, e_tch) / e)
    assert max(worst) <= ER.M_BOUND, worst
    pe.clear_environment_cache()


def test_envmap_conditions_sequence_passes_flip_rotation_and_brightness_on(pkg, pe, gpu):
    """The host path's own arguments (env_flip, env_rot -> roll, env_brightness, the spin table, cube_of under time padding) reach
    the kernels: kernels against the torch loop on the device with all of them set, on SMOOTH lights without symmetry in the
    azimuth (envmap_refs.smooth_panorama, rolled and scaled per frame), outside the tie mask.
    Bound 1e-5, by the reasoning of test_envmap_spin_cpu.py::test_quarter_turn_rolls_the_image: the two cube builds differ by an
    ulp or two of a texel coordinate (<= 8e-6 texel) of a panorama that changes by < 0.05 per texel, ~4e-7, times a tone-map slope
    of < 20 at these values (channel 0 is ~0.02 .. 0.04, the others ~0.4 .. 1), plus a few ulp of tone maps in [-1, 1] (~5e-7);
    a lost flip, a roll the wrong way or a lost brightness move the image by 0.01 and more."""
    pe.clear_environment_cache()
    H, W, T, spin, _ = ER.NODE_CASE
    base = ER.smooth_panorama()
    env = torch.stack([torch.roll(base, 5 * k, dims=1) * s for k, s in enumerate((1.0, 1.5, 0.6))])
    args = (env, (H, W), T + 2, "proj", 0.5, True, 37.0)
    kw = dict(device=gpu, env_spin=spin, env_sequence=True, clip_frames=T)
    a = pe.envmap_conditions(*args, backend="hip", **kw)
    b = pe.envmap_conditions(*args, backend="torch", **kw)
    mask = ER.tie_mask(pe.latlong_vec((H, W), device="cpu"), pe.spin_table(spin, T + 2))
    diff = ER.max_err((a["env_ldr"][0], a["env_log"][0]), (b["env_ldr"][0].double().cpu(), b["env_log"][0].double().cpu()), mask)
    print(f"env-seq smooth lights, flip / rot 37 / brightness 0.5 / spin {spin} / T {T} padded to {T + 2}: max|hip - torch(device)| {diff:.3e}")
    assert a["env_ldr"].shape == (1, 3, T + 2, H, W) and diff <= 1e-5
    for wrong in (dict(env_flip=False), dict(env_rot=360.0 - 37.0), dict(env_brightness=1.0)):
        pe.clear_environment_cache()
        w = dict(env_brightness=0.5, env_flip=True, env_rot=37.0)
        w.update(wrong)
        c = pe.envmap_conditions(env, (H, W), T + 2, "proj", backend="torch", **w, **kw)
        far = ER.max_err((a["env_ldr"][0], a["env_log"][0]), (c["env_ldr"][0].double().cpu(), c["env_log"][0].double().cpu()), mask)
        assert far > 0.01, (wrong, far)
    pe.clear_environment_cache()


@pytest.fixture(scope="module")
def forward_pipe(pkg, gpu):
    sw, cfgm = pkg.synthetic_weights, pkg.diffusion_renderer_config
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
    return p


def _node_inputs(pkg, T, H=32, W=32):
    sw = pkg.synthetic_weights
    g = [sw.synth_tensor("seq." + k, (1, T, H, W, 3), torch.float32).abs() for k in ("depth", "normal", "roughness", "metallic", "base_color")]
    env = sw.synth_tensor("seq.env", (T, 32, 64, 3), torch.float32).abs() * 4.0
    return g, env


def test_forward_node_with_a_light_sequence(pkg, pe, gpu, forward_pipe, monkeypatch):
    """The forward node on the tiny forward net, 9 frames, 2 steps, a 9-frame env_map: a finite picture that differs from the static
    one, goes through one drn_env_cubes / drn_env_project_seq pair (9 <= 16 frames) and equals the composition by hand (the
    conditions of envmap_conditions handed to the pipeline as the node hands them); a 1-frame env_map equals env_sequence off."""
    launches = []
    real = pkg.native.env_project_seq
    monkeypatch.setattr(pkg.native, "env_project_seq",
                        lambda cubes, cube_of, *a, **kw: (launches.append((cubes.shape[0], cube_of.tolist(), kw.get("t0"))), real(cubes, cube_of, *a, **kw))[1])
    pe.clear_environment_cache()
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    g, env = _node_inputs(pkg, 9)

    def run(e, **kw):
        (out,) = node.run_forward_pass(forward_pipe, *g, e, guidance=0.0, seed=5, env_format="proj", env_brightness=1.0,
                                       env_flip_horizontal=False, env_rotation=180.0, **kw)
        return out

    plain = run(env)
    assert launches == []
    seq = run(env, env_sequence=True)
    assert launches == [(9, list(range(9)), 0)]
    assert seq.shape == (1, 9, 32, 32, 3) and bool(torch.isfinite(seq).all()) and 0.0 <= seq.min() and seq.max() <= 1.0
    assert not torch.equal(seq, plain)
    # by hand: the sequence's conditions, then the pipeline as the node calls it
    cond = pe.envmap_conditions(env, (32, 32), 9, "proj", 1.0, False, 180.0, device=gpu, env_sequence=True)
    batch = {k: v.permute(0, 4, 1, 2, 3) * 2.0 - 1.0 for k, v in zip(("depth", "normal", "roughness", "metallic", "basecolor"), g)}
    batch["video"] = batch["depth"]
    batch.update(env_ldr=cond["env_ldr"], env_log=cond["env_log"], env_nrm=cond["env_nrm"].expand(1, -1, 9, -1, -1))
    hand = torch.from_numpy(forward_pipe.generate_video(data_batch=batch, seed=5)).float() / 255.0
    assert torch.equal(seq, hand)
    pe.clear_environment_cache()
    assert torch.equal(run(env[:1], env_sequence=True), plain)                           # N = 1: today's path, bit for bit
    assert len(launches) == 1
    pe.clear_environment_cache()


def test_forward_node_sequence_with_time_padding_and_windows(pkg, pe, gpu, forward_pipe):
    """fit='crop' pads 10 frames to 17: the last light repeats over the padded frames, which are cut away - the first 10 frames
    equal the run whose env_map was padded by hand to 17 frames on a 17-frame clip's conditions.  Windows: the conditions are
    built for the whole clip, so a windowed run takes the sequence as it takes a spinning light."""
    pe.clear_environment_cache()
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    g, env = _node_inputs(pkg, 10)
    kw = dict(guidance=0.0, seed=5, env_format="proj", env_rotation=180.0)
    (fit,) = node.run_forward_pass(forward_pipe, *g, env, env_sequence=True, fit="crop", **kw)
    (static,) = node.run_forward_pass(forward_pipe, *g, env, fit="crop", **kw)
    assert fit.shape == (1, 10, 32, 32, 3) and bool(torch.isfinite(fit).all()) and not torch.equal(fit, static)
    cond = pe.envmap_conditions(env, (32, 32), 17, "proj", 1.0, False, 180.0, device=gpu, env_sequence=True, clip_frames=10)
    by_hand = pe.envmap_conditions(torch.cat([env, env[9:].expand(7, -1, -1, -1)]), (32, 32), 17, "proj", 1.0, False, 180.0,
                                   device=gpu, env_sequence=True)
    assert torch.equal(cond["env_ldr"], by_hand["env_ldr"]) and torch.equal(cond["env_log"], by_hand["env_log"])
    with pytest.raises(ValueError, match=r"N = 10 .* T = 9"):
        node.run_forward_pass(forward_pipe, *(x[:, :9] for x in g), env, env_sequence=True, **kw)
    pe.clear_environment_cache()
    g17, env17 = _node_inputs(pkg, 17)
    (win,) = node.run_forward_pass(forward_pipe, *g17, env17, env_sequence=True, window_frames=9, window_overlap=1, **kw)
    (win_static,) = node.run_forward_pass(forward_pipe, *g17, env17, window_frames=9, window_overlap=1, **kw)
    assert win.shape == (1, 17, 32, 32, 3) and bool(torch.isfinite(win).all()) and not torch.equal(win, win_static)
    (head,) = node.run_forward_pass(forward_pipe, *(x[:, :9].contiguous() for x in g17), env17[:9], env_sequence=True, window_frames=9,
                                    window_overlap=1, **kw)
    assert torch.equal(win[:, :8], head[:, :8])                                          # the first window sees lights 0 .. 8
    pe.clear_environment_cache()
