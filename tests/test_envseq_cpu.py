"""A light per frame (env_sequence) on the CPU: the torch path that specifies it, the sampling grid the kernel receives, the frame
count check, time padding, the cache, the nodes with a recorder pipeline, and the proof that the bounds of the GPU tests
(tests/envseq_refs.py) pass correct fp32 evaluations of both entries and fail the wrong ones."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import envmap_refs as ER
import envseq_refs as SR


@pytest.fixture(scope="module")
def pe(pkg):
    return ER.pe_module(pkg)


@pytest.fixture(autouse=True)
def _fresh_cache(pe):
    pe.clear_environment_cache()
    yield
    pe.clear_environment_cache()


def _lights(T=3, He=24, We=48):
    return torch.stack([torch.rand(He, We, 3, generator=torch.Generator().manual_seed(77 + k)).pow(4) * 50.0 for k in range(T)])


# ------------------------------------------------------------------------------------------------ reading the sequence
def test_process_comfyui_sequence_keeps_every_frame(pe):
    env = _lights(3)
    variants = {"nhwc": env, "nchw": env.permute(0, 3, 1, 2).contiguous(), "rgba": torch.cat([env, torch.ones_like(env[..., :1])], -1),
                "gray": env[..., :1].contiguous()}
    for k, v in variants.items():
        seq = pe.process_comfyui_sequence(v.clone())
        assert seq.shape == (3, 24, 48, 3), k
        assert torch.equal(seq[0], pe.process_comfyui_tensor(v.clone())), k                 # frame 0: what is read today
        for t in range(3):
            assert torch.equal(seq[t], pe.process_comfyui_tensor(v[t:t + 1].clone())), (k, t)
    one = pe.process_comfyui_sequence(env[0])
    assert one.shape == (1, 24, 48, 3) and torch.equal(one[0], pe.process_comfyui_tensor(env[0]))


def test_cube_sample_grid_is_the_grid_of_latlong_to_cubemap_official(pe):
    for (He, We), R in ((SR.PANO_SIZES[0], 8), (SR.PANO_SIZES[1], 32), (SR.PANO_SIZES[0], 64)):
        grid = pe.cube_sample_grid(R, "cpu")
        assert grid.shape == (6, R, R, 2) and grid.dtype == torch.float32 and grid.is_contiguous()
        assert pe.cube_sample_grid(R, "cpu") is grid                                          # once per (R, device)
        latlong = pe.apply_hdr_preprocessing(SR.panoramas(He, We)[1], 0.5, True, 37.0, "cpu")
        src = latlong.permute(2, 0, 1).unsqueeze(0)
        faces = [F.grid_sample(src, grid[s:s + 1], mode="bilinear", padding_mode="border", align_corners=False)[0].permute(1, 2, 0)
                 for s in range(6)]
        assert torch.equal(torch.stack(faces), pe.latlong_to_cubemap_official(latlong, [R, R]))


def test_sequence_roll_is_torchs_roll(pe):
    for We in (48, 31):
        for rot in (0.0, 90.0, 37.0, 359.0, 360.0, 180.0):
            x = torch.arange(We).view(1, We, 1).float().expand(2, We, 3)
            want = pe.apply_hdr_preprocessing(x, 1.0, False, rot, "cpu")
            roll = pe.sequence_roll(We, rot)
            assert 0 <= roll < We and torch.equal(want, torch.roll(x, roll, dims=1)), (We, rot)


# ------------------------------------------------------------------------------------------------ semantics
@pytest.mark.parametrize("spin", [0.0, 111.0])
def test_frame_t_is_the_static_call_on_frame_t(pe, spin):
    """Frame t of the sequence result == the single-light call on env_map[t:t+1] (under the same spin: its frame t)."""
    env = _lights(3)
    kw = dict(env_brightness=1.3, env_flip=True, env_rot=37.0, device="cpu", num_frames=3, use_cache=False, env_spin=spin)
    seq = pe.render_projection_from_panorama(env, (16, 24), env_sequence=True, **kw)
    off = pe.render_projection_from_panorama(env, (16, 24), **kw)
    for k in ("env_ldr", "env_log"):
        assert seq[k].shape == (3, 16, 24, 3)
        for t in range(3):
            one = pe.render_projection_from_panorama(env[t:t + 1], (16, 24), **kw)
            assert torch.equal(seq[k][t], one[k][t]), (k, t)
        assert torch.equal(seq[k][0], off[k][0]) and not torch.equal(seq[k][1], off[k][1])    # off: frame 0 lights every frame
    cond = pe.envmap_conditions(env, (16, 24), 3, "proj", 1.3, True, 37.0, device="cpu", env_spin=spin, env_sequence=True)
    assert cond["env_ldr"].shape == cond["env_log"].shape == (1, 3, 3, 16, 24) and cond["env_nrm"].shape == (1, 3, 1, 16, 24)
    assert torch.equal(cond["env_ldr"][0].permute(1, 2, 3, 0), seq["env_ldr"] * 2.0 - 1.0)


def test_one_frame_is_todays_path_and_todays_cache_key(pe):
    env = _lights(1)
    for source in (env, env[0]):
        pe.clear_environment_cache()
        a = pe.envmap_conditions(source, (8, 12), 4, "proj", 1.0, False, 90.0, device="cpu", env_sequence=True)
        keys = set(pe._env_cache.cache)
        pe.clear_environment_cache()
        b = pe.envmap_conditions(source, (8, 12), 4, "proj", 1.0, False, 90.0, device="cpu")
        assert keys == set(pe._env_cache.cache) and len(keys) == 1 and "seq" not in next(iter(keys))
        assert torch.equal(a["env_ldr"], b["env_ldr"]) and torch.equal(a["env_log"], b["env_log"])


def test_frame_count_must_match_the_clip(pe):
    env = _lights(3)
    with pytest.raises(ValueError, match=r"N = 3 .* T = 4"):
        pe.envmap_conditions(env, (8, 12), 4, "proj", device="cpu", env_sequence=True)
    with pytest.raises(ValueError, match=r"N = 3 .* T = 2"):
        pe.render_projection_from_panorama(env, (8, 12), device="cpu", num_frames=2, env_sequence=True, use_cache=False)
    with pytest.raises(ValueError, match=r"N = 3 .* T = 5"):                              # the clip's own count decides, not T'
        pe.envmap_conditions(env, (8, 12), 3, "ball", device="cpu", env_sequence=True, clip_frames=5)
    with pytest.raises(ValueError, match="ball"):
        pe.envmap_conditions(env, (8, 12), 3, "ball", device="cpu", env_spin=30.0, env_sequence=True)
    with pytest.raises(ValueError, match="hip"):
        pe.envmap_conditions(env, (8, 12), 3, "proj", device="cpu", backend="hip", env_sequence=True)
    with pytest.raises(ValueError, match="backend"):
        pe.envmap_conditions(env, (8, 12), 3, "proj", device="cpu", backend="triton", env_sequence=True)
    assert pe.get_cache_stats()["cache_size"] == 0
    pe.envmap_conditions(env, (8, 12), 4, "proj", device="cpu")                            # off: any N, as today


def test_time_padding_repeats_the_last_light(pe):
    """A fit pads T = 3 to T' = 5 and rescales the spin: frames 0..2 keep their light and their angle, 3 and 4 get light 2."""
    env = _lights(3)
    assert pe.sequence_cube_of(3, 5) == [0, 1, 2, 2, 2]
    spin = 90.0 * 5 / 3
    pad = pe.envmap_conditions(env, (8, 12), 5, "proj", 1.0, False, 0.0, device="cpu", env_spin=spin, env_sequence=True, clip_frames=3)
    assert pad["env_ldr"].shape == (1, 3, 5, 8, 12)
    for t, k in enumerate([0, 1, 2, 2, 2]):
        pe.clear_environment_cache()
        one = pe.envmap_conditions(env[k:k + 1], (8, 12), 5, "proj", 1.0, False, 0.0, device="cpu", env_spin=spin)
        assert torch.equal(pad["env_ldr"][:, :, t], one["env_ldr"][:, :, t]) and torch.equal(pad["env_log"][:, :, t], one["env_log"][:, :, t])


def test_ball_sequence_is_the_per_frame_calls(pe):
    env = _lights(3, 20, 20)
    for res in ((8, 12), (9, 13), (20, 20)):                                             # resized (to an odd size too), and at its own size
        pe.clear_environment_cache()
        seq = pe.envmap_conditions(env, res, 4, "ball", device="cpu", env_sequence=True, clip_frames=3)
        assert seq["env_ldr"].shape == (1, 3, 4) + res
        for t, k in enumerate([0, 1, 2, 2]):
            one = pe.tonemap_image_direct(env[k:k + 1], res, device="cpu", num_frames=1, use_cache=False)
            for name in ("env_ldr", "env_log"):
                assert torch.equal(seq[name][0, :, t].permute(1, 2, 0), one[name][0] * 2.0 - 1.0), (res, t, name)


def test_cache_tells_sequences_apart(pe):
    env = _lights(3)
    moved = env.clone()
    moved[1, 11, 23] += 40.0          # one texel of one frame: a small light that moved
    idx = torch.linspace(0, env.numel() - 1, 1000).long()
    assert torch.equal(env.reshape(-1)[idx], moved.reshape(-1)[idx])                       # the whole-tensor sample misses it ...
    assert pe.compute_tensor_hash(env) == pe.compute_tensor_hash(moved)
    assert pe._sequence_hash(env) != pe._sequence_hash(moved)                              # ... every frame's own does not

    def run(e, T=3, **kw):
        return pe.render_projection_from_panorama(e, (24, 48), 1.0, False, 0.0, "cpu", T, True, **kw)

    a = run(env, env_sequence=True)
    assert run(env, env_sequence=True) is a and pe.get_cache_stats()["cache_size"] == 1     # same call: hit
    b = run(moved, env_sequence=True)
    assert b is not a and pe.get_cache_stats()["cache_size"] == 2 and not torch.equal(a["env_log"][1], b["env_log"][1])
    assert torch.equal(a["env_log"][0], b["env_log"][0]) and torch.equal(a["env_log"][2], b["env_log"][2])
    run(env)                                                                                # off: today's key, another entry
    run(env, env_sequence=True, env_spin=120.0)                                             # the spin
    run(env, T=5, env_sequence=True, clip_frames=3)                                         # T'
    assert pe.get_cache_stats()["cache_size"] == 5
    keys = sorted(k.split("_", 1)[1] for k in pe._env_cache.cache)
    assert sum("proj_seq3_" in k for k in keys) == 4 and sum("_T5_" in k for k in keys) == 1
    pe.envmap_conditions(_lights(3, 20, 20), (8, 12), 3, "ball", device="cpu", env_sequence=True)
    assert any("ball_seq3_T3" in k for k in pe._env_cache.cache)


# ------------------------------------------------------------------------------------------------ nodes
class _Recorder:
    device = "cpu"
    batch_passes = False

    def set_model_type(self, t):
        self.model_type = t

    def generate_video(self, data_batch, normalize_normal=False, seed=None):
        self.batch = data_batch
        B, _, T, H, W = data_batch["video"].shape
        return np.full((B, T, H, W, 3), 128, dtype=np.uint8)


def _gbuffers(T, H, W):
    return [torch.rand(1, T, H, W, 3, generator=torch.Generator().manual_seed(5 + i)) for i in range(5)]


def test_nodes_declare_env_sequence(pkg):
    import importlib
    nodes = importlib.import_module(pkg.__name__ + ".nodes")
    for cls, fn in ((nodes.Cosmos1ForwardRenderer, "run_forward_pass"), (nodes.Cosmos1Relight, "run_relight")):
        kind, opt = cls.INPUT_TYPES()["optional"]["env_sequence"]
        assert kind == "BOOLEAN" and opt["default"] is False and "frame t" in opt["tooltip"]
        assert inspect.signature(getattr(cls, fn)).parameters["env_sequence"].default is False
    assert inspect.signature(nodes._forward_pass).parameters["env_sequence"].default is False


def test_forward_node_hands_the_sequence_on(pkg, pe, monkeypatch):
    seen = {}
    real = pe.envmap_conditions

    def recording(env_map, resolution, num_frames, *a, **kw):
        seen.update(num_frames=num_frames, env_sequence=kw.get("env_sequence"), clip_frames=kw.get("clip_frames"))
        return real(env_map, resolution, num_frames, *a, **kw)
    monkeypatch.setattr(pe, "envmap_conditions", recording)
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    p, env = _Recorder(), _lights(3, 16, 32)
    g = _gbuffers(3, 32, 32)
    node.run_forward_pass(p, *g, env, env_rotation=0.0)
    off = p.batch["env_ldr"].clone()
    assert seen == dict(num_frames=3, env_sequence=False, clip_frames=3)
    node.run_forward_pass(p, *g, env, env_rotation=0.0, env_sequence=True)
    on = p.batch["env_ldr"]
    assert seen == dict(num_frames=3, env_sequence=True, clip_frames=3) and on.shape == off.shape == (1, 3, 3, 32, 32)
    assert torch.equal(on[:, :, 0], off[:, :, 0]) and not torch.equal(on[:, :, 2], off[:, :, 2])
    for t in range(3):
        pe.clear_environment_cache()
        one = real(env[t:t + 1], (32, 32), 3, "proj", 1.0, False, 0.0, device="cpu")
        assert torch.equal(on[:, :, t], one["env_ldr"][:, :, t])
    # a fit that pads time: the un-padded T goes to the check, T' to the projection; the padded frames are cut away
    g10 = _gbuffers(10, 40, 36)
    env10 = _lights(10, 16, 32)
    (out,) = node.run_forward_pass(p, *g10, env10, env_rotation=0.0, env_sequence=True, fit="crop")
    assert seen == dict(num_frames=17, env_sequence=True, clip_frames=10) and out.shape == (1, 10, 32, 32, 3)
    pe.clear_environment_cache()
    last = real(env10[9:10], (32, 32), 17, "proj", 1.0, False, 0.0, device="cpu")
    for t in (9, 10, 16):
        assert torch.equal(p.batch["env_ldr"][:, :, t], last["env_ldr"][:, :, t])
    with pytest.raises(ValueError, match=r"N = 3 .* T = 10"):
        node.run_forward_pass(p, *g10, env, env_sequence=True, fit="crop")


# ------------------------------------------------------------------------------------------------ the bounds of the GPU tests
# every wrong variant of the cube build fails at (at least) the case named here; the test below asserts exactly that
CUBE_MUTANT_CASE = {
    "flip_lost": "24x48_R8_flip1_rot0", "roll_wrong_way": "24x48_R8_flip0_rot90", "roll_before_flip": "17x31_R32_flip1_rot37",
    "roll_rounded": "24x48_R32_flip0_rot37", "brightness_after_clamp": "b2.0_n0+3", "not_cleaned": "24x48_R8_flip0_rot0",
    "panorama_0": "n1+2", "n0_ignored": "n2+1", "grid_xy_swapped": "17x31_R8_flip0_rot0", "align_corners": "24x48_R32_flip0_rot0",
    "wrap": "24x48_R32_flip0_rot0", "he_we_exchanged": "17x31_R32_flip0_rot0"}


@pytest.mark.parametrize("i", range(len(SR.CUBE_CASES)), ids=SR.CUBE_CASE_IDS)
def test_cubes_bound_passes_a_correct_standin_and_fails_the_wrong_ones(pkg, i):
    assert SR.M_CUBES <= SR.M_MAX and SR.M_CUBES & (SR.M_CUBES - 1) == 0
    c = SR.cube_case(pkg, i)
    args = (c["latlong"], c["grid"], c["n0"], c["n"], c["brightness"], c["flip"], c["rot"])
    good = SR.cube_err(SR.standin_cubes(*args), c)
    print(f"env-seq case {SR.CUBE_CASE_IDS[i]}: E_ref {c['e_ref']:.3e}, stand-in / E_ref {good / c['e_ref']:.2f}")
    assert good <= SR.M_CUBES * c["e_ref"]
    assert set(CUBE_MUTANT_CASE) == set(SR.CUBE_MUTANTS)
    for mutant, where in CUBE_MUTANT_CASE.items():
        if where in SR.CUBE_CASE_IDS[i]:
            bad = SR.cube_err(SR.standin_cubes(*args, mutant=mutant), c)
            assert bad > SR.M_MAX * c["e_ref"], (mutant, bad, c["e_ref"])


def test_every_cube_mutant_names_a_case():
    for mutant, where in CUBE_MUTANT_CASE.items():
        assert any(where in cid for cid in SR.CUBE_CASE_IDS), (mutant, where)
    seen = {(c["brightness"], c["n0"]) for c in SR.CUBE_CASES}
    assert len(seen) == 9 and len(SR.CUBE_CASES) == 32


@pytest.mark.parametrize("i", range(len(SR.PROJ_CASES)), ids=SR.PROJ_CASE_IDS)
def test_projection_bound_passes_a_correct_standin_and_fails_the_wrong_ones(pkg, i):
    c = SR.proj_case(pkg, i)
    good, rest = SR.proj_err(SR.standin_project_seq(c), c)
    print(f"env-seq case {SR.PROJ_CASE_IDS[i]}: E_ref {c['e_ref']:.3e}, stand-in / E_ref {good / c['e_ref']:.2f}")
    assert rest and good <= ER.M_BOUND * c["e_ref"]
    for mutant in SR.PROJ_MUTANTS:
        bad, rest = SR.proj_err(SR.standin_project_seq(c, mutant=mutant), c)
        assert not rest or bad > ER.M_MAX * c["e_ref"], (mutant, bad, rest)
