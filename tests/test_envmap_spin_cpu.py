"""The rotating environment light (env_spin) on the CPU: the torch path that specifies it, its pin to the reference's own
functions (tests/golden/envmap.safetensors, written by tools/make_goldens.py from the reference), the cache, the errors, and the
proof that the GPU test's bound (tests/envmap_refs.py) passes a correct fp32 evaluation and fails the wrong ones."""
import math

import pytest
import torch

import envmap_refs as ER
from conftest import load_golden


@pytest.fixture(scope="module")
def pe(pkg):
    return ER.pe_module(pkg)


@pytest.fixture(scope="module")
def gold():
    return load_golden("envmap.safetensors")[0]


def _pano(gold):
    return gold["in.pano"]


# ------------------------------------------------------------------------------------------------ pinned to the reference
def test_process_comfyui_tensor_equals_reference(pe, gold):
    pano = _pano(gold)
    variants = {"bhwc": pano, "bchw": pano.permute(0, 3, 1, 2).contiguous(), "rgba": torch.cat([pano, torch.ones_like(pano[..., :1])], -1),
                "gray": pano[..., :1].contiguous(), "hwc": pano[0]}
    for k, v in variants.items():
        got, want = pe.process_comfyui_tensor(v.clone()), gold["process_comfyui_tensor." + k]
        assert got.shape == want.shape and torch.equal(got.nan_to_num(-7.0), want.nan_to_num(-7.0)), k   # NaN texel: same place


def test_hdr_preprocessing_equals_reference(pe, gold):
    latlong = pe.process_comfyui_tensor(_pano(gold))
    assert latlong.isnan().any() and latlong.isinf().any()
    for flip in (False, True):
        for rot in (0, 90, 180):
            got = pe.apply_hdr_preprocessing(latlong.clone(), 0.7, flip, float(rot), "cpu")
            assert torch.equal(got, gold[f"apply_hdr_preprocessing.b0.7.flip{int(flip)}.rot{rot}"]), (flip, rot)


def test_cubemap_directions_and_tone_maps_equal_reference(pe, gold):
    clean = gold["apply_hdr_preprocessing.b0.7.flip0.rot0"]
    cube = pe.latlong_to_cubemap_official(clean, [16, 16])
    want = gold["latlong_to_cubemap_official.16x16"]
    assert cube.shape == want.shape and (cube - want).abs().max() <= 1e-6                        # a grid_sample path
    for H, W in ((9, 14), (6, 20)):
        assert torch.equal(pe.latlong_vec((H, W), device="cpu"), gold[f"latlong_vec.{H}x{W}"])
    m = pe.hdr_mapping_official(want, log_scale=10000.0)
    assert torch.equal(m["env_ev0"], gold["hdr_mapping_official.env_ev0"])
    assert torch.equal(m["env_log"], gold["hdr_mapping_official.env_log"])


def test_tonemap_image_direct_equals_reference(pe, gold):
    clean = gold["apply_hdr_preprocessing.b0.7.flip0.rot0"]
    d = pe.tonemap_image_direct(clean.clone(), (16, 32), device="cpu", num_frames=2, use_cache=False)
    for k in ("env_ldr", "env_log"):
        assert torch.equal(d[k], gold[f"tonemap_image_direct.native.{k}"]), k
    d = pe.tonemap_image_direct(clean.clone(), (10, 14), device="cpu", num_frames=2, use_cache=False)
    for k in ("env_ldr", "env_log"):
        want = gold[f"tonemap_image_direct.resized.{k}"]
        assert d[k].shape == want.shape and (d[k] - want).abs().max() <= 1e-6, k                 # an interpolate path


ANGLES = {"0": 0.0, "37": 37.0, "90": 90.0, "m45": -45.0}


def test_rotate_y_and_spun_direction_equal_reference(pe, gold):
    """Pins the sign convention of the spin: rotate_y and the hook's `vec @ rotate_y(theta)[:3, :3].T`."""
    vec = pe.latlong_vec((9, 14), device="cpu")
    for tag, deg in ANGLES.items():
        ry = pe.rotate_y(math.radians(deg), device="cpu")
        assert ry.dtype == torch.float32 and torch.equal(ry, gold[f"rotate_y.{tag}"]), tag
        assert torch.equal(vec.view(-1, 3) @ ry[:3, :3].T, gold[f"vec_rotated.{tag}"]), tag
    # the table the kernel receives holds exactly the matrix entries, at theta_t = radians(spin) * t / T
    tab = pe.spin_table(111.0, 3)
    assert tab.shape == (3, 2) and tab.dtype == torch.float32
    for t in range(3):
        ry = pe.rotate_y(math.radians(111.0) * t / 3)
        assert tab[t, 0] == ry[0, 0] == ry[2, 2] and tab[t, 1] == ry[0, 2] == -ry[2, 0]


# ------------------------------------------------------------------------------------------------ semantics of env_spin
def test_spin_zero_is_todays_result_and_frame_zero_is_static(pe):
    env = ER.panorama()
    kw = dict(env_brightness=1.3, env_flip=True, env_rot=90.0, device="cpu", num_frames=3, use_cache=False)
    a = pe.render_projection_from_panorama(env, (16, 24), **kw)
    b = pe.render_projection_from_panorama(env, (16, 24), env_spin=0.0, **kw)
    c = pe.render_projection_from_panorama(env, (16, 24), env_spin=0.0, backend="torch", **kw)
    s = pe.render_projection_from_panorama(env, (16, 24), env_spin=111.0, **kw)
    for k in ("env_ldr", "env_log"):
        assert a[k].shape == (3, 16, 24, 3) and torch.equal(a[k], b[k]) and torch.equal(a[k], c[k])
        assert s[k].shape == (3, 16, 24, 3) and torch.equal(s[k][0], a[k][0])          # theta_0 = 0: cos 1, sin 0, exact
        assert not torch.equal(s[k][1], a[k][1]) and not torch.equal(s[k][2], s[k][1])
    e0 = pe.envmap_conditions(env, (16, 24), 3, "proj", 1.3, True, 90.0, device="cpu")
    e1 = pe.envmap_conditions(env, (16, 24), 3, "proj", 1.3, True, 90.0, device="cpu", env_spin=111.0)
    assert e1["env_ldr"].shape == e1["env_log"].shape == (1, 3, 3, 16, 24) and e1["env_nrm"].shape == (1, 3, 1, 16, 24)
    assert torch.equal(e1["env_nrm"], e0["env_nrm"])                                   # camera-space directions do not turn
    assert torch.equal(e1["env_ldr"][0].permute(1, 2, 3, 0), s["env_ldr"] * 2.0 - 1.0)
    pe.clear_environment_cache()


def test_quarter_turn_rolls_the_image(pe):
    """W = 32, T = 4, spin 360: frame 1 is turned by +90 degrees, which on a lat-long image is a roll by -W/4 columns.
    Bound 1e-5: the two images differ by the rounding of the turned directions (a few 2^-24 relative, times 256 texels of a cube
    face: ~1e-4 texel of a panorama that changes by < 0.01 per cube texel) and by a few ulp of tone maps in [0, 1] (~5e-7);
    turned the wrong way round the images are 0.1 and more apart."""
    env = ER.smooth_panorama()
    kw = dict(env_brightness=1.0, env_flip=False, env_rot=0.0, device="cpu", num_frames=4, use_cache=False)
    s = pe.render_projection_from_panorama(env, (16, 32), env_spin=360.0, **kw)
    st = pe.render_projection_from_panorama(env, (16, 32), **kw)
    for k in ("env_ldr", "env_log"):
        right = (s[k][1] - torch.roll(st[k][0], -8, dims=1)).abs().max().item()
        wrong = (s[k][1] - torch.roll(st[k][0], 8, dims=1)).abs().max().item()
        half = (s[k][2] - torch.roll(st[k][0], 16, dims=1)).abs().max().item()
        print(f"{k}: quarter turn {right:.2e} (wrong way {wrong:.2e}), half turn {half:.2e}")
        assert right <= 1e-5 and half <= 1e-5 and wrong > 0.1


def test_cache_tells_spin_and_frames_apart(pe):
    pe.clear_environment_cache()
    env = ER.panorama()

    def run(T, spin):
        return pe.render_projection_from_panorama(env, (8, 12), 1.0, False, 0.0, "cpu", T, True, env_spin=spin)

    a = run(3, 120.0)
    assert pe.get_cache_stats()["cache_size"] == 1
    assert run(3, 120.0) is a and pe.get_cache_stats()["cache_size"] == 1              # same call: hit
    b = run(3, 240.0)
    assert b is not a and pe.get_cache_stats()["cache_size"] == 2                      # another spin: miss
    c = run(4, 120.0)
    assert c["env_ldr"].shape[0] == 4 and pe.get_cache_stats()["cache_size"] == 3      # another T under spin: miss
    d = run(3, 0.0)
    assert pe.get_cache_stats()["cache_size"] == 4 and torch.equal(d["env_ldr"][0], a["env_ldr"][0])
    pe.clear_environment_cache()


def test_errors(pe):
    env = ER.panorama()
    with pytest.raises(ValueError, match="ball"):
        pe.envmap_conditions(torch.rand(20, 20, 3), (8, 12), 2, "ball", device="cpu", env_spin=30.0)
    assert pe.envmap_conditions(torch.rand(20, 20, 3), (8, 12), 2, "ball", device="cpu", env_spin=0.0)["env_ldr"].shape == (1, 3, 2, 8, 12)
    with pytest.raises(ValueError, match="hip"):
        pe.render_projection_from_panorama(env, (8, 12), device="cpu", num_frames=2, env_spin=30.0, backend="hip", use_cache=False)
    with pytest.raises(ValueError, match="hip"):
        pe.envmap_conditions(env, (8, 12), 2, device="cpu", backend="hip")
    with pytest.raises(ValueError, match="backend"):
        pe.render_projection_from_panorama(env, (8, 12), device="cpu", backend="triton", use_cache=False)
    pe.clear_environment_cache()


def test_forward_node_declares_env_spin(pkg):
    import inspect
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]
    assert node.INPUT_TYPES()["optional"]["env_spin"] == ("FLOAT", {"default": 0.0, "min": -720.0, "max": 720.0, "step": 1.0})
    assert inspect.signature(node.run_forward_pass).parameters["env_spin"].default == 0.0


# ------------------------------------------------------------------------------------------------ the bound of the GPU test
@pytest.mark.parametrize("i", range(len(ER.CASES)), ids=ER.CASE_IDS)
def test_bound_passes_a_correct_standin_and_fails_the_wrong_ones(pkg, i):
    """M_BOUND * E_ref (what tests/test_envmap_gpu.py asks of the kernel) holds for an independent fp32 evaluation and is missed by
    every mistake the kernel could plausibly make."""
    assert ER.M_BOUND <= ER.M_MAX and ER.M_BOUND & (ER.M_BOUND - 1) == 0
    H, W, T, spin, R = ER.CASES[i]
    c = ER.case(pkg, i)
    bound = ER.M_BOUND * c["e_ref"]
    good = ER.max_err(ER.standin(c["cube"], c["vec"], spin, T), c["ref"], c["mask"])
    print(f"case {ER.CASE_IDS[i]}: E_ref {c['e_ref']:.3e}, tie share {c['mask'].float().mean().item():.4f}, stand-in / E_ref {good / c['e_ref']:.2f}")
    assert good <= bound
    for mutant in ER.MUTANTS:
        bad = ER.max_err(ER.standin(c["cube"], c["vec"], spin, T, mutant=mutant), c["ref"], c["mask"])
        assert bad > ER.M_MAX * c["e_ref"], (mutant, bad, bound)
