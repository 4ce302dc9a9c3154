"""The comparators of tests/vae_refs.py must bite (no GPU needed): every bound that tests/test_vae_kernels_gpu.py puts on a
tokenizer kernel is run here on the same inputs against (a) a plain torch stand-in with the kernel's rounding points, which
must PASS - a correct bf16 implementation stays inside every cap - and (b) subtly wrong versions of that stand-in, which must
FAIL the same check."""
import pytest
import torch

import vae_refs as R

BF = torch.bfloat16
S3, T3 = (1, 3, 3), (3, 1, 1)


def _conv_checks(g, size, integer, mutant, cin_live=None, seed=3):
    T, H, W = size
    x, w, b, res = R.conv_inputs(g, T, H, W, integer, seed=seed, cin_live=cin_live)
    ref, mag = R.conv_ref(g, x, w, b, res, T, H, W)
    out = R.conv_standin(g, x, w, b, res, T, H, W, mutant)
    if integer:
        return torch.equal(out, ref.to(BF)), f"{(out != ref.to(BF)).sum().item()} of {out.numel()} differ"
    r = R.ulp_check(out, ref, mag=mag, max_ulp=2 if res is not None else 1, frac_exact=0.97 if res is not None else 0.98)
    return r["ok"], R.fmt(r)


@pytest.mark.parametrize("integer", [True, False])
def test_conv_standin_passes_every_model_case(integer):
    """The random-data cases exactly as the GPU test builds them (same sizes, same seed); the integer form at the ragged size."""
    bad = []
    for tag, g, live in R.conv_model_cases():
        ok, msg = _conv_checks(g, R.conv_sizes(g)[2] if integer else R.conv_model_size(g), integer, None, live,
                               seed=3 if integer else R.CONV_MODEL_SEED)
        print(f"conv stand-in {tag} integer={integer}: {msg}")
        if not ok:
            bad.append((tag, msg))
    assert not bad, bad


def test_conv_exact_integer_outputs_exercise_the_bf16_rounding():
    g = R.geom(512, 512, S3, pad=1, res="fresh")
    T, H, W = R.conv_sizes(g)[2]
    x, w, b, res = R.conv_inputs(g, T, H, W, True, seed=3)
    ref, _ = R.conv_ref(g, x, w, b, res, T, H, W)
    inexact = (ref.to(BF).double() != ref).double().mean().item()
    assert inexact > 0.2, inexact
    g0 = g._replace(res=None)
    conv, _ = R.conv_ref(g0, x, w, b, None, T, H, W)
    assert conv.abs().max() < 2 ** 24 and torch.equal(conv, conv.round())


CONV_MUTANTS = [
    ("swap_khkw", R.geom(128, 128, S3, pad=1)),
    ("border_tap", R.geom(128, 128, S3, pad=1)),
    ("zero_causal", R.geom(128, 128, T3)),
    ("t_off", R.geom(128, 128, T3, stride=(2, 1, 1), t_off=2, res="fresh")),
    ("bias_late", R.geom(128, 128, S3, pad=1)),
]


@pytest.mark.parametrize("mutant,g", CONV_MUTANTS, ids=[m for m, _ in CONV_MUTANTS])
@pytest.mark.parametrize("integer", [True, False])
def test_conv_mutants_are_caught(mutant, g, integer):
    size = R.conv_sizes(g)[2]
    ok, msg = _conv_checks(g, size, integer, None)
    assert ok, ("the unmutated stand-in must pass", msg)
    ok, msg = _conv_checks(g, size, integer, mutant)
    print(f"conv mutant {mutant} integer={integer}: caught={not ok}  {msg}")
    assert not ok, (mutant, msg)


# ------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("C,H,W", R.GN_CASES)
def test_groupnorm_standins_pass_the_centred_bound(C, H, W):
    x, gm, bt = R.gn_inputs(C, H, W, "centred")
    ref = R.gn_ref(x, gm, bt, False)
    for name, y in (("torch bf16", R.gn_torch_bf16(x, gm, bt, False)), ("kernel arithmetic", R.gn_standin(x, gm, bt, False)),
                    ("fp32 variance", R.gn_standin(x, gm, bt, False, mutant="fp32_var"))):
        r = R.ulp_check(y, ref, max_ulp=1, frac_exact=0.995)
        print(f"groupnorm {name} C{C} {H}x{W} centred: {R.fmt(r)}")
        assert r["ok"], (name, R.fmt(r))
    r = R.ulp_check(R.gn_standin(x, gm, bt, False, mutant="frame0"), ref, max_ulp=1, frac_exact=0.995)
    assert not r["ok"], ("frame 0's statistics for every frame must be caught", R.fmt(r))


@pytest.mark.parametrize("C,H,W", R.GN_OFFSET_CASES)
def test_groupnorm_offset_frames_catch_the_fp32_variance(C, H, W):
    """Frames with mean / std of 32 .. 250: forming the variance from sums already cast to fp32 cancels; the fp64 form does not."""
    x, gm, bt = R.gn_inputs(C, H, W, "offset")
    ref = R.gn_ref(x, gm, bt, False)
    yard = R.ulp_check(R.gn_torch_bf16(x, gm, bt, False), ref, max_ulp=1, frac_exact=0.0)
    good = R.ulp_check(R.gn_standin(x, gm, bt, False), ref, max_ulp=1, frac_exact=yard["exact"] - 0.01)
    mut = R.ulp_check(R.gn_standin(x, gm, bt, False, mutant="fp32_var"), ref, max_ulp=1, frac_exact=yard["exact"] - 0.01)
    print(f"groupnorm offset C{C} {H}x{W}: torch bf16 {R.fmt(yard)} | fp64 variance {R.fmt(good)} | fp32 variance {R.fmt(mut)}")
    assert yard["bad"] == 0, R.fmt(yard)
    assert good["ok"], R.fmt(good)
    assert not mut["ok"], R.fmt(mut)


def test_groupnorm_silu_standin_stays_inside_twice_torchs_mismatch_share():
    x, gm, bt = R.gn_inputs(256, 6, 21, "centred")
    ref = R.gn_ref(x, gm, bt, True)
    t = R.ulp_check(R.gn_torch_bf16(x, gm, bt, True), ref, max_ulp=1, frac_exact=0.0)
    k = R.ulp_check(R.gn_standin(x, gm, bt, True), ref, max_ulp=1, frac_exact=0.0)
    print(f"groupnorm+silu: torch {R.fmt(t)} | kernel arithmetic {R.fmt(k)}")
    assert t["bad"] == 0 and k["bad"] == 0
    assert 1 - k["exact"] <= 2 * (1 - t["exact"]) + 1e-3


# ------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("n,extra", R.SOFTMAX_CASES)
@pytest.mark.parametrize("scale", [1.0, 512 ** -0.5])
def test_softmax_bound_passes_fp32_and_catches_small_probability_errors(n, extra, scale):
    _, s = R.softmax_inputs(n, extra, scale)
    ref = R.softmax_ref(s, scale)
    r = R.softmax_check(R.softmax_standin(s, scale), ref)
    print(f"softmax stand-in n={n} scale={scale:.4f}: {R.fmt(r)}")
    assert r["ok"], R.fmt(r)
    mut = R.softmax_standin(s, scale, mutant="small_3pct")
    if n >= 2304:        # today's assertion lets the mutant through where most of the row is small probabilities
        assert torch.allclose(mut[:4].float(), ref[:4].float(), atol=4e-3, rtol=8e-3)
    assert not R.softmax_check(mut, ref)["ok"]


# ------------------------------------------------------------------------------------------------ temporal attention
@pytest.mark.parametrize("T,C,P", R.TATTN_CASES)
def test_temporal_attention_bound(T, C, P):
    q, k, v = R.tattn_inputs(T, C, P)
    scale = C ** -0.5
    ref, mag = R.attn_ref(q, k, v, scale, True)
    for name, out in (("P in bf16", R.tattn_standin(q, k, v, scale)), ("P in fp32", R.tattn_standin(q, k, v, scale, p_bf16=False))):
        r = R.attn_check(out, ref, mag)
        print(f"temporal attention stand-in ({name}) T{T} C{C} P{P}: {R.fmt(r)}")
        assert r["ok"], (name, R.fmt(r))
    if T > 1:
        r = R.attn_check(R.tattn_standin(q, k, v, scale, mutant="no_mask"), ref, mag)
        assert not r["ok"], ("attention without the causal mask must be caught", R.fmt(r))


@pytest.mark.parametrize("P", R.SPATIAL_ATTN_KEYS)
def test_spatial_attention_chain_bound(P):
    q, k, v = (t[:, None] for t in R.spatial_attn_inputs(P))
    scale = 512 ** -0.5
    ref, mag = R.attn_ref(q, k, v, scale, False)
    r = R.attn_check(R.tattn_standin(q, k, v, scale, causal=False), ref, mag)
    print(f"spatial attention stand-in P{P}: {R.fmt(r)}")
    assert r["ok"], R.fmt(r)
    vbad = torch.roll(v, 1, 0)                                  # V rows shifted by one key: a transposed / shifted V^T must be caught
    assert not R.attn_check(R.tattn_standin(q, k, vbad, scale, causal=False), ref, mag)["ok"]


# ------------------------------------------------------------------------------------------------ layout, resampling
def test_planar_to_cl_reference_catches_a_written_tail():
    x = R.rnd((16, 2, 3, 5), seed=1)
    fill = torch.full((2, 5, 7, 64), 7.0, dtype=BF)
    ref = R.planar_to_cl_ref(x, 64, 1, fill)
    assert torch.equal(R.planar_to_cl_standin(x, 64, 1, fill), ref)
    assert not torch.equal(R.planar_to_cl_standin(x, 64, 1, fill, mutant="tail"), ref)
    assert torch.equal(ref[:, 1:4, 1:6, :16].permute(3, 0, 1, 2), x) and (ref[:, 0] == 7).all() and (ref[..., 16:] == 7).all()


@pytest.mark.parametrize("T", [1, 2, 4, 5])
def test_resample_reference_equals_the_fp32_restatement(T):
    """The fp64 means rounded once equal the kernel's fp32 expression ((a + b) + d) + e) * 0.25 on these inputs."""
    x = R.rnd((64, T, 6, 8), seed=18)
    xf = x.float()
    m0 = ((((xf[:, :, 0::2, 0::2] + xf[:, :, 0::2, 1::2]) + xf[:, :, 1::2, 0::2]) + xf[:, :, 1::2, 1::2]) * 0.25).to(BF)
    assert torch.equal(R.resample_ref(x, 0), m0)
    To = (T + 1) // 2
    m1 = torch.stack([(xf[:, max(2 * t - 1, 0)] + xf[:, min(2 * t, T - 1)]) * 0.5 for t in range(To)], 1).to(BF)
    assert torch.equal(R.resample_ref(x, 1), m1)
    assert R.resample_ref(x, 2).shape[1] == (2 * T - 1 if T > 1 else 1)
    assert all(torch.equal(R.resample_ref(x, 2)[:, t], x[:, (t + 1) // 2]) for t in range(R.resample_ref(x, 2).shape[1]))
    assert R.resample_ref(x, 3).shape == (64, T, 12, 16) and torch.equal(R.resample_ref(x, 3)[:, :, 1::2, 0::2], x)


def test_ulp_check_counts_ulps_of_the_terms_when_given_a_magnitude():
    ref = torch.tensor([1.0, 0.001, 100.0], dtype=torch.float64)
    out = torch.tensor([1.0 + 2.0 ** -7, 0.001, 100.0], dtype=BF)
    assert R.ulp_check(out, ref, max_ulp=1, frac_exact=0.5, atol_rel=0.0)["ok"]
    out[0] = 1.0 + 2.0 ** -5
    r = R.ulp_check(out, ref, max_ulp=1, frac_exact=0.5, atol_rel=0.0)
    assert not r["ok"] and r["bad"] == 1 and 3.5 < r["worst_ulp"] < 4.1
    assert R.ulp_check(out, ref, mag=torch.full((3,), 8.0), max_ulp=1, frac_exact=0.5, atol_rel=0.0)["ok"]
    assert not R.ulp_check(out, ref, mag=torch.full((3,), 8.0), max_ulp=1, frac_exact=0.9, atol_rel=0.0)["ok"]
