"""Long clips on the host: the window planner's properties over a grid, the blend reference, and the proof that the inputs
of tests/test_windows_gpu.py can tell a wrong post-process kernel from a right one.  No GPU."""
import numpy as np
import pytest
import torch

import window_refs as R
from oracle import dit_oracle as O


def _legal(Wf):
    return range(0, (Wf - 1) // 2 + 1)


@pytest.mark.parametrize("Wf", [9, 17, 57])
def test_plan_properties_over_the_grid(pkg, Wf):
    plan_windows, ramp_weights = pkg.windows.plan_windows, pkg.windows.ramp_weights
    for Ov in _legal(Wf):
        w = ramp_weights(Ov)
        assert w.dtype == np.float32 and w.shape == (Ov,)
        assert all(np.float32((j + 1) / (Ov + 1)) == w[j] for j in range(Ov))
        assert all(0.0 < x < 1.0 for x in w) and all(w[j] < w[j + 1] for j in range(Ov - 1))
        for T in range(1, 201):
            plan = plan_windows(T, Wf, Ov)
            if T <= Wf:
                assert plan == [pkg.windows.Window(0, 0, 0, T, 0)]
                continue
            stride = Wf - Ov
            n = -(-(T - Ov) // stride)
            assert len(plan) == n >= 2
            assert [p.start for p in plan] == [i * stride for i in range(n - 1)] + [T - Wf]
            at = 0
            for i, p in enumerate(plan):
                assert 0 <= p.start and p.start + Wf <= T                       # every window has the full length, inside the clip
                assert p.write_lo == p.ramp_at and p.write_hi == (Wf if i == n - 1 else Wf - Ov)
                assert 0 <= p.write_lo < p.write_hi <= Wf
                assert p.out_at == p.start + p.write_lo == at                   # the written ranges tile [0, T) once, in order
                at += p.write_hi - p.write_lo
                if i == 0:
                    assert p.ramp_at == 0
                else:
                    q = plan[i - 1]
                    # the ramp is exactly the predecessor's last Ov frames (its carry, the frames it did not write) ...
                    assert p.start + p.ramp_at == q.start + Wf - Ov == q.start + q.write_hi
                    # ... and lies inside this window too
                    assert 0 <= p.ramp_at and p.ramp_at + Ov <= Wf
            assert at == T


def test_plan_examples(pkg):
    W = pkg.windows.Window
    plan = pkg.windows.plan_windows
    assert plan(21, 9, 2) == [W(0, 0, 0, 7, 0), W(7, 0, 0, 7, 7), W(12, 2, 2, 9, 14)]     # last window shifted back: 2 frames discarded
    assert plan(106, 57, 8) == [W(0, 0, 0, 49, 0), W(49, 0, 0, 57, 49)]                   # two windows cover 2 * 57 - 8 frames
    assert plan(113, 57, 8) == [W(0, 0, 0, 49, 0), W(49, 0, 0, 49, 49), W(56, 42, 42, 57, 98)]
    assert plan(17, 9, 1) == [W(0, 0, 0, 8, 0), W(8, 0, 0, 9, 8)]
    assert plan(18, 9, 0) == [W(0, 0, 0, 9, 0), W(9, 0, 0, 9, 9)]                          # hard cuts


@pytest.mark.parametrize("T,Wf,Ov", [(20, 8, 0), (20, 10, 2), (20, 1, 0), (20, 0, 0), (20, 9, 5), (20, 9, -1), (20, 57, 29),
                                     (0, 9, 2), (-3, 9, 2), (20, 9.0, 2), (20, 9, 1.5), (20, "9", 2), (20, True, 0)])
def test_plan_rejects_illegal_arguments(pkg, T, Wf, Ov):
    with pytest.raises(ValueError):
        pkg.windows.plan_windows(T, Wf, Ov)


def test_ramp_weights_reject(pkg):
    for bad in (-1, 1.5, None):
        with pytest.raises(ValueError):
            pkg.windows.ramp_weights(bad)
    assert pkg.windows.ramp_weights(0).shape == (0,)


def test_blend_reference_is_postprocess_without_a_ramp(pkg):
    for normalize in (False, True):
        v, p = R.case_inputs(2, 5, 7, 2)
        assert torch.equal(R.blend_postprocess(v, None, None, 0, 0, R.TW, normalize), O.postprocess(v, normalize))
        assert torch.equal(R.blend_postprocess(v, None, None, 3, 3, 7, normalize), O.postprocess(v[:, :, 3:7], normalize))
        # with a ramp, the frames outside it are still the plain post-process and the ramp frames are not
        w = R.ramp_table(pkg, 2)
        got, plain = R.blend_postprocess(v, p, w, 3, 0, R.TW, normalize), O.postprocess(v, normalize)
        assert torch.equal(got[:, :3], plain[:, :3]) and torch.equal(got[:, 5:], plain[:, 5:])
        assert not torch.equal(got[:, 3:5], plain[:, 3:5])


def test_blend_reference_spells_the_contract(pkg):
    """One value by hand: three fp32 roundings, then bf16."""
    a, b, w = np.float32(0.328125), np.float32(-0.77734375), np.float32(2 / 3)
    want = np.float32(a + np.float32(w * np.float32(b - a)))
    v = torch.full((1, 3, R.TW, 1, 1), float(b)).to(R.BF)
    p = torch.full((1, 3, 2, 1, 1), float(a)).to(R.BF)
    wt = torch.tensor([0.5, float(w)])
    got = R.blend_postprocess(v, p, wt, 0, 1, 2, False)
    ref = O.postprocess(torch.full((1, 3, 1, 1, 1), float(want)).to(R.BF), False)
    assert torch.equal(got, ref)


def _changed(video, prev, w, geo, normalize, variant):
    ref = R.blend_postprocess(video, prev, w, *geo, normalize)
    return int((R.blend_postprocess(video, prev, w, *geo, normalize, variant=variant) != ref).sum())


def test_value_grid_separates_every_wrong_kernel(pkg):
    """The value-grid tensors of the GPU test: every stand-in changes output bytes - the fused blend among them, for each ramp
    table whose weights do not multiply exactly (O = 1 is w = 1/2: fused and unfused agree for every input, and a reversed
    one-entry table is the table)."""
    vals = R.bf16_values()
    assert vals.numel() == 2 * (0x4080 + 1) and all(x in vals.float() for x in (0.0, 1.0, -1.0, 4.0, -4.0))
    assert (vals.view(torch.int16) == -32768).any()                            # -0 is there
    for knee in (0.2, 0.4):
        assert torch.tensor(knee).to(R.BF) in vals
    for Ov in R.GRID_OVERLAPS:
        video, prev = R.value_grid(Ov)
        assert video.shape == (1, 3, R.TW, *R.GRID_HW) and prev.shape == (1, 3, Ov, *R.GRID_HW)
        for j in range(Ov):                                                     # every value is a carry value of every ramp frame
            assert torch.equal(torch.unique(prev[:, :, j].reshape(-1).view(torch.int16)), torch.unique(vals.view(torch.int16)))
        w = R.ramp_table(pkg, Ov)
        for normalize in (False, True):
            for variant in R.VARIANTS:
                n = _changed(video, prev, w, (0, 0, R.TW), normalize, variant)
                exact = Ov == 1 and variant in ("fma", "fma_sub_rounded", "reversed")
                no_normal = variant == "after_normal" and not normalize
                print(f"value grid O={Ov} normalize={normalize} {variant}: {n} bytes differ")
                assert (n == 0) if (exact or no_normal) else (n >= 8), (Ov, normalize, variant, n)


def test_small_cases_separate_the_wrong_kernels(pkg):
    """The small-shape cases of the GPU test, taken together: every stand-in but the fused blends (the value grid's business)
    changes bytes at every shape."""
    for H, W in R.SHAPES:
        hits = {v: 0 for v in R.VARIANTS}
        for B in (1, 2):
            for Ov in R.OVERLAPS[1:]:
                video, prev = R.case_inputs(B, H, W, Ov)
                w = R.ramp_table(pkg, Ov)
                for geo in R.case_geometries(Ov):
                    for variant in R.VARIANTS:
                        hits[variant] += _changed(video, prev, w, geo, True, variant)
        for variant in R.VARIANTS:
            if not variant.startswith("fma"):
                assert hits[variant] > 0, (H, W, variant)


def test_node_inputs_and_pipeline_attributes(pkg):
    P = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline
    p = P("/ckpt", "m.pt")
    assert (p.window_frames, p.window_overlap) == (0, 8)
    for name in ("Cosmos1InverseRenderer", "Cosmos1ForwardRenderer"):
        opt = pkg.NODE_CLASS_MAPPINGS[name].INPUT_TYPES()["optional"]
        assert opt["window_frames"][0] == "INT" and opt["window_frames"][1]["default"] == 0
        assert "57" in opt["window_frames"][1]["tooltip"]
        assert opt["window_overlap"][0] == "INT" and opt["window_overlap"][1]["default"] == 8
    # windows off: no plan, whatever the clip; windows on: planner errors surface, a short clip keeps today's path
    p.device = torch.device("cpu")
    clip = {"rgb": torch.zeros(1, 3, 21, 8, 8)}
    assert p._window_plan(clip) is None
    p.window_frames, p.window_overlap = 9, 2
    assert [w.start for w in p._window_plan(clip)] == [0, 7, 12]
    assert p._window_plan({"rgb": torch.zeros(1, 3, 9, 8, 8)}) is None
    p.window_overlap = 5
    with pytest.raises(ValueError, match="window_overlap"):
        p.generate_video(clip)
    p.window_frames, p.window_overlap = 10, 2
    with pytest.raises(ValueError, match="window_frames"):
        p.generate_video(clip)


def test_static_light_follows_the_clip_length_through_the_cache(pkg):
    """A long clip and then one of its windows alone use the same environment map at two lengths: the cached static frame (its key
    carries no T) comes back at the length asked for, in both env formats."""
    import importlib
    pe = importlib.import_module(pkg.__name__ + ".preprocess_envmap")
    pe.clear_environment_cache()
    env = pkg.synthetic_weights.synth_tensor("win.env", (1, 16, 32, 3), torch.float32).abs() * 4.0
    for fmt in ("proj", "ball"):
        long = pe.envmap_conditions(env, (16, 16), 17, fmt, device="cpu")
        short = pe.envmap_conditions(env, (16, 16), 9, fmt, device="cpu")
        for k in ("env_ldr", "env_log"):
            assert long[k].shape == (1, 3, 17, 16, 16) and short[k].shape == (1, 3, 9, 16, 16), (fmt, k)
            assert torch.equal(short[k], long[k][:, :, :9])
    pe.clear_environment_cache()


def test_windows_under_sequence_parallelism_are_refused(pkg):
    P = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline

    class _Sharded:
        process_group = object()
    p = P("/ckpt", "m.pt", model_instance=_Sharded())
    p.window_frames = 9
    with pytest.raises(NotImplementedError):
        p.generate_video({"rgb": torch.zeros(1, 3, 21, 8, 8)})
