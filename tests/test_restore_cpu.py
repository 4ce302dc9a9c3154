"""The fit's way back on the CPU (fit.plan_restore / restore_frames): the plan's rules, its tables against F.interpolate in
float64, the torch specification against the bound of tests/restore_refs.py and bit for bit where the weights are dyadic, the
wrong stand-ins that bound has to catch, the nodes' `fit_restore` input and the pipeline's `restore_plan` attribute."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import restore_refs as R


@pytest.fixture(scope="module")
def fit(pkg):
    return R.fit_module(pkg)


# ----------------------------------------------------------------------------------------------- plan
def test_stretch_can_always_be_restored(fit):
    for H, W in [(h, 16 + (h * 11) % 115) for h in range(16, 131, 3)]:
        for fh, fw in ((0, 0), (32, 0), (0, 48), (64, 32), (16, 128)):
            p = fit.plan_fit(10, H, W, "stretch", fh, fw)
            r = fit.plan_restore(p)
            assert (r.T, r.H_model, r.W_model, r.H, r.W) == (10, p.H_out, p.W_out, H, W)
            assert tuple(r.y_lo_n.shape) == (H, 2) and tuple(r.x_lo_n.shape) == (W, 2)
            assert r.y_lo_n.dtype == torch.int32 and r.y_w.dtype == torch.float32 and r.x_w.dtype == torch.float32
            assert r.y_w.shape[0] == H and r.x_w.shape[0] == W
            for lo_n, w, n_in, n_out in ((r.y_lo_n, r.y_w, p.H_out, H), (r.x_lo_n, r.x_w, p.W_out, W)):
                lo, n = lo_n[:, 0].long(), lo_n[:, 1].long()
                assert (lo >= 0).all() and (n >= 1).all() and (lo + n <= n_in).all() and int(n.max()) == w.shape[1]
                assert (w.double().sum(dim=1) - 1.0).abs().max() <= 1e-6
                if n_out >= n_in:
                    assert w.shape[1] <= 2                                    # an up-scale has at most 2 taps per axis
                y, _ = fit.axis_taps(n_in, n_out, 0, n_out)
                assert torch.equal(lo_n, torch.from_numpy(y))                 # the tables are axis_taps(H', H, 0, H)
            assert r.identity == ((p.H_out, p.W_out) == (H, W))


def test_crop_that_cut_nothing_can_be_restored(fit):
    p = fit.plan_fit(57, 1080, 1920, "crop", 576, 1024)
    assert (p.y0, p.x0, p.H_full, p.W_full) == (0, 0, 576, 1024)
    r = fit.plan_restore(p)
    assert (r.T, r.H_model, r.W_model, r.H, r.W) == (57, 576, 1024, 1080, 1920) and not r.identity
    assert r.y_w.shape[1] == 2 and r.x_w.shape[1] == 2
    s = fit.plan_restore(fit.plan_fit(57, 1080, 1920, "stretch", 576, 1024))
    assert torch.equal(r.y_lo_n, s.y_lo_n) and torch.equal(r.y_w, s.y_w) and torch.equal(r.x_w, s.x_w)
    # a clip already on the grid: a crop that is the identity
    r = fit.plan_restore(fit.plan_fit(9, 32, 48, "crop"))
    assert r.identity and (r.H, r.W) == (32, 48)


def test_crop_that_cut_cannot_be_restored(fit):
    for args in ((9, 70, 75, "crop"), (9, 70, 75, "crop", 32, 32), (57, 1080, 1920, "crop"), (9, 40, 36, "crop", 32, 32)):
        p = fit.plan_fit(*args)
        with pytest.raises(ValueError, match="crop cannot be undone") as e:
            fit.plan_restore(p)
        assert "stretch" in str(e.value)


def test_identity_is_detected_and_only_cuts_in_time(fit):
    r = fit.plan_restore(fit.plan_fit(10, 32, 48, "stretch"))
    assert r.identity and r.T == 10 and r.y_w.shape[1] == 1 and bool((r.x_w == 1.0).all())
    u8 = R.source(2, 17, 32, 48)
    out = fit.restore_frames(u8, r)
    assert out.shape == (2, 10, 32, 48, 3) and torch.equal(out, u8[:, :10])
    assert out.data_ptr() == u8.data_ptr()                                    # the input, cut: nothing computed
    assert not fit.plan_restore(fit.plan_fit(10, 32, 49, "stretch")).identity


def test_max_taps_refusal(fit):
    # 16 rows stretched to 16 * 17 by the fit (an up-scale: 2 taps) come back through a 17x shrink: 35 taps
    p = fit.plan_fit(1, 16, 64, "stretch", 16 * 17, 64)
    with pytest.raises(ValueError, match="taps"):
        fit.plan_restore(p)
    assert fit.plan_restore(fit.plan_fit(1, 16, 64, "stretch", 16 * 15, 64)).y_w.shape[1] <= fit.MAX_TAPS


# ----------------------------------------------------------------------------------------------- tables and specification
def test_tables_in_float64_equal_interpolate_in_float64(pkg, fit):
    worst = 0.0
    for g in R.GEOMETRIES + R.DYADIC:
        (hm, wm), (h, w) = g
        y_lo_n, y_w = fit.axis_taps(hm, h, 0, h)
        x_lo_n, x_w = fit.axis_taps(wm, w, 0, w)
        img = R.source(1, 1, hm, wm, seed=5)[0, 0, :, :, 0].double()
        got = R.dense(torch.from_numpy(y_lo_n), y_w, hm) @ img @ R.dense(torch.from_numpy(x_lo_n), x_w, wm).T
        ref = F.interpolate(img[None, None], size=(h, w), mode="bilinear", antialias=True, align_corners=False)[0, 0]
        worst = max(worst, float((got - ref).abs().max()))
        # the plan's fp32 tables are these, rounded
        r = R.restore_plan(pkg, g, 1)
        assert torch.equal(r.y_w, torch.from_numpy(y_w.astype(np.float32))) and torch.equal(r.x_lo_n, torch.from_numpy(x_lo_n))
    print(f"restore tables vs F.interpolate(float64) on the 0..255 scale: max abs difference {worst:.2e}")
    assert worst <= 1e-12


def test_specification_meets_the_bound_at_every_case(pkg, fit):
    lo, hi = 1.0, 0.0
    for g, B, Ts, Td in R.grid():
        c = R.case(pkg, g, B, Ts, Td)
        p = c["rplan"]
        assert tuple(c["ref64"].shape) == (B, Td, p.H, p.W, 3) and (p.H, p.W) == g[1]
        got = fit.restore_frames(c["src"], p, backend="torch")
        assert got.dtype == torch.uint8 and torch.equal(got, c["spec"]) and torch.equal(got, fit.restore_frames(c["src"], p))
        ok, ratio = R.bound_excess(got, c["ref64"], c["e_ref"])
        assert ok and ratio <= 1.0 + 1e-9, (c["name"], ratio)      # one rounding of a value within E_ref: ratio <= 1 by construction
        assert 0 < c["e_ref"] < 1e-3, (c["name"], c["e_ref"])       # (fp32 on the 0..255 scale: a few 1e-5)
        # every disagreement with round(ref64) lies within M * E_ref of a tie
        differ = got != R.round_u8(c["ref64"])
        tie = (c["ref64"] - c["ref64"].floor() - 0.5).abs()
        assert not differ.any() or float(tie[differ].max()) <= R.M_BOUND * c["e_ref"], c["name"]
        ok, _ = R.bound_excess(R.round_u8(c["ref64"]), c["ref64"], c["e_ref"])
        assert ok
        lo, hi = min(lo, c["e_ref"]), max(hi, c["e_ref"])
    print(f"restore specification: E_ref {lo:.2e} .. {hi:.2e} over {len(list(R.grid()))} cases")


@pytest.mark.parametrize("g", R.DYADIC, ids=[R.geometry_id(g) for g in R.DYADIC])
def test_specification_is_bit_exact_where_the_weights_are_dyadic(pkg, fit, g):
    """Dyadic weights make every fp32 operation exact, and ties real: round-half-even of ref64, bit for bit.  The x2 shrink has
    three taps of 3/7, 3/7, 1/7 in its first and last row and column (torch's support is cut at the picture's border and
    renormalised); there a product of an eighth and a seventh can be a tie that fp32 cannot decide, so those outputs are held to
    the bound and every other one to equality.  Round-half-up is told apart by the same inputs."""
    for B in R.BATCHES:
        for Ts, Td in R.TIMES:
            c = R.case(pkg, g, B, Ts, Td)
            mask = R.dyadic_mask(c["rplan"])[None, None, :, :, None].expand_as(c["ref64"])
            whole = bool(mask.all())
            assert whole == (g != R.DYADIC[1]) and float(mask.float().mean()) > 0.8
            want = R.round_u8(c["ref64"])
            got = fit._restore_torch(c["src"], c["rplan"])
            assert torch.equal(got[mask], want[mask]), c["name"]
            assert R.bound_excess(got, c["ref64"], c["e_ref"])[0], c["name"]
            assert whole == (c["e_ref"] == 0)
            if c["rplan"].identity:
                assert torch.equal(got, c["src"][:, :Td])
            else:
                up = R.round_half_up(c)
                assert not torch.equal(up[mask], want[mask]), c["name"]                # real ties: half-up changes bytes here


def test_round_half_up_cannot_miss_the_bound_away_from_dyadic_weights(pkg):
    """Why the dyadic cases exist: at the grid's cases round-half-up stays inside the bound (a tie within E_ref admits both
    neighbours), so only exact ties tell the two roundings apart."""
    for g, B, Ts, Td in R.grid():
        c = R.case(pkg, g, B, Ts, Td)
        assert R.bound_excess(R.round_half_up(c), c["ref64"], c["e_ref"])[0], c["name"]


@pytest.mark.parametrize("name", list(R.wrong_stand_ins()))
def test_wrong_stand_in_misses_the_bound(pkg, name):
    f = R.wrong_stand_ins()[name]
    missed = []
    for g, B, Ts, Td in R.grid():
        if B != 1:
            continue
        c = R.case(pkg, g, B, Ts, Td)
        ok, _ = R.bound_excess(f(c), c["ref64"], c["e_ref"])
        if not ok:
            missed.append(c["name"])
    print(f"{name}: misses the bound at {len(missed)} cases, first {missed[:2]}")
    assert missed, name


def test_flat_frames_come_back_flat(fit):
    clip = R.flat_clip()
    r = fit.plan_restore(fit.plan_fit(256, *R.FLAT[1], "stretch", *R.FLAT[0], windowed=True))
    out = fit.restore_frames(clip, r, backend="torch")
    assert out.shape == (1, 256, 27, 40, 3)
    assert torch.equal(out, torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1, 1).expand_as(out))


def test_restore_frames_errors(fit):
    r = fit.plan_restore(fit.plan_fit(3, 27, 40, "stretch", 16, 32))
    u8 = R.source(1, 9, 16, 32)
    assert fit.restore_frames(u8, r).shape == (1, 3, 27, 40, 3)
    with pytest.raises(ValueError, match="needs a GPU tensor"):
        fit.restore_frames(u8, r, backend="hip")
    with pytest.raises(ValueError, match="unknown backend"):
        fit.restore_frames(u8, r, backend="triton")
    with pytest.raises(ValueError, match=r"uint8 \[B, T, H, W, 3\]"):
        fit.restore_frames(u8.float(), r)
    with pytest.raises(ValueError, match=r"uint8 \[B, T, H, W, 3\]"):
        fit.restore_frames(u8[..., :2], r)
    with pytest.raises(ValueError, match="plan was made for"):
        fit.restore_frames(u8[:, :, :, :16], r)
    with pytest.raises(ValueError, match="plan was made for"):
        fit.restore_frames(u8[:, :2], r)                                       # fewer frames than the plan returns


# ----------------------------------------------------------------------------------------------- nodes
@pytest.mark.parametrize("node", ["Cosmos1InverseRenderer", "Cosmos1ForwardRenderer"])
def test_nodes_declare_fit_restore(pkg, node):
    kind, o = pkg.NODE_CLASS_MAPPINGS[node].INPUT_TYPES()["optional"]["fit_restore"]
    assert kind == "BOOLEAN" and o["default"] is False
    tip = o["tooltip"]
    assert "source size" in tip and "whole picture" in tip and "not renormalised" in tip


class _Recorder:
    """Stands where the pipeline stands: keeps the batch and the restore plan it is handed, and answers with grey frames of the
    size the pipeline would return."""
    device = "cpu"
    batch_passes = False
    restore_plan = "unset"

    def __init__(self):
        self.calls = 0

    def set_model_type(self, t):
        self.model_type = t

    def generate_video(self, data_batch, normalize_normal=False, seed=None):
        self.calls += 1
        self.batch = data_batch
        self.seen_plan = self.restore_plan
        B, _, T, H, W = data_batch["video"].shape
        if self.restore_plan is not None:
            T, H, W = self.restore_plan.T, self.restore_plan.H, self.restore_plan.W
        return np.full((B, T, H, W, 3), 128, dtype=np.uint8)


def _gbuffers(T, H, W):
    return {k: R.source(1, T, H, W, seed=i).float() / 255.0
            for i, k in enumerate(("depth", "normal", "roughness", "metallic", "base_color"))}


def test_inverse_node_sets_and_clears_the_restore_plan(pkg):
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    p = _Recorder()
    image = R.source(1, 10, 40, 36).float() / 255.0
    outs = node.run_inverse_pass(p, image, fit="stretch", fit_restore=True)
    r = p.seen_plan
    assert (r.T, r.H_model, r.W_model, r.H, r.W) == (10, 32, 32, 40, 36) and p.batch["rgb"].shape == (1, 3, 17, 32, 32)
    assert len(outs) == 5 and all(o.shape == (10, 40, 36, 3) for o in outs)
    outs = node.run_inverse_pass(p, image, fit="stretch")                      # restore off: cleared, the model's size
    assert p.seen_plan is None and p.restore_plan is None and all(o.shape == (10, 32, 32, 3) for o in outs)
    node.run_inverse_pass(p, image, fit="stretch", fit_restore=True)
    assert p.restore_plan is not None
    # fit off ignores the flag and hands over today's tensor
    on_grid = R.source(1, 9, 32, 48).float() / 255.0
    node.run_inverse_pass(p, on_grid, fit="off", fit_restore=True)
    assert p.seen_plan is None and torch.equal(p.batch["rgb"], on_grid.permute(0, 4, 1, 2, 3) * 2.0 - 1.0)
    # a crop that cuts, with restore on: refused before the pipeline is called
    calls = p.calls
    with pytest.raises(ValueError, match="crop cannot be undone"):
        node.run_inverse_pass(p, image, fit="crop", fit_restore=True)
    assert p.calls == calls and p.restore_plan is None
    node.run_inverse_pass(p, image, fit="crop")                                # the same crop without restore is today's fit
    assert p.calls == calls + 5 and p.seen_plan is None
    # windows: the plan returns the clip's own frames, none were added
    node.run_inverse_pass(p, R.source(1, 21, 40, 36).float() / 255.0, fit="stretch", fit_restore=True, window_frames=9,
                          window_overlap=2)
    assert p.seen_plan.T == 21 and p.batch["rgb"].shape == (1, 3, 21, 32, 32)


def test_forward_node_sets_and_clears_the_restore_plan(pkg):
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    p = _Recorder()
    g = _gbuffers(10, 40, 36)
    env = torch.rand(1, 16, 32, 3)

    def run(**kw):
        return node.run_forward_pass(p, g["depth"], g["normal"], g["roughness"], g["metallic"], g["base_color"], env, **kw)[0]
    out = run(fit="stretch", fit_restore=True)
    r = p.seen_plan
    assert (r.T, r.H_model, r.W_model, r.H, r.W) == (10, 32, 32, 40, 36) and out.shape == (1, 10, 40, 36, 3)
    out = run(fit="stretch", fit_restore=False)
    assert p.seen_plan is None and p.restore_plan is None and out.shape == (1, 10, 32, 32, 3)
    calls = p.calls
    with pytest.raises(ValueError, match="crop cannot be undone"):
        run(fit="crop", fit_restore=True)
    assert p.calls == calls and p.restore_plan is None
    run(fit="off", fit_restore=True)                                           # fit off ignores the flag: today's tensor
    assert p.seen_plan is None and torch.equal(p.batch["depth"], g["depth"].permute(0, 4, 1, 2, 3) * 2.0 - 1.0)


# ----------------------------------------------------------------------------------------------- pipeline
def test_pipeline_has_no_restore_plan_by_default(pkg, fit):
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline("/nonexistent", "x.pt", model_type=None)
    assert p.restore_plan is None
    u8 = R.source(1, 9, 16, 32)
    assert p._restored(u8) is u8                                               # None: today's path, today's bits
    p.restore_plan = fit.plan_restore(fit.plan_fit(3, 27, 40, "stretch", 16, 32))
    assert torch.equal(p._restored(u8), fit.restore_frames(u8, p.restore_plan)) and p._restored(u8).shape == (1, 3, 27, 40, 3)
    # a window's written frames: restored on their own, as many as were written
    whole = fit.restore_frames(u8, dataclasses.replace(p.restore_plan, T=9))
    assert torch.equal(p._restored(u8[:, 2:7], frames=5), whole[:, 2:7])
