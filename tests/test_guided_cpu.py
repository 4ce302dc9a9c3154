"""The guided way back on the CPU (fit.plan_restore_guided / restore_frames_guided; the references: tests/guided_refs.py):
`axis_taps(reach=1.0)` against today's tables, the plan's rules and errors, the torch specification under its own bound at every
case, flat frames, every wrong stand-in missing the bound at its named case, the quality on a piecewise-constant scene, and the
nodes with recorder pipelines."""
import dataclasses

import numpy as np
import pytest
import torch

import guided_refs as G
import restore_refs as R
from test_relight_cpu import _Pipe, _relight


@pytest.fixture(scope="module")
def fit(pkg):
    return G.fit_module(pkg)


# ----------------------------------------------------------------------------------------------- tables and plan
def _axis_taps_before(n_in, n_full, off, n_out):
    """`fit.axis_taps` as it stood before it took a reach, kept here word for word as the yardstick of `reach=1.0`."""
    scale = n_in / n_full
    support = max(scale, 1.0)
    i = np.arange(off, off + n_out, dtype=np.float64)
    c = scale * (i + 0.5)
    lo = np.maximum(0, (c - support + 0.5).astype(np.int64))
    hi = np.minimum((c + support + 0.5).astype(np.int64), n_in)
    span = int((hi - lo).max())
    j = lo[:, None] + np.arange(span, dtype=np.int64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((j - c[:, None] + 0.5) / support))
    w[j >= hi[:, None]] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    nz = w != 0.0
    first = nz.argmax(axis=1)
    last = span - 1 - nz[:, ::-1].argmax(axis=1)
    n = last - first + 1
    K = int(n.max())
    cols = first[:, None] + np.arange(K)[None, :]
    out = np.where(cols <= last[:, None], np.take_along_axis(w, np.minimum(cols, span - 1), axis=1), 0.0)
    return np.stack([lo + first, n], axis=1).astype(np.int32), out


def test_reach_one_is_todays_tables_bit_for_bit(fit):
    for (hm, wm), (h, w) in R.GEOMETRIES + R.DYADIC + R.EXTRA:
        for n_in, n_out in ((hm, h), (wm, w), (h, hm), (w, wm)):          # the way back and the fit
            want = _axis_taps_before(n_in, n_out, 0, n_out)
            for got in (fit.axis_taps(n_in, n_out, 0, n_out), fit.axis_taps(n_in, n_out, 0, n_out, reach=1.0)):
                assert got[0].dtype == want[0].dtype and np.array_equal(got[0], want[0])
                assert got[1].dtype == np.float64 and got[1].tobytes() == want[1].tobytes()
    lo_n, w = fit.axis_taps(70, 48, 8, 32)                                # a crop's offset
    want = _axis_taps_before(70, 48, 8, 32)
    assert np.array_equal(lo_n, want[0]) and w.tobytes() == want[1].tobytes()


def test_plan_rules(fit):
    plan = fit.plan_fit(10, 1080, 1920, "stretch", 576, 1024)
    g = fit.plan_restore_guided(plan, 12.0)
    assert (g.T, g.H_model, g.W_model, g.H, g.W) == (10, 576, 1024, 1080, 1920)
    assert g.y_w.shape == (1080, 4) and g.x_w.shape == (1920, 4) and g.y_w.dtype == torch.float32       # four taps when up-scaling
    assert g.eps == 2.0 ** -10 and g.sigma == 12.0
    assert torch.allclose(g.y_w.double().sum(dim=1), torch.ones(1080, dtype=torch.float64), atol=1e-6)
    lo, n = g.y_lo_n[:, 0].long(), g.y_lo_n[:, 1].long()
    assert int(lo.min()) == 0 and int((lo + n).max()) == 576 and int(n.min()) >= 1
    # the tables are axis_taps at reach 2.0
    lo_n, w = fit.axis_taps(576, 1080, 0, 1080, reach=2.0)
    assert np.array_equal(lo_n, g.y_lo_n.numpy()) and np.array_equal(w.astype(np.float32), g.y_w.numpy())
    # the range table: float64, rounded once
    d = np.arange(256, dtype=np.float64)
    assert g.tab.dtype == torch.float32 and np.array_equal(g.tab.numpy(), np.exp(-d * d / 288.0).astype(np.float32))
    assert float(g.tab[0]) == 1.0 and float(g.tab[255]) == 0.0
    # shrinking 32 -> 23: six taps
    assert fit.plan_restore_guided(fit.plan_fit(1, 37, 23, "stretch", 32, 32), 12.0).x_w.shape[1] == 6
    # a crop that cut nothing can be brought back, one that cut cannot
    fit.plan_restore_guided(fit.plan_fit(3, 64, 96, "crop", 32, 48), 8.0)
    with pytest.raises(ValueError, match="crop cannot be undone"):
        fit.plan_restore_guided(fit.plan_fit(3, 70, 75, "crop"), 12.0)
    for sigma in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="restore_sigma must be positive"):
            fit.plan_restore_guided(plan, sigma)
    with pytest.raises(ValueError, match="taps per output sample; at most 8"):
        fit.plan_restore_guided(fit.plan_fit(1, 16, 16, "stretch", 48, 48), 12.0)        # a x3 shrink: 12 taps


def test_guide_lo_is_the_fits_own_tables_on_bytes(fit):
    plan = fit.plan_fit(5, 40, 36, "stretch")                                  # pads time to 9: the guide keeps 5 frames
    down = fit.plan_guide_lo(plan)
    assert (down.T, down.H_model, down.W_model, down.H, down.W) == (5, 40, 36, 32, 32) and not down.identity
    assert down.y_lo_n is plan.y_lo_n and down.x_w is plan.x_w
    hi = R.source(2, 5, 40, 36, seed=3)
    lo = fit.restore_frames(hi, down)
    ref64 = R.apply64(hi, R.dense(plan.y_lo_n, plan.y_w, 40), R.dense(plan.x_lo_n, plan.x_w, 36), 5)
    e_ref = float((fit._restore_torch(hi, down, rounded=False).double() - ref64).abs().max())
    assert lo.shape == (2, 5, 32, 32, 3) and 0 < e_ref < 1e-4 and R.bound_excess(lo, ref64, e_ref)[0]      # the restore tests' bound
    assert fit.plan_guide_lo(fit.plan_fit(9, 32, 48, "stretch")).identity
    with pytest.raises(ValueError, match="crop cannot be undone"):
        fit.plan_guide_lo(fit.plan_fit(3, 70, 75, "crop"))
    # source_guide: bytes as they are, floats rounded once
    g8 = fit.source_guide(plan, hi, 12.0, "cpu")
    gf = fit.source_guide(plan, hi.float() / 255.0, 12.0, "cpu")
    assert torch.equal(g8.hi, hi) and torch.equal(gf.hi, hi) and torch.equal(g8.lo, lo) and torch.equal(gf.lo, lo)
    assert g8.plan.T == 5 and g8.plan.x_w.shape[1] == 4
    with pytest.raises(ValueError, match="the plan was made for"):
        fit.source_guide(plan, hi[:, :4], 12.0, "cpu")


# ----------------------------------------------------------------------------------------------- the specification
def test_specification_meets_the_bound_at_every_case(pkg):
    cases = [G.case(pkg, *key) for key in G.grid()] + [f(pkg) for f in G.NAMED.values()]
    assert len(cases) == 6 * 3 * 3 + 2
    for c in cases:
        ok, ratio = G.bound_excess(c["spec"], c["ref64"], c["e_ref"])
        print(f"guided-spec {c['name']}: E_ref {c['e_ref']:.3e}, ratio {ratio:.3f}")
        assert 0 < c["e_ref"] < 5e-4 and ok, c["name"]                         # fp32 on the 0..255 scale: ~1e-4
        assert float((c["spec"].double() - c["ref64"]).abs().max()) <= 0.5 + c["e_ref"]
        assert torch.equal(c["spec"], G.fit_module(pkg).restore_frames_guided(c["src"], c["gplan"], c["hi"], c["lo"], c["t0"]))


def test_the_two_float64_evaluations_agree(pkg):
    for c in (G.case(pkg, G.GEOMETRIES[1], 2, 2, 3, 2, 5, 2), G.sweep_case(pkg), G.fallback_case(pkg)):
        assert float((G.taps64(c) - c["ref64"]).abs().max()) < 1e-9


def test_the_fallback_is_the_spatial_filter_alone(pkg):
    c = G.fallback_case(pkg)
    p = c["gplan"]
    spatial = R.apply64(c["src"], G.dense(p.y_lo_n, p.y_w, p.H_model), G.dense(p.x_lo_n, p.x_w, p.W_model), p.T)
    assert float((spatial - c["ref64"]).abs().max()) < 1e-4                    # (the rows of the fp32 tables sum to 1 +- 1e-7)


def test_flat_frames_come_back_flat(fit, pkg):
    src, gplan, hi, lo = G.flat_case(pkg)
    got = fit.restore_frames_guided(src, gplan, hi, lo)
    assert got.shape == (1, 256, 27, 40, 3)
    assert torch.equal(got, torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1, 1).expand_as(got))


@pytest.mark.parametrize("name", list(G.wrong_stand_ins()))
def test_wrong_stand_in_misses_the_bound(pkg, name):
    where, wrong = G.wrong_stand_ins()[name]
    c = where(pkg)
    assert G.bound_excess(c["spec"], c["ref64"], c["e_ref"])[0]
    ok, ratio = G.bound_excess(wrong(c), c["ref64"], c["e_ref"])
    assert not ok, (name, c["name"], ratio)


def test_guided_beats_the_plain_way_back_on_a_piecewise_constant_scene(fit, pkg):
    """Guide = palette colours +- 3 levels, G-buffer = another palette on the same 7 regions, both through the fit's tables, 32 x 64
    -> 60 x 120, sigma 12: the guided result's mean absolute error against the truth is below half the plain restore's."""
    src, gplan, hi, lo, truth, rplan = G.quality_scene(pkg)
    assert (gplan.H_model, gplan.W_model, gplan.H, gplan.W) == (32, 64, 60, 120) and len(torch.unique(truth.view(-1, 3), dim=0)) == 7
    guided = fit.restore_frames_guided(src, gplan, hi, lo)
    plain = fit.restore_frames(src, rplan)
    mae_g = float((guided.double() - truth.double()).abs().mean())
    mae_p = float((plain.double() - truth.double()).abs().mean())
    print(f"guided-quality: MAE plain {mae_p:.2f}, guided {mae_g:.2f} of 255")
    assert mae_p > 1.0 and mae_g < 0.5 * mae_p


def test_restore_frames_guided_errors(fit, pkg):
    c = G.case(pkg, G.GEOMETRIES[0], 2, 2, 3, 2, 5, 2)
    src, p, hi, lo = c["src"], c["gplan"], c["hi"], c["lo"]
    with pytest.raises(ValueError, match="unknown backend"):
        fit.restore_frames_guided(src, p, hi, lo, 2, backend="cuda")
    with pytest.raises(ValueError, match="needs a GPU tensor"):
        fit.restore_frames_guided(src, p, hi, lo, 2, backend="hip")
    with pytest.raises(ValueError, match="needs uint8"):
        fit.restore_frames_guided(src.float(), p, hi, lo, 2)
    with pytest.raises(ValueError, match="needs uint8"):
        fit.restore_frames_guided(src, p, hi.float(), lo, 2)
    with pytest.raises(ValueError, match="the plan was made for"):
        fit.restore_frames_guided(src[:, :1], p, hi, lo, 2)
    with pytest.raises(ValueError, match="the plan needs guides"):
        fit.restore_frames_guided(src, p, hi, lo[:, :4], 2)
    with pytest.raises(ValueError, match="the plan needs guides"):
        fit.restore_frames_guided(src, p, lo, lo, 2)
    with pytest.raises(ValueError, match="guide clips"):
        fit.restore_frames_guided(torch.cat([src, src[:1]]), p, hi, lo, 2)
    for t0 in (-1, 4):
        with pytest.raises(ValueError, match="outside the guide"):
            fit.restore_frames_guided(src, p, hi, lo, t0)
    assert torch.equal(fit.restore_frames_guided(src, p, hi, lo, 2, backend="torch"), c["spec"])


# ----------------------------------------------------------------------------------------------- pipeline
def test_pipeline_takes_the_guided_route_only_with_a_guide(pkg, fit):
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline("/nonexistent", "x.pt", model_type=None)
    assert p.restore_guide is None
    plan = fit.plan_fit(9, 27, 40, "stretch", 16, 32)
    hi = R.source(1, 9, 27, 40, seed=5)
    guide = fit.source_guide(plan, hi, 12.0, "cpu")
    u8 = R.source(1, 9, 16, 32)
    p.restore_guide = guide
    assert p._restored(u8) is u8                                               # no restore plan: nothing to guide
    p.restore_plan = fit.plan_restore(plan)
    whole = fit.restore_frames_guided(u8, guide.plan, guide.hi, guide.lo)
    assert torch.equal(p._restored(u8), whole) and whole.shape == (1, 9, 27, 40, 3)
    assert not torch.equal(whole, fit.restore_frames(u8, p.restore_plan))
    # a window's written frames read the guide from the window's place in the clip
    assert torch.equal(p._restored(u8[:, 2:7], frames=5, t0=2), whole[:, 2:7])
    assert not torch.equal(p._restored(u8[:, 2:7], frames=5, t0=0), whole[:, 2:7])
    p.restore_guide = None
    assert torch.equal(p._restored(u8), fit.restore_frames(u8, p.restore_plan))       # today's path, today's bits


# ----------------------------------------------------------------------------------------------- nodes
@pytest.mark.parametrize("node", ["Cosmos1InverseRenderer", "Cosmos1Relight"])
def test_nodes_declare_the_guide(pkg, node):
    cls = {**pkg.NODE_CLASS_MAPPINGS, **pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS}[node]
    opt = cls.INPUT_TYPES()["optional"]
    assert opt["restore_guide"][0] == ["off", "source"] and opt["restore_guide"][1]["default"] == "off"
    kind, o = opt["restore_sigma"]
    assert kind == "FLOAT" and (o["default"], o["min"], o["max"]) == (12.0, 1.0, 64.0)
    assert "restore_guide" not in pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"].INPUT_TYPES()["optional"]


class _Recorder:
    """Stands where the pipeline stands: keeps the restore plan and guide it is handed, and answers with grey frames."""
    device = "cpu"
    batch_passes = False
    restore_plan = restore_guide = "unset"

    def set_model_type(self, t):
        self.model_type = t

    def generate_video(self, data_batch, normalize_normal=False, seed=None):
        self.seen_plan, self.seen_guide = self.restore_plan, self.restore_guide
        B, _, T, H, W = data_batch["video"].shape
        if self.restore_plan is not None:
            T, H, W = self.restore_plan.T, self.restore_plan.H, self.restore_plan.W
        return np.full((B, T, H, W, 3), 128, dtype=np.uint8)


def test_inverse_node_hands_over_and_clears_the_guide(pkg, fit):
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    p = _Recorder()
    u8 = R.source(1, 10, 40, 36)
    for image in (u8, u8.float() / 255.0):
        node.run_inverse_pass(p, image, fit="stretch", fit_restore=True, restore_guide="source", restore_sigma=9.0)
        g = p.seen_guide
        assert p.seen_plan is not None and isinstance(g, fit.RestoreGuide)
        want = fit.source_guide(fit.plan_fit(10, 40, 36, "stretch"), u8, 9.0, "cpu")
        assert torch.equal(g.hi, u8) and torch.equal(g.lo, want.lo) and g.lo.shape == (1, 10, 32, 32, 3)
        assert g.plan.sigma == 9.0 and torch.equal(g.plan.tab, want.plan.tab) and g.plan.T == 10
        assert (g.plan.H_model, g.plan.W_model, g.plan.H, g.plan.W) == (32, 32, 40, 36)
    # off, and the cases where the input is ignored: cleared, today's path
    for kw in (dict(fit="stretch", fit_restore=True), dict(fit="stretch", fit_restore=True, restore_guide="off"),
               dict(fit="stretch", restore_guide="source"), dict(fit="crop", restore_guide="source")):
        node.run_inverse_pass(p, u8.float() / 255.0, **kw)
        assert p.seen_guide is None and p.restore_guide is None, kw
    node.run_inverse_pass(p, R.source(1, 9, 32, 48).float() / 255.0, fit="off", fit_restore=True, restore_guide="source")
    assert p.seen_guide is None and p.seen_plan is None
    # windows: the guide keeps the clip's own frames
    node.run_inverse_pass(p, R.source(1, 21, 40, 36), fit="stretch", fit_restore=True, window_frames=9, window_overlap=2,
                          restore_guide="source")
    assert p.seen_guide.hi.shape == (1, 21, 40, 36, 3) and p.seen_guide.plan.T == 21
    with pytest.raises(ValueError, match="restore_guide must be"):
        node.run_inverse_pass(p, u8, fit="stretch", fit_restore=True, restore_guide="image")
    with pytest.raises(ValueError, match="crop cannot be undone"):
        node.run_inverse_pass(p, u8, fit="crop", fit_restore=True, restore_guide="source")
    # the forward node has no such input and never sets a guide
    fwd = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    gb = [R.source(1, 10, 40, 36, seed=i).float() / 255.0 for i in range(5)]
    p.restore_guide = "stale"
    fwd.run_forward_pass(p, *gb, torch.rand(1, 16, 32, 3), fit="stretch", fit_restore=True)
    assert p.seen_guide is None and p.seen_plan is not None


class _GuidedPipe(_Pipe):
    """test_relight_cpu's recorder, with the way back the pipeline takes when it holds a guide."""
    restore_guide = None

    def _frames(self, batch, k):
        guide, plan, self.restore_plan = self.restore_guide, self.restore_plan, None
        try:
            u8 = super()._frames(batch, k)
        finally:
            self.restore_plan = plan
        self.seen_guides = getattr(self, "seen_guides", []) + [guide]
        if plan is None:
            return u8
        T = min(u8.shape[1], plan.T)
        if guide is None:
            return self.fit.restore_frames(u8, dataclasses.replace(plan, T=T))
        return self.fit.restore_frames_guided(u8, dataclasses.replace(guide.plan, T=T), guide.hi, guide.lo)


@pytest.mark.parametrize("as_bytes", (True, False), ids=("uint8", "fp32"))
def test_relight_with_a_guide_is_the_composition_by_hand(pkg, fit, as_bytes):
    T, H, W = 10, 40, 36
    u8 = G.scene(pkg, fit.plan_fit(T, H, W, "stretch", windowed=True), 1, T, seed=7)[0]
    image = u8 if as_bytes else u8.float() / 255.0
    env = torch.rand(1, 16, 32, 3, generator=torch.Generator().manual_seed(5)) * 3.0
    kw = dict(seed=3, env_spin=45.0, fit="stretch")
    p = _GuidedPipe(fit)
    got = _relight(pkg).run_relight(p, p, image, env, fit_restore=True, restore_guide="source", restore_sigma=20.0, **kw)
    assert got[0].shape == (1, T, H, W, 3) and all(o.shape == (T, H, W, 3) for o in got[1:])
    assert p.seen_guides[:5] == [None] * 5 and isinstance(p.seen_guides[5], fit.RestoreGuide)       # the inverse stage stays small
    q = _GuidedPipe(fit)
    small = _relight(pkg).run_relight(q, q, image, env, **kw)                  # everything at the model's size
    assert small[0].shape == (1, T, 32, 32, 3) and q.seen_guides == [None] * 6
    guide = fit.source_guide(fit.plan_fit(T, H, W, "stretch"), u8, 20.0, "cpu")
    plain = _relight(pkg).run_relight(q, q, image, env, fit_restore=True, **kw)
    for a, s, pl in zip(got, small, plain):
        b = (s * 255.0).round().to(torch.uint8).reshape(1, T, 32, 32, 3)
        assert torch.equal(b.float() / 255.0, s.reshape(1, T, 32, 32, 3))
        want = fit.restore_frames_guided(b, guide.plan, guide.hi, guide.lo).float() / 255.0
        assert torch.equal(a.reshape(1, T, H, W, 3), want)
        assert not torch.equal(a, pl)                                          # and it is not the plain way back
    # the G-buffers are what the inverse node returns with the guide
    inv = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]().run_inverse_pass(
        _GuidedPipe(fit), image, seed=3, fit="stretch", fit_restore=True, restore_guide="source", restore_sigma=20.0)
    assert all(torch.equal(a, b) for a, b in zip(got[1:], inv))
    # restore_guide = "off" is today's relight, bit for bit
    off = _relight(pkg).run_relight(q, q, image, env, fit_restore=True, restore_guide="off", restore_sigma=20.0, **kw)
    assert all(torch.equal(a, b) for a, b in zip(off, plain))
