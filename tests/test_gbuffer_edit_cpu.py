"""Relight edits on the CPU: gbuffer_edit.edit_gbuffers (the torch specification) against the independent numpy reference on the
whole case grid, the proof that every wrong stand-in fails its named case, the rule's invariants, every check_edit refusal, and
Cosmos1Relight with recorder pipelines: today's bytes by default, the edit applied by hand otherwise, refusals before any call,
source-size masks and layers through the fit's own tables."""
import numpy as np
import pytest
import torch

import fit_refs as FR
import gbuffer_edit_refs as R
from test_relight_cpu import GBUFFERS, _Pipe

NAMES = ("edit_mask", "edit_base_color_tint", "edit_base_color_gain", "edit_roughness_gain", "edit_metallic_gain",
         "edit_base_color_offset", "edit_roughness_offset", "edit_metallic_offset", "insert_mask", "insert_base_color",
         "insert_metallic", "insert_roughness", "insert_normal", "insert_depth")


@pytest.fixture(scope="module")
def E(pkg):
    return R.edit_module(pkg)


@pytest.fixture(scope="module")
def cases():
    """Every case and its reference result, computed once and left unchanged."""
    built = {name: make() for name, make in R.CASES.items()}
    return {name: (c, R.ref_edit(c)) for name, c in built.items()}


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def to_edit(E, c):
    return E.GBufferEdit(c["gain"], c["offset"], _t(c["edit_mask"]), [_t(l) for l in c["layers"]], _t(c["insert_mask"]))


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_specification_equals_the_reference(E, cases, name):
    c, want = cases[name]
    got = E.edit_gbuffers([_t(m) for m in c["maps"]], to_edit(E, c))
    assert len(got) == 5
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.uint8 and np.array_equal(g.numpy(), w), (name, R.MAPS[k])
    assert any(not np.array_equal(w, m) for w, m in zip(want, c["maps"])), "the case edits nothing"


@pytest.mark.parametrize("wrong", list(R.STAND_INS))
def test_every_wrong_stand_in_fails_its_case(cases, wrong):
    c, want = cases[R.STAND_INS[wrong]]
    got = R.ref_edit(c, wrong=wrong)
    assert any(not np.array_equal(g, w) for g, w in zip(got, want)), f"{wrong} is not seen by {R.STAND_INS[wrong]}"


def test_a_fused_blend_and_a_reciprocal_mask_give_the_rule_s_bytes():
    """What the kernel is free in (and so no stand-in): a fused multiply-add in the blend and the mask read as m * (1 / 255), over
    all 65 536 byte pairs under the 16 mask values of the grid."""
    F = np.float32
    a, b = np.meshgrid(np.arange(256, dtype=F), np.arange(256, dtype=F), indexing="ij")
    for m in R.MASK_VALUES:
        rule = np.rint(a + R.UNIT[m] * (b - a))
        fused = np.rint((a.astype(np.float64) + np.float64(R.UNIT[m]) * (b - a).astype(np.float64)).astype(F))
        recip = np.rint(a + (F(m) * (F(1.0) / F(255.0))) * (b - a))
        assert np.array_equal(rule, fused) and np.array_equal(rule, recip), m


def test_invariants(E):
    c = R.make(30, 2, 3, 4, 6, (2, 3), (2, 3), (2, 3), layers=range(5))
    maps = [_t(m) for m in c["maps"]]
    same = E.edit_gbuffers(maps, E.GBufferEdit())
    assert all(torch.equal(a, b) for a, b in zip(same, maps))                                   # the identity edit
    zero = dict(c, edit_mask=np.zeros_like(c["edit_mask"]), insert_mask=np.zeros_like(c["insert_mask"]))
    got = E.edit_gbuffers(maps, to_edit(E, zero))
    assert all(torch.equal(a, b) for a, b in zip(got, maps))                                    # zero masks, normal map included
    full = dict(c, edit_mask=np.full_like(c["edit_mask"], 255), layers=[None] * 5, insert_mask=None)
    got = E.edit_gbuffers(maps, to_edit(E, full))
    for k in range(5):
        assert np.array_equal(got[k].numpy(), R.ref_affine(c["maps"][k], c["gain"][k], c["offset"][k])), k    # m_e = 255: the affine
    ident = R.make(30, 2, 3, 4, 6, None, (2, 3), (2, 3), layers=range(5), affine=False)
    ident["insert_mask"][...] = 255
    got = E.edit_gbuffers([_t(m) for m in ident["maps"]], to_edit(E, ident))
    for k in range(5):
        L = ident["layers"][k]
        assert np.array_equal(got[k].numpy(), R.ref_normal(L) if k == R.NORMAL else L), k       # m_i = 255: the layer
    assert not np.array_equal(R.ref_normal(ident["layers"][3]), ident["layers"][3])
    with pytest.raises(ValueError, match="needs GPU tensors"):
        E.edit_gbuffers(maps, to_edit(E, c), backend="hip")
    with pytest.raises(ValueError, match="unknown backend"):
        E.edit_gbuffers(maps, to_edit(E, c), backend="triton")
    # float32 masks and layers stand for round(v * 255)
    f = dict(c)
    e = to_edit(E, f)
    e.edit_mask = e.edit_mask.float() / 255.0
    e.layers = [l.float() / 255.0 for l in e.layers]
    want = R.ref_edit(c)
    assert all(np.array_equal(g.numpy(), w) for g, w in zip(E.edit_gbuffers(maps, e), want))


def _refused(E, match, shape=(2, 3, 16, 32), source_hw=None, **kw):
    with pytest.raises(ValueError, match=match):
        E.check_edit(E.GBufferEdit(**kw), shape, source_hw=source_hw)


def test_check_edit_refuses(E):
    u8 = torch.uint8
    m = torch.zeros(2, 3, 16, 32, dtype=u8)
    L = torch.zeros(2, 3, 16, 32, 3, dtype=u8)
    five = lambda l: [l, None, None, None, None]
    rows = lambda k, c, v, base: [[v if (i, j) == (k, c) else base for j in range(3)] for i in range(5)]
    E.check_edit(E.GBufferEdit(rows(0, 1, 8.0, 1.0), rows(2, 0, -255.0, 0.0), m, five(L), m[:1, :1]), (2, 3, 16, 32))      # valid
    _refused(E, "needs insert_mask", layers=five(L))
    _refused(E, "insert_mask without any layer", insert_mask=m)
    for bad in (float("nan"), float("inf")):
        _refused(E, "finite", gain=rows(0, 0, bad, 1.0))
        _refused(E, "finite", offset=rows(4, 2, -bad, 0.0))
    _refused(E, r"gain must lie in \[0, 8\]", gain=rows(1, 0, 8.5, 1.0))
    _refused(E, r"gain must lie in \[0, 8\]", gain=rows(1, 0, -0.01, 1.0))
    _refused(E, r"offset must lie in \[-255, 255\]", offset=rows(2, 1, 255.5, 0.0))
    _refused(E, r"offset must lie in \[-255, 255\]", offset=rows(2, 1, -256.0, 0.0))
    _refused(E, "normal map takes no gain or offset", gain=rows(3, 0, 0.5, 1.0))
    _refused(E, "normal map takes no gain or offset", offset=rows(3, 2, 1.0, 0.0))
    _refused(E, "has 2 frames: 1 .* or the clip's 3", edit_mask=m[:, :2])
    _refused(E, "has 2 frames: 1 .* or the clip's 3", layers=five(L[:, :2]), insert_mask=m)
    _refused(E, "has 2 clips: 1 .* or the batch's 3", shape=(3, 3, 16, 32), insert_mask=m, layers=five(L[:1]))
    _refused(E, "uint8 or float32", edit_mask=m.to(torch.float16))
    _refused(E, "uint8 or float32", insert_mask=m, layers=five(L.to(torch.int32)))
    _refused(E, "neither the model's", edit_mask=m[:, :, :8])
    _refused(E, r"neither the model's \(16, 32\) nor the source's \(20, 40\)", source_hw=(20, 40), edit_mask=m[:, :, :8])
    E.check_edit(E.GBufferEdit(edit_mask=torch.zeros(1, 1, 20, 40)), (2, 3, 16, 32), source_hw=(20, 40))
    _refused(E, r"must be \[B, T, H, W\]", edit_mask=m[0])
    _refused(E, r"must be \[B, T, H, W, 3\]", insert_mask=m, layers=five(L[..., :2]))


# ----------------------------------------------------------------------------------------------- the node
@pytest.fixture(scope="module")
def fit(pkg):
    return FR.fit_module(pkg)


@pytest.fixture(scope="module")
def env():
    return torch.rand(1, 16, 32, 3, generator=torch.Generator().manual_seed(5)) * 3.0


def _relight(pkg):
    return pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()


def _node_case(T, H, W, seed=40):
    """Masks, two layers and the settings of a node call at (T, H, W), with the edit they stand for."""
    g = torch.Generator().manual_seed(seed)
    em = (torch.rand(1, T, H, W, generator=g) * 1.6 - 0.3).clamp(0, 1)
    im = (torch.rand(1, 1, H, W, generator=g) * 1.6 - 0.3).clamp(0, 1)
    base = torch.rand(1, 1, H, W, 3, generator=g)
    nrm = torch.rand(1, T, H, W, 3, generator=g)
    kw = dict(edit_mask=em[0], edit_base_color_tint=0xFF8040, edit_base_color_gain=1.5, edit_roughness_gain=0.0,
              edit_roughness_offset=0.25, edit_metallic_gain=0.5, edit_metallic_offset=-0.1, insert_mask=im[0, 0],
              insert_base_color=base[0], insert_normal=nrm)
    gain = [[255 / 255.0 * 1.5, 128 / 255.0 * 1.5, 64 / 255.0 * 1.5], [0.5] * 3, [0.0] * 3, [1.0] * 3, [1.0] * 3]
    offset = [[0.0] * 3, [-0.1 * 255.0] * 3, [0.25 * 255.0] * 3, [0.0] * 3, [0.0] * 3]
    return kw, gain, offset, em, im, base, nrm


def _bytes(t):
    return (t * 255.0).round().clamp(0, 255).to(torch.uint8).numpy()


def test_the_default_call_is_today_s_call(pkg, fit, env, E):
    T, H, W = 9, 64, 64
    image = FR.source(1, T, H, W, seed=11)
    p, q = _Pipe(fit), _Pipe(fit)
    want = _relight(pkg).run_relight(p, p, image, env, seed=3)
    opt = _relight(pkg).INPUT_TYPES()["optional"]
    defaults = {k: opt[k][1].get("default") for k in NAMES}
    got = _relight(pkg).run_relight(q, q, image, env, seed=3, **defaults)
    assert E.build_edit(pkg.nodes.standardize_to_5d, **defaults) is None                       # no edit object is built
    assert p.ways == q.ways and all(torch.equal(a, b) for a, b in zip(got, want))
    plan = fit.plan_fit(T, H, W, "crop", 0, 0)
    for n, u8 in zip(GBUFFERS, q.inverse_outs):
        assert torch.equal(q.forward_batch[n], fit.fit_frames(u8[:, :T], plan, "cpu")), n      # the forward stage: today's bytes


@pytest.mark.parametrize("batch_passes", (False, True), ids=("pass_by_pass", "batched_passes"))
def test_an_edit_reaches_the_forward_stage_and_comes_back(pkg, fit, env, batch_passes):
    T, H, W = 9, 32, 48
    image = FR.source(1, T, H, W, seed=12)
    kw, gain, offset, em, im, base, nrm = _node_case(T, H, W)
    p = _Pipe(fit, batch_passes)
    got = _relight(pkg).run_relight(p, p, image, env, seed=3, **kw)
    assert p.calls == 6
    case = {"maps": [o[:, :T].numpy() for o in p.inverse_outs], "gain": gain, "offset": offset, "edit_mask": _bytes(em),
            "insert_mask": _bytes(im), "layers": [_bytes(base), None, None, _bytes(nrm), None]}
    want = R.ref_edit(case)
    plan = fit.plan_fit(T, H, W, "crop", 0, 0)
    for k, n in enumerate(GBUFFERS):
        assert not np.array_equal(want[k], case["maps"][k]) or n == "depth"
        assert torch.equal(p.forward_batch[n], fit.fit_frames(_t(want[k]), plan, "cpu")), n    # rendered from the edited maps
        assert torch.equal(got[1 + k], _t(want[k]).float().reshape(T, H, W, 3) / 255.0), n      # and those are what comes back
    assert np.array_equal(want[4], case["maps"][4])                                             # depth was not touched


def test_edit_refusals_come_before_any_call(pkg, fit, env):
    T, H, W = 9, 32, 48
    image = FR.source(1, T, H, W, seed=13)
    m, L = torch.zeros(H, W), torch.zeros(1, H, W, 3)
    bad = [("needs insert_mask", dict(insert_base_color=L)), ("insert_mask without any layer", dict(insert_mask=m)),
           ("finite", dict(edit_roughness_gain=float("nan"))), ("finite", dict(edit_metallic_offset=float("inf"))),
           (r"gain must lie in \[0, 8\]", dict(edit_metallic_gain=9.0)), (r"gain must lie in \[0, 8\]", dict(edit_base_color_gain=-1.0)),
           (r"offset input must lie in \[-1, 1\]", dict(edit_roughness_offset=1.5)), ("display colour", dict(edit_base_color_tint=1 << 24)),
           ("has 4 frames: 1 .* or the clip's 9", dict(edit_mask=torch.zeros(1, 4, H, W))),
           ("has 2 clips: 1 .* or the batch's 1", dict(insert_mask=m, insert_depth=torch.zeros(2, 1, H, W, 3))),
           ("uint8 or float32", dict(edit_mask=m.double())), ("neither the model's", dict(edit_mask=torch.zeros(H, W + 16)))]
    for match, kw in bad:
        a, b = _Pipe(fit), _Pipe(fit)
        with pytest.raises(ValueError, match=match):
            _relight(pkg).run_relight(a, b, image, env, seed=3, **kw)
        assert a.calls == 0 and b.calls == 0, match
    a, b = _Pipe(fit), _Pipe(fit)
    with pytest.raises(ValueError, match=r"neither the model's \(64, 64\) nor the source's \(70, 75\)"):
        _relight(pkg).run_relight(a, b, FR.source(1, 9, 70, 75), env, fit="crop", edit_mask=torch.zeros(32, 32))
    assert a.calls == 0 and b.calls == 0


@pytest.mark.parametrize("mode", ("stretch", "crop"))
def test_source_size_masks_and_layers_go_through_the_fit_s_tables(pkg, fit, env, mode):
    """stretch 40 x 36 -> 32 x 32 (resampled) and a cutting crop 70 x 75 -> 64 x 64 (a pure centre crop: slices by hand)."""
    T, (H, W) = 9, (40, 36) if mode == "stretch" else (70, 75)
    image = FR.source(1, T, H, W, seed=14)
    kw, gain, offset, em, im, base, nrm = _node_case(T, H, W, seed=41)
    p = _Pipe(fit)
    got = _relight(pkg).run_relight(p, p, image, env, seed=3, fit=mode, **kw)
    plan = fit.plan_fit(T, H, W, mode)
    Hm, Wm = plan.H_out, plan.W_out
    assert (Hm, Wm) != (H, W) and (mode == "stretch" or (plan.y0, plan.x0) == (3, 5))

    def by_hand(u8_5d):
        if mode == "crop":
            return u8_5d[:, :, plan.y0:plan.y0 + Hm, plan.x0:plan.x0 + Wm]
        r = fit.RestorePlan(u8_5d.shape[1], H, W, Hm, Wm, plan.y_lo_n, plan.y_w, plan.x_lo_n, plan.x_w, False)
        return fit.restore_frames(u8_5d, r, backend="torch")

    three = lambda m: torch.from_numpy(_bytes(m)).unsqueeze(-1).expand(*m.shape, 3).contiguous()
    case = {"maps": [o[:, :T].numpy() for o in p.inverse_outs], "gain": gain, "offset": offset,
            "edit_mask": by_hand(three(em))[..., 0].numpy(), "insert_mask": by_hand(three(im))[..., 0].numpy(),
            "layers": [by_hand(torch.from_numpy(_bytes(base))).numpy(), None, None, by_hand(torch.from_numpy(_bytes(nrm))).numpy(), None]}
    want = R.ref_edit(case)
    fplan = fit.plan_fit(T, Hm, Wm, "crop", 0, 0)
    for k, n in enumerate(GBUFFERS):
        assert torch.equal(p.forward_batch[n], fit.fit_frames(_t(want[k]), fplan, "cpu")), n
        assert torch.equal(got[1 + k], _t(want[k]).float().reshape(T, Hm, Wm, 3) / 255.0), n
    # the same masks and layers handed in at the model's size are used as they are; a mask may ride as three equal channels
    q = _Pipe(fit)
    kw2 = dict(kw, edit_mask=_t(case["edit_mask"])[0], insert_mask=three(_t(case["insert_mask"]).float() / 255.0)[0],
               insert_base_color=_t(case["layers"][0])[0], insert_normal=_t(case["layers"][3]))
    again = _relight(pkg).run_relight(q, q, image, env, seed=3, fit=mode, **kw2)
    assert all(torch.equal(a, b) for a, b in zip(again, got))


def test_the_node_declares_the_edit_inputs(pkg):
    opt = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"].INPUT_TYPES()["optional"]
    assert tuple(opt)[-len(NAMES):] == NAMES and tuple(opt)[-len(NAMES) - 1] == "ensemble_align"       # appended after the ensemble's
    for k in ("edit_mask", "insert_mask"):
        assert opt[k][0] == "MASK" and "default" not in opt[k][1]
    for k in NAMES[9:]:
        assert opt[k][0] == "IMAGE" and "default" not in opt[k][1]
    assert opt["edit_base_color_tint"][0] == "INT" and opt["edit_base_color_tint"][1]["default"] == 0xFFFFFF
    assert opt["edit_base_color_tint"][1]["display"] == "color"
    for k in ("edit_base_color_gain", "edit_roughness_gain", "edit_metallic_gain"):
        assert opt[k][0] == "FLOAT" and (opt[k][1]["default"], opt[k][1]["min"], opt[k][1]["max"]) == (1.0, 0.0, 8.0)
    for k in ("edit_base_color_offset", "edit_roughness_offset", "edit_metallic_offset"):
        assert opt[k][0] == "FLOAT" and (opt[k][1]["default"], opt[k][1]["min"], opt[k][1]["max"]) == (0.0, -1.0, 1.0)
    import inspect
    sig = inspect.signature(pkg.nodes.Cosmos1Relight.run_relight)
    assert tuple(sig.parameters)[-len(NAMES):] == NAMES
    assert [sig.parameters[k].default for k in NAMES] == [None, 0xFFFFFF, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0] + [None] * 6
    assert len(pkg.nodes.NODE_CLASS_MAPPINGS) + len(pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS) == 5
