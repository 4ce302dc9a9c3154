"""Seed ensembles on the CPU: the torch specification (ensemble.reduce_members) against the numpy reference of
tests/ensemble_refs.py on the whole case grid, the proof that the grid tells every wrong stand-in from the reference, the
robustness inequality on a synthetic scene, and the orchestration - the pipeline's member loop with a recorder model, the public
generate_video_ensemble, the refusals, and what the nodes set."""
import dataclasses

import numpy as np
import pytest
import torch

import ensemble_refs as R
from stub_vae import StubVAE

BF = torch.bfloat16


def _members(mem):
    return [torch.from_numpy(m).view(-1, 3) for m in mem]


def _flat(t):
    return None if t is None else t.numpy().reshape(-1)


# ----------------------------------------------------------------------------------------------- the reduce
def test_specification_is_the_reference_on_the_whole_grid(pkg):
    E = pkg.ensemble
    ran = 0
    for name, mode, mem in R.cases():
        members = _members(mem)
        for spread in (False, True):
            r, sp = E.reduce_members(members, mode, spread=spread)
            want_r, want_sp = R.reduce_ref(list(mem), mode, spread)
            assert r.dtype == torch.uint8 and r.shape == members[0].shape, name
            assert np.array_equal(_flat(r), want_r), (name, spread)
            assert (sp is None) == (not spread), name
            if spread:
                assert sp.shape == r.shape and np.array_equal(_flat(sp), want_sp), (name, "spread")
        ran += 1
    assert ran == 3 * len(R.SIZES) + 3 * 16 + 2 + 2 * len(R.SET_N) + len(R.SET_N) + 2 + 1 + 6


def test_the_rules_on_values_worked_out_by_hand(pkg):
    E = pkg.ensemble

    def both(cols, mode):
        mem = np.array(cols, dtype=np.uint8).T.copy()                  # [N, n]
        mem = np.ascontiguousarray(np.pad(mem, ((0, 0), (0, (-mem.shape[1]) % 3))))
        r, sp = E.reduce_members(_members(mem), mode, spread=True)
        wr, wsp = R.reduce_ref(list(mem), mode, True)
        assert np.array_equal(_flat(r), wr) and np.array_equal(_flat(sp), wsp)
        return [int(v) for v in wr[:len(cols)]], [int(v) for v in wsp[:len(cols)]]
    # the two middle values averaged, half to even: 1.5 -> 2, 2.5 -> 2, 254.5 -> 254; the deviations by the same rule
    assert both([(1, 2), (2, 3), (254, 255), (0, 255), (7, 7)], "median") == ([2, 2, 254, 128, 7], [0, 0, 0, 128, 0])
    assert both([(9, 1, 5), (0, 0, 255), (255, 0, 255)], "median") == ([5, 0, 255], [4, 0, 0])
    assert both([(1, 3, 2, 200), (10, 10, 11, 11)], "median") == ([2, 10], [1, 0])               # 2.5 -> 2; 10.5 -> 10
    # the mean, half to even: 6 / 4 = 1.5 -> 2, 2 / 4 = 0.5 -> 0, 10 / 4 = 2.5 -> 2, 7 / 3 -> 2, 8 / 3 -> 3
    assert both([(1, 1, 1, 3), (0, 0, 1, 1), (2, 2, 3, 3)], "mean")[0] == [2, 0, 2]
    assert both([(2, 2, 3), (2, 3, 3), (0, 0, 255)], "mean")[0] == [2, 3, 85]
    # N = 1: a copy with spread 0 - but a normal is renormalised
    one = np.array([[200, 128, 128, 0, 255, 7]], dtype=np.uint8)
    for mode in ("median", "mean"):
        r, sp = E.reduce_members(_members(one), mode, spread=True)
        assert np.array_equal(_flat(r), one[0]) and not sp.any()
    r, sp = E.reduce_members(_members(one), "normal", spread=True)
    assert [int(v) for v in _flat(r)] == [255, 128, 128, 53, 202, 57] and [int(v) for v in _flat(sp)] == [110, 110, 110, 0, 0, 0]
    # opposite vectors: the sum is exactly zero -> 128, 128, 128 and the full spread
    opp = np.array([[0, 255, 0], [255, 0, 255]], dtype=np.uint8)
    r, sp = E.reduce_members(_members(opp), "normal", spread=True)
    assert [int(v) for v in _flat(r)] == [128] * 3 and [int(v) for v in _flat(sp)] == [255] * 3


def test_grid_tells_every_wrong_stand_in_from_the_reference():
    assert len(R.WRONG) >= 12
    named = {name: (mode, mem) for name, mode, mem in R.cases(big=False) if name in set(R.WRONG.values())}
    for kind, case in R.WRONG.items():
        mode, mem = named[case]
        want_r, want_sp = R.reduce_ref(list(mem), mode, True)
        got_r, got_sp = R.wrong(kind, list(mem), mode, True)
        n_r, n_sp = int((got_r != want_r).sum()), int((got_sp != want_sp).sum())
        print(f"ensemble stand-in {kind:28s} at {case:18s}: {n_r} result bytes, {n_sp} spread bytes differ")
        assert n_r + n_sp > 0, (kind, case)
    # the stand-ins that only the spread shows are seen there and only there
    mode, mem = named[R.WRONG["spread_wrong_centre"]]
    assert np.array_equal(R.wrong("spread_wrong_centre", list(mem), mode, True)[0], R.reduce_ref(list(mem), mode)[0])


def test_reduce_members_refusals_and_dispatch_on_the_cpu(pkg):
    E = pkg.ensemble
    m = torch.zeros(4, 3, dtype=torch.uint8)
    for kw, match in ((dict(members=[m], mode="mode"), "mode"), (dict(members=[m], mode="median", backend="cuda"), "backend"),
                      (dict(members=[], mode="median"), "members"), (dict(members=[m] * 17, mode="median"), "members"),
                      (dict(members=[m, m.float()], mode="median"), "uint8"), (dict(members=[m, m[:3]], mode="mean"), "one result"),
                      (dict(members=[torch.zeros(4, 4, dtype=torch.uint8)], mode="normal"), "pixels"),
                      (dict(members=[m], mode="median", backend="hip"), "GPU")):
        with pytest.raises(ValueError, match=match):
            E.reduce_members(**kw)
    a, b = torch.full((2, 5, 3), 9, dtype=torch.uint8), torch.full((2, 5, 3), 20, dtype=torch.uint8)
    for backend in ("auto", "torch"):
        r, sp = E.reduce_members([a, b.transpose(0, 1).contiguous().transpose(0, 1)], "mean", spread=True, backend=backend)
        assert r.shape == (2, 5, 3) and int(r[0, 0, 0]) == 14 and int(sp[0, 0, 0]) == 6          # 14.5 -> 14; |9-14|, |20-14| -> 5.5 -> 6


def test_check_ensemble_rules(pkg):
    chk = pkg.ensemble.check_ensemble
    for n in (1, 2, 16):
        chk(n, "median")
        chk(n, "mean")
    chk(1, "median", init_noise=torch.zeros(1))                     # one member with a start noise is today's call
    for bad in (0, 17, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="ensemble"):
            chk(bad, "median")
    for bad in ("normal", "max", None):
        with pytest.raises(ValueError, match="ensemble_reduce"):
            chk(2, bad)
    with pytest.raises(ValueError, match="init_noise"):
        chk(2, "median", init_noise=torch.zeros(1))
    assert pkg.ensemble.member_seed(5, 2) == 7 and pkg.ensemble.member_seed(2 ** 64 - 1, 1) == 0
    assert pkg.ensemble.member_seed(2 ** 64 - 2, 3) == 1


def test_ensemble_is_closer_to_the_truth_than_any_member():
    """Recorded in profiles/ensemble_parity.txt; the condition is the inequality and fixes no number."""
    f = R.robustness_figures(5)
    print("ensemble robustness, N = 5, 20 % salt per member: member MAE " + ", ".join(f"{v:.3f}" for v in f["member_mae"])
          + f"; median {f['median_mae']:.3f}, mean {f['mean_mae']:.3f}")
    print("ensemble robustness, normals: member mean angular error " + ", ".join(f"{v:.3f}" for v in f["member_deg"])
          + f" deg; renormalised sum {f['normal_deg']:.3f} deg")
    assert f["median_mae"] < min(f["member_mae"])
    assert f["normal_deg"] < min(f["member_deg"])


# ----------------------------------------------------------------------------------------------- the pipeline
class _RecorderModel:
    """Stands in for the renderer model: one row per pass, moved by the pass and by the seed, so members and passes differ; keeps
    what every call was handed and what the pipeline's restore settings were at that moment."""
    process_group = None
    net = None

    def __init__(self):
        self.config = {}
        self.vae = StubVAE()
        self.calls, self.seen, self.pipeline, self.fail_at = [], [], None, None

    def to(self, device):
        return self

    def generate_samples_from_batch(self, data_batch, **kw):
        if self.fail_at is not None and len(self.calls) == self.fail_at:
            raise RuntimeError("member failed")
        self.calls.append(kw)
        self.seen.append((self.pipeline.restore_plan, self.pipeline.restore_guide))
        P = data_batch["context_index"].shape[0]
        z = self.vae.encode(data_batch["rgb"]).float()
        move = data_batch["context_index"][:, 0].float().view(P, 1, 1, 1, 1) * 0.07 + ((kw["seed"] * 37) % 11 - 5) * 0.04
        wobble = torch.sin(torch.arange(z.numel(), dtype=torch.float32).view(z.shape) * (1 + kw["seed"] % 5)) * 0.1
        return (z + wobble + move).to(BF)                          # a pass is the same sample alone and in a batch of passes

    def decode(self, sample):
        return self.vae.decode(sample)


@dataclasses.dataclass
class _Plan:
    T: int


@pytest.fixture
def rig(pkg, monkeypatch):
    import window_refs as WR
    mod = pkg.diffusion_renderer_pipeline
    monkeypatch.setattr(mod.N, "postprocess_window_u8",
                        lambda video, prev, ramp, ramp_at, lo, hi, normalize, out=None: WR.blend_postprocess(video, prev, ramp, ramp_at,
                                                                                                              lo, hi, normalize))
    model = _RecorderModel()
    p = mod.CleanDiffusionRendererPipeline("/nonexistent", "x.pt", model_type=None, model_instance=model, guidance=0.0, num_steps=2)
    p.device = torch.device("cpu")
    p.set_model_type("inverse")
    model.pipeline = p
    rgb = pkg.synthetic_weights.synth_tensor("ensemble.pipe.rgb", (1, 3, 17, 48, 64), torch.float32, scale=0.6)
    batch = {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[0], [3]], dtype=torch.long)}
    return mod, p, model, batch


def _by_hand(outs, flags, reduce, spread=False):
    """outs[k][p]: member k's array of pass p -> per pass the reference's reduce."""
    res = []
    for i, flag in enumerate(flags):
        mem = [np.ascontiguousarray(o[i]).reshape(-1) for o in outs]
        r, sp = R.reduce_ref(mem, "normal" if flag else reduce, spread)
        res.append((r.reshape(outs[0][i].shape), None if sp is None else sp.reshape(outs[0][i].shape)))
    return res


def test_ensemble_one_makes_exactly_todays_calls(rig, monkeypatch):
    mod, p, model, batch = rig
    assert p.ensemble == 1 and p.ensemble_reduce == "median"
    base = p.generate_video_passes(batch, [False, True], seed=5)
    calls = [dict(c) for c in model.calls]
    monkeypatch.setattr(mod, "reduce_results", lambda *a, **k: pytest.fail("ensemble = 1 reduces nothing"))
    del model.calls[:]
    p.ensemble, p.ensemble_reduce = 1, "mean"
    again = p.generate_video_passes(batch, [False, True], seed=5)
    assert [set(c) for c in model.calls] == [set(c) for c in calls] and [c["seed"] for c in model.calls] == [5]
    assert set(model.calls[0]) == {"guidance", "state_shape", "num_steps", "is_negative_prompt", "seed", "init_noise"}
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    noise = torch.zeros(2, 16, 3, 6, 8)
    p.generate_video_passes(batch, [False, True], seed=5, init_noise=noise)          # a start noise is fine without an ensemble
    assert model.calls[-1]["init_noise"] is noise


@pytest.mark.parametrize("path", ("whole_clip", "windowed", "pixel_tiled"))
@pytest.mark.parametrize("reduce", ("median", "mean"))
def test_ensemble_is_the_members_in_seed_order_reduced_per_pass(rig, path, reduce):
    mod, p, model, batch = rig
    if path == "windowed":
        p.window_frames, p.window_overlap = 9, 2
    if path == "pixel_tiled":
        p.tile_height, p.tile_width, p.tile_overlap = 32, 32, 8
    flags = [False, True]
    members = [p.generate_video_passes(batch, flags, seed=40 + k) for k in range(3)]
    per_member = len(model.calls) // 3
    del model.calls[:]
    p.ensemble, p.ensemble_reduce = 3, reduce
    got = p.generate_video_passes(batch, flags, seed=40)
    assert [c["seed"] for c in model.calls] == [40] * per_member + [41] * per_member + [42] * per_member, path
    assert all(c["init_noise"] is None for c in model.calls)
    want = _by_hand(members, flags, reduce)
    assert len(got) == 2
    for g, (w, _), m0 in zip(got, want, members[0]):
        assert isinstance(g, np.ndarray) and g.dtype == np.uint8 and g.shape == m0.shape
        assert np.array_equal(g, w), path
    assert not np.array_equal(got[0], members[0][0])                                # the members do differ
    # the three public calls, host and device results
    one = dict(batch, context_index=batch["context_index"][1:2])
    a = p.generate_video(one, normalize_normal=True, seed=40)
    b = p.generate_video_each([dict(batch, context_index=batch["context_index"][0:1]), one], flags, seed=40, to_host=False)
    assert np.array_equal(a, got[1]) and isinstance(b[1], torch.Tensor) and np.array_equal(b[1].numpy(), got[1])
    assert np.array_equal(b[0].numpy(), got[0])
    # the pipeline's own seed where the call names none
    p.seed = 40
    assert np.array_equal(p.generate_video(one, normalize_normal=True), a)


def test_member_seeds_wrap_at_two_to_the_64(rig):
    mod, p, model, batch = rig
    p.ensemble = 3
    p.generate_video_passes(batch, [False, True], seed=2 ** 64 - 1)
    assert [c["seed"] for c in model.calls] == [2 ** 64 - 1, 0, 1]


def test_restore_runs_once_after_the_reduce_and_the_plan_comes_back(rig, monkeypatch):
    mod, p, model, batch = rig
    flags = [False, True]
    members = [p.generate_video_passes(batch, flags, seed=7 + k) for k in range(3)]
    want = _by_hand(members, flags, "median", spread=True)
    plain, guided = [], []

    def restore(u8, plan):
        plain.append((u8.clone(), plan))
        return u8[:, :plan.T, ::2]

    def restore_guided(u8, plan, hi, lo, t0=0):
        guided.append((u8.clone(), plan, hi, lo, t0))
        return u8[:, :plan.T, 1::2]
    monkeypatch.setattr(mod, "restore_frames", restore)
    monkeypatch.setattr(mod, "restore_frames_guided", restore_guided)
    plan = _Plan(T=11)
    p.restore_plan, p.ensemble = plan, 3
    del model.seen[:]
    got = p.generate_video_passes(batch, flags, seed=7)
    assert len(model.seen) == 3 and all(s == (None, None) for s in model.seen)        # the members render without a way back
    assert p.restore_plan is plan and p.restore_guide is None
    assert len(plain) == 2 and not guided                                            # once per result, on the REDUCED result
    for (u8, pl), (w, _), g in zip(plain, want, got):
        assert pl is plan and np.array_equal(u8.numpy(), w) and np.array_equal(g, w[:, :11, ::2])
    # with a guide: the results come back guided, the spreads of generate_video_ensemble by the plain restore
    guide = type("Guide", (), {"plan": _Plan(T=17), "hi": object(), "lo": object()})()
    p.restore_guide = guide
    del plain[:], model.seen[:]
    each = [dict(batch, context_index=batch["context_index"][i:i + 1]) for i in range(2)]
    res, spr = p.generate_video_ensemble(each, flags, seed=7)
    assert all(s == (None, None) for s in model.seen) and p.restore_plan is plan and p.restore_guide is guide
    assert len(guided) == 2 and len(plain) == 2
    for i in range(2):
        assert guided[i][1] == _Plan(T=11) and guided[i][2] is guide.hi and guided[i][4] == 0
        assert np.array_equal(guided[i][0].numpy(), want[i][0]) and np.array_equal(plain[i][0].numpy(), want[i][1])
        assert np.array_equal(res[i], want[i][0][:, :11, 1::2]) and np.array_equal(spr[i], want[i][1][:, :11, ::2])
        assert res[i].shape[:3] == spr[i].shape[:3]
    # a member that raises: the plan and the guide are put back, nothing is restored
    del plain[:], guided[:], model.calls[:]
    model.fail_at = 1
    with pytest.raises(RuntimeError, match="member failed"):
        p.generate_video_passes(batch, flags, seed=7)
    assert p.restore_plan is plan and p.restore_guide is guide and not plain and not guided


def test_generate_video_ensemble_returns_results_and_spreads(rig):
    mod, p, model, batch = rig
    flags = [False, True]
    each = [dict(batch, context_index=batch["context_index"][i:i + 1]) for i in range(2)]
    members = [p.generate_video_each(each, flags, seed=3 + k) for k in range(4)]
    p.ensemble, p.ensemble_reduce = 4, "mean"
    want = _by_hand(members, flags, "mean", spread=True)
    res, spr = p.generate_video_ensemble(each, flags, seed=3)
    assert len(res) == len(spr) == 2
    for i in range(2):
        assert isinstance(res[i], np.ndarray) and res[i].shape == spr[i].shape == (1, 17, 48, 64, 3) and spr[i].dtype == np.uint8
        assert np.array_equal(res[i], want[i][0]) and np.array_equal(spr[i], want[i][1])
    assert spr[0].any() and (spr[1][..., 0] == spr[1][..., 1]).all() and (spr[1][..., 1] == spr[1][..., 2]).all()
    assert np.array_equal(p.generate_video_each(each, flags, seed=3)[0], res[0])          # _render asks for no spread, same result
    dres, dspr = p.generate_video_ensemble(each, flags, seed=3, to_host=False)
    assert isinstance(dres[0], torch.Tensor) and np.array_equal(dspr[1].numpy(), spr[1])
    with pytest.raises(ValueError, match="flags"):
        p.generate_video_ensemble(each, [False], seed=3)
    # one member: the reduce still runs - the plain pass is the member with spread 0, the normal pass is renormalised
    p.ensemble = 1
    res1, spr1 = p.generate_video_ensemble(each, flags, seed=3)
    assert np.array_equal(res1[0], members[0][0]) and not spr1[0].any()
    assert np.array_equal(res1[1], _by_hand(members[:1], flags, "mean")[1][0])


def test_every_refusal_comes_before_any_model_call(rig):
    mod, p, model, batch = rig
    flags = [False, True]
    each = [dict(batch, context_index=batch["context_index"][i:i + 1]) for i in range(2)]
    calls = (lambda **k: p.generate_video(each[0], **k), lambda **k: p.generate_video_passes(batch, flags, **k),
             lambda **k: p.generate_video_each(each, flags, **k))
    for bad in (0, 17, 2.0, "3", True):
        p.ensemble = bad
        for call in calls + (lambda **k: p.generate_video_ensemble(each, flags),):
            with pytest.raises(ValueError, match="ensemble"):
                call()
    p.ensemble, p.ensemble_reduce = 2, "max"
    for call in calls + (lambda **k: p.generate_video_ensemble(each, flags),):
        with pytest.raises(ValueError, match="ensemble_reduce"):
            call()
    p.ensemble_reduce = "median"
    for call in calls:
        with pytest.raises(ValueError, match="init_noise"):
            call(init_noise=torch.zeros(1, 16, 3, 6, 8))
    assert not model.calls


# ----------------------------------------------------------------------------------------------- nodes
class _Recorder:
    """A plain object where the pipeline stands: records what the nodes set and hand over, and every look at its device."""

    def __init__(self):
        self.num_steps = 15
        self.calls, self.touched = [], []

    @property
    def device(self):
        self.touched.append("device")
        return "cpu"

    def set_model_type(self, kind):
        self.touched.append("set_model_type")
        self.kind = kind

    def _out(self, data_batch, to_host):
        ref = data_batch.get("rgb", data_batch.get("depth"))
        B, _, T, H, W = ref.shape
        o = torch.zeros(B, T, H, W, 3, dtype=torch.uint8)
        return o.numpy() if to_host else o

    def generate_video(self, data_batch, normalize_normal=False, seed=None, to_host=True):
        self.calls.append((self.kind, self.ensemble, self.ensemble_reduce))
        return self._out(data_batch, to_host)

    def generate_video_passes(self, data_batch, normalize_normal, seed=None, to_host=True):
        self.calls.append((self.kind, self.ensemble, self.ensemble_reduce))
        return [self._out(data_batch, to_host) for _ in normalize_normal]


def _nodes(pkg):
    return (pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"], pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"],
            pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"])


def test_node_inputs_and_what_the_nodes_set(pkg):
    inv_c, fwd_c, rel_c = _nodes(pkg)
    for cls in (inv_c, rel_c):
        opt = cls.INPUT_TYPES()["optional"]
        kind, o = opt["ensemble"]
        assert kind == "INT" and (o["default"], o["min"], o["max"]) == (1, 1, 16) and "seed + 1" in o["tooltip"]
        assert opt["ensemble_reduce"][0] == ["median", "mean"] and opt["ensemble_reduce"][1]["default"] == "median"
    fopt = fwd_c.INPUT_TYPES()["optional"]
    assert "ensemble" not in fopt and "ensemble_reduce" not in fopt
    assert inv_c.RETURN_TYPES == ("IMAGE",) * 5 and rel_c.RETURN_TYPES == ("IMAGE",) * 6 and fwd_c.RETURN_TYPES == ("IMAGE",)
    assert len(pkg.NODE_CLASS_MAPPINGS) == 4 and pkg.nodes.EXTRA_NODE_DISPLAY_NAME_MAPPINGS == {"Cosmos1Relight": "Cosmos1 Relight"}
    sw = pkg.synthetic_weights
    image = sw.synth_tensor("ensemble.node", (1, 9, 48, 64, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("ensemble.env", (1, 16, 32, 3), torch.float32).abs()
    inv, fwd, rel = inv_c(), fwd_c(), rel_c()
    r = _Recorder()
    inv.run_inverse_pass(r, image)                                               # the defaults: one sample
    inv.run_inverse_pass(r, image, ensemble=3)
    inv.run_inverse_pass(r, image, ensemble=5, ensemble_reduce="mean")
    inv.run_inverse_pass(r, image)                                               # every call sets both
    assert r.calls == [("inverse", 1, "median"), ("inverse", 3, "median"), ("inverse", 5, "mean"), ("inverse", 1, "median")]
    r = _Recorder()
    r.ensemble, r.ensemble_reduce = 4, "mean"                                    # left behind by an inverse run on the same object
    fwd.run_forward_pass(r, *[image] * 5, env)
    assert r.calls == [("forward", 1, "median")]
    r = _Recorder()
    rel.run_relight(r, r, image, env, ensemble=3, ensemble_reduce="mean")
    rel.run_relight(r, r, image, env)
    assert r.calls == [("inverse", 3, "mean"), ("forward", 1, "median"), ("inverse", 1, "median"), ("forward", 1, "median")]


def test_nodes_refuse_before_any_upload(pkg):
    inv_c, fwd_c, rel_c = _nodes(pkg)
    inv, rel = inv_c(), rel_c()
    u8 = torch.zeros(1, 9, 48, 64, 3, dtype=torch.uint8)                          # uint8 frames are uploaded by the ingest
    env = torch.ones(1, 16, 32, 3)
    for kw in ({"ensemble": 0}, {"ensemble": 17}, {"ensemble": 2.5}, {"ensemble": 2, "ensemble_reduce": "max"}):
        r = _Recorder()
        for run in (lambda: inv.run_inverse_pass(r, u8, **kw), lambda: rel.run_relight(r, r, u8, env, **kw)):
            with pytest.raises(ValueError, match="ensemble"):
                run()
        assert not r.calls and not r.touched and not hasattr(r, "ensemble"), kw
    with pytest.raises(TypeError):
        fwd_c().run_forward_pass(_Recorder(), *[u8] * 5, env, ensemble=2)
    r = _Recorder()
    inv.run_inverse_pass(r, u8, ensemble=2)
    assert r.calls == [("inverse", 2, "median")] and "device" in r.touched
