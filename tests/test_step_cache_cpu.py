"""The step cache without a GPU (step_cache.py): the numpy reference of tests/step_cache_refs.py against the module's
specification and against math.fsum, wrong stand-ins that each fail a named case, the controller on scripted probe answers and
over a torch three-stage stub, the model's two loops with a recorder net, the pipeline with a recorder model, and the nodes."""
import logging
import math
import os
import re

import numpy as np
import pytest
import torch

import step_cache_refs as R
from conftest import ROOT
from stub_vae import StubVAE

BF = torch.bfloat16


def to_t(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(BF)


def to_bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


# ----------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("n", R.SIZES + (5 * 8192 + 77, 70 * 8192 + 3))
def test_probe_reference_orders_agree_and_bound_fsum(pkg, n):
    """The lane-by-lane loop, its vectorised form and the module's specification give the same bits; and the ordered fp64 sum of
    n non-negative terms lies within n * 2^-53 (relative) of the exact sum: every partial sum is at most the exact total, so each
    of the at most n - 1 roundings errs by at most 2^-53 of it."""
    B = 2
    rb = R.rand_bits(f"cpu.ref.{n}", (B, n), 1.5)
    xb = R.bf16_bits(R.f32(rb) + R.f32(R.rand_bits(f"cpu.d.{n}", (B, n), 0.05)))
    fast = R.probe_ref(xb, rb, fast=True)
    if n <= 5 * 8192 + 77:
        assert np.array_equal(R.probe_ref(xb, rb, fast=False).view(np.uint64), fast.view(np.uint64))
    spec = pkg.step_cache.probe_reference(to_t(xb), to_t(rb))
    assert spec.dtype == np.float64 and np.array_equal(spec.view(np.uint64), fast.view(np.uint64))
    num, den = R.terms(xb, rb)
    for b in range(B):
        for got, t in ((fast[b, 0], num[b]), (fast[b, 1], den[b])):
            exact = math.fsum(t.tolist())
            assert abs(got - exact) <= n * 2.0 ** -53 * exact
    assert pkg.step_cache.delta_from_stats(spec.tolist()) == R.delta_ref(fast)


def test_residual_and_apply_reference_is_torch(pkg):
    xs = R.all_finite_bf16()
    partners = np.array([0x0000, 0x8000, 0x3F80, 0xBF80, 0x0001, 0x7F7F, 0xFF7F, 0x3C00, 0x7F80, 0xFF80, 0x7FC0], dtype=np.uint16)
    ab, bb = np.repeat(xs, partners.size), np.tile(partners, xs.size)
    ta, tb = to_t(ab), to_t(bb)
    SC = pkg.step_cache
    assert R.same_as_torch(R.residual_ref(ab, bb), to_bits(SC.residual_reference(ta, tb)))
    assert R.same_as_torch(R.apply_ref(ab, bb), to_bits(SC.apply_reference(ta, tb)))
    assert R.same_as_torch(R.residual_ref(ab, bb), to_bits((ta.float() - tb.float()).bfloat16()))
    assert R.is_nan(R.residual_ref(ab, bb)).sum() == 65280 and not R.same_as_torch(R.apply_ref(ab, bb), to_bits(ta))
    sp = np.array([0x7F80, 0xFF80, 0x7FC0], dtype=np.uint16)
    assert R.residual_ref(sp, sp).tolist() == [0x7FC0, 0x7FC0, 0x7FC0] and R.apply_ref(sp[:2], sp[:2]).tolist() == [0x7F80, 0xFF80]


def test_case_grid_reaches_what_the_kernels_branch_on():
    cases = R.probe_cases()
    assert {n for _, _, n, *_ in cases} >= set(R.SIZES) and {B for _, B, *_ in cases} == {1, 2, 3}
    for off in range(1, 8):
        assert any(c[3] == off and c[4] == 0 for c in cases) and any(c[3] == 0 and c[4] == off for c in cases)
        assert any(c[3] == off and c[4] == off and c[5] == off for c in cases)
    # past one sweep of the 2048 blocks, on both address paths
    assert any(B * -(-n // 8192) > 2048 and n % 8 for _, B, n, *_ in cases)
    assert any(B * -(-n // 8192) > 2048 and n % 8 == 0 for _, B, n, *_ in cases)
    assert any(n > 2048 * 256 * 8 and n % 8 for n in R.EW_SIZES) and any(2048 * 256 < n < 2048 * 256 * 8 for n in R.EW_SIZES)
    text = open(os.path.join(ROOT, "diffusionrenderer-comfyui_amd", "csrc", "step_cache.hip")).read()
    assert re.search(r"SC_CHUNK = 8192;", text) and re.search(r"SC_MAX_BLOCKS = 2048;", text) and re.search(r"SC_THREADS = 256;", text)


def _one(value, n=16):
    return R.bf16_bits(np.full((1, n), value, dtype=np.float32))


def test_wrong_probes_each_fail_a_named_case():
    same = lambda a, b: np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))
    # den from x: x = 2 ref
    x, ref = _one(2.0), _one(1.0)
    assert R.probe_ref(x, ref).tolist() == [[16.0, 16.0]] and R.probe_ref(x, ref, "den_from_x").tolist() == [[16.0, 32.0]]
    # a signed difference: a stream that moved up and down by the same amount has not stood still
    x = R.bf16_bits(np.array([[2.0, 0.0] * 8], dtype=np.float32))
    assert R.probe_ref(x, ref)[0, 0] == 16.0 and R.probe_ref(x, ref, "signed")[0, 0] == 0.0
    # one sum over the whole batch: a small clip that moved far hides behind a large clip that stood still
    xb = np.concatenate([_one(100.0), _one(0.03)])
    rb = np.concatenate([_one(100.0), _one(0.01)])
    assert R.delta_ref(R.probe_ref(xb, rb)) > 1.9 and R.delta_ref(R.probe_ref(xb, rb, "whole_batch")) < 1e-3
    # a fused or fp64 subtract: 1 - 2^-30 is 1 in fp32
    x, ref = _one(1.0), _one(2.0 ** -30)
    assert R.probe_ref(x, ref)[0, 0] == 16.0 and not same(R.probe_ref(x, ref), R.probe_ref(x, ref, "fp64_subtract"))
    # a chunk of the neighbouring clip: clip 0's ragged last chunk must stop at its own end
    n = 8193
    rb = R.rand_bits("wrong.ref", (2, n), 1.0)
    xb = rb.copy()
    xb[1] = R.bf16_bits(R.f32(rb[1]) * np.float32(1.5))
    good, bad = R.probe_ref(xb, rb), R.probe_ref(xb, rb, "neighbour_chunk")
    assert good[0, 0] == 0.0 and bad[0, 0] > 0.0 and same(good[1], bad[1])


# ----------------------------------------------------------------------------------------------- a three-stage stub
def _stages():
    """head, tail, final on bf16 bits [B, n] (numpy) - deterministic, each rounding to bf16 once."""
    head = lambda b: R.bf16_bits(R.f32(b) * np.float32(0.75) + np.roll(R.f32(b), 1, axis=1) * np.float32(0.25))
    tail = lambda b: R.bf16_bits(R.f32(b) + np.tanh(R.f32(b) * np.float32(1.7)) * np.float32(0.5))
    final = lambda b: R.bf16_bits(R.f32(b) * np.float32(1.25) - np.float32(0.125))
    return head, tail, final


def _torch_stages():
    head, tail, final = _stages()
    wrap = lambda f: (lambda t: to_t(f(to_bits(t))))
    return wrap(head), wrap(tail), wrap(final)


def _inputs(n_steps, B=2, n=8192 + 24, drift=0.02):
    base = R.f32(R.rand_bits("stub.inputs", (B, n), 1.0))
    wobble = R.f32(R.rand_bits("stub.wobble", (B, n), 1.0))
    return [R.bf16_bits(base * np.float32(1.0 + drift * i) + wobble * np.float32(drift * i)) for i in range(n_steps)]


@pytest.mark.parametrize("thr,max_run", [(1e-30, 3), (0.05, 3), (0.5, 2), (1.0, 1)])
def test_controller_over_a_stub_is_the_composition_by_hand(pkg, thr, max_run):
    SC = pkg.step_cache
    inputs = _inputs(7)
    want, want_log = R.hand_loop(inputs, thr, max_run, *_stages())
    c = SC.Controller(thr, max_run, len(inputs), *_torch_stages(), SC.TorchBackend())
    got = [to_bits(c.step(to_t(i))) for i in inputs]
    assert c.log == want_log
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    plain = [_stages()[2](_stages()[1](_stages()[0](i))) for i in inputs]
    computed = [k for k, (cpt, _) in enumerate(c.log) if cpt]
    assert all(np.array_equal(got[k], plain[k]) for k in computed)
    if thr == 1e-30:
        assert computed == list(range(7))
    if thr >= 0.5:
        assert len(computed) < 7 and any(not np.array_equal(got[k], plain[k]) for k in range(7) if k not in computed)
    assert c.end() is c.log and c.ref is None and c.R is None


def test_wrong_rules_each_fail_a_named_case():
    inputs = _inputs(7, drift=0.03)
    stages = _stages()
    want, want_log = R.hand_loop(inputs, 0.5, 3, *stages)
    assert [c for c, _ in want_log] == [True, False, False, False, True, False, True]

    def differs(variant, thr=0.5):
        got, log = R.hand_loop(inputs, thr, 3, *stages, variant=variant)
        ref, ref_log = R.hand_loop(inputs, thr, 3, *stages)
        return log != ref_log or any(not np.array_equal(g, w) for g, w in zip(got, ref))
    # against the previous step's X1 the drift never adds up: the logged deltas stay at one step's worth
    assert differs("prev_x1")
    _, log = R.hand_loop(inputs, 0.5, 3, *stages, variant="prev_x1")
    assert log[3][1] < want_log[3][1] / 2
    for variant in ("refresh_ref", "refresh_R", "R_before_head", "den_from_x", "whole_batch"):
        assert differs(variant), variant
    # a threshold between the worst clip's delta and the pooled one: the pooled probe skips where the rule computes
    d_worst = want_log[1][1]
    _, pooled = R.hand_loop(inputs, 0.5, 3, *stages, variant="whole_batch")
    assert pooled[1][1] != d_worst


# ----------------------------------------------------------------------------------------------- scripted deltas
class _Scripted:
    """A backend whose probe answers from a script; the tensors are step numbers."""

    def __init__(self, script):
        self.script, self.asked = list(script), []

    def copy(self, x, into=None):
        return ("ref", x)

    def probe(self, x, ref):
        self.asked.append((x, ref))
        return self.script[x]

    def residual(self, x, ref, into=None):
        return ("R", x, ref)

    def apply(self, x, r):
        return ("applied", x, r)


def _scripted(pkg, script, thr, max_run, n=None):
    be = _Scripted(script)
    n = len(script) if n is None else n
    c = pkg.step_cache.Controller(thr, max_run, n, head=lambda i: i, tail=lambda x: ("tail", x), final=lambda x: x, backend=be)
    return [c.step(i) for i in range(len(script))], c, be


def test_controller_on_scripted_deltas(pkg):
    one = lambda d: [(d, 1.0)]
    # first and last forced, however small the deltas; max_run = 3 forces a computed step after three skipped
    outs, c, be = _scripted(pkg, [one(0.0)] * 8, 0.1, 3)
    assert [cpt for cpt, _ in c.log] == [True, False, False, False, True, False, False, True]
    assert [d for _, d in c.log] == [None, 0.0, 0.0, 0.0, None, 0.0, 0.0, None]
    assert [x for x, _ in be.asked] == [1, 2, 3, 5, 6]                       # a forced step does not ask (and does not synchronise)
    # ref and R are those of the last COMPUTED step: skipped steps do not refresh them
    assert [r for _, r in be.asked] == [("ref", 0)] * 3 + [("ref", 4)] * 2
    assert outs[0] == ("tail", 0) and outs[2] == ("applied", 2, ("R", ("tail", 0), ("ref", 0)))
    assert outs[6] == ("applied", 6, ("R", ("tail", 4), ("ref", 4)))
    outs, c, _ = _scripted(pkg, [one(0.0)] * 5, 0.1, 1)
    assert [cpt for cpt, _ in c.log] == [True, False, True, False, True]
    # thr just above / below a delta: skip iff delta < thr
    d = 0.1
    for thr, skipped in ((np.nextafter(d, 1.0), True), (d, False), (np.nextafter(d, 0.0), False)):
        _, c, _ = _scripted(pkg, [one(d)] * 3, float(thr), 3)
        assert c.log[1] == (not skipped, d)
    # den = 0, NaN and inf compute; the worst clip decides
    for stats in ([(0.0, 0.0)], [(1.0, 0.0)], [(float("nan"), 1.0)], [(1.0, float("nan"))], [(float("inf"), 1.0)], [(1.0, float("inf"))],
                  [(0.0, 1.0), (0.0, 0.0)], [(1e300, 1e-300)]):
        _, c, _ = _scripted(pkg, [stats] * 3, 1.0, 3)
        assert c.log[1] == (True, math.inf), stats
    _, c, _ = _scripted(pkg, [[(0.01, 1.0), (0.3, 1.0), (0.02, 1.0)]] * 3, 0.2, 3)
    assert c.log[1] == (True, 0.3)
    _, c, _ = _scripted(pkg, [[(0.01, 1.0), (0.3, 2.0), (0.02, 1.0)]] * 3, 0.2, 3)
    assert c.log[1] == (False, 0.15)
    # one step and two steps: everything is forced; a step past the announced count is computed
    for n in (1, 2):
        _, c, be = _scripted(pkg, [one(0.0)] * n, 0.5, 3)
        assert [cpt for cpt, _ in c.log] == [True] * n and not be.asked
    _, c, _ = _scripted(pkg, [one(0.0)] * 4, 0.5, 3, n=2)
    assert [cpt for cpt, _ in c.log] == [True] * 4


def test_controller_refusals_and_log_line(pkg, caplog):
    SC = pkg.step_cache
    ok = dict(head=None, tail=None, final=None, backend=None)
    for thr, run, n in ((0.0, 3, 4), (-1.0, 3, 4), (1.5, 3, 4), (float("nan"), 3, 4), (float("inf"), 3, 4), (True, 3, 4), ("0.1", 3, 4),
                        (0.1, 0, 4), (0.1, 2.5, 4), (0.1, True, 4), (0.1, 3, 0), (0.1, 3, 2.0)):
        with pytest.raises(ValueError):
            SC.Controller(thr, run, n, **ok)
    SC.check_step_cache(0.0)
    SC.check_step_cache(1.0, 1)
    SC.check_step_cache(0.0, tile_join="latent")
    SC.check_step_cache(np.float32(0.25), np.int64(2))
    with pytest.raises(ValueError, match="latent"):
        SC.check_step_cache(0.1, tile_join="latent")
    _, c, _ = _scripted(pkg, [[(0.0, 1.0)]] * 6, 0.1, 3)
    with caplog.at_level(logging.INFO, logger=SC.__name__):
        c.end()
    lines = [r.getMessage() for r in caplog.records if r.name == SC.__name__]
    assert len(lines) == 1 and "computed 3 of 6" in lines[0]


# ----------------------------------------------------------------------------------------------- the model's loops
class _RecorderNet:
    """Stands in for the DiT: records the cache calls around its forwards; optionally raises at a step."""

    def __init__(self, log, fail_at=None):
        self.log, self.fail_at, self.calls = log, fail_at, 0
        self.step_cache_log = []

    def prepare_timesteps(self, ts):
        pass

    def cache_begin(self, thr, max_run, n_steps):
        self.log.append(("cache_begin", thr, max_run, n_steps))

    def cache_end(self):
        self.log.append(("cache_end",))

    def __call__(self, x, timesteps, latent_condition, context_index):
        if self.calls == self.fail_at:
            raise RuntimeError("the net failed")
        self.calls += 1
        self.log.append(("net", tuple(x.shape), float(timesteps)))
        return (x.float() * 0.5 / (1.0 + float(timesteps))).to(BF)


def _cpu_model(pkg, monkeypatch, log, fail_at=None):
    mod = pkg.model_diffusion_renderer
    monkeypatch.setattr(mod.N, "edm_scale_input", lambda x, c_in: (log.append(("edm_scale_input",)), (x.float() * c_in).to(BF))[1])
    monkeypatch.setattr(mod.N, "cfg_combine", lambda c, u, g: (log.append(("cfg_combine",)), (c.float() + (c.float() - u.float()) * g).to(BF))[1])
    monkeypatch.setattr(mod.N, "edm_step", lambda mo, x, *k: (log.append(("edm_step",)), (x.float() * 0.9 + mo.float() * 0.1).to(BF))[1])
    cfgd = pkg.diffusion_renderer_config.get_inverse_renderer_config()
    cfgd["model_type"] = "inverse"
    m = mod.CleanDiffusionRendererModel(cfgd, device="cpu")
    m.net, m.vae = _RecorderNet(log, fail_at), StubVAE()
    return m


def _batch(pkg):
    rgb = pkg.synthetic_weights.synth_tensor("sc.cpu.rgb", (1, 3, 9, 32, 32), torch.float32, scale=0.6).to(BF)
    return {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[0], [3]], dtype=torch.long)}


@pytest.mark.parametrize("sampler", ("euler", "dpmpp_2m"))
@pytest.mark.parametrize("guidance", (0.0, 1.5))
def test_model_loops_wrap_their_steps_in_one_begin_and_end(pkg, monkeypatch, sampler, guidance):
    log = []
    m = _cpu_model(pkg, monkeypatch, log)
    noise = pkg.synthetic_weights.synth_tensor("sc.cpu.xT", (1, 16, 2, 4, 4), torch.float32, scale=80.0)
    kw = dict(guidance=guidance, seed=3, state_shape=[16, 2, 4, 4], num_steps=4, init_noise=noise, sampler=sampler)
    plain = m.generate_samples_from_batch(_batch(pkg), **kw)
    base = list(log)
    assert not any(e[0].startswith("cache") for e in base) and sum(e[0] == "net" for e in base) == 4
    if sampler == "euler":                                # Euler's calls as they were
        per_step = ["edm_scale_input", "net"] + (["cfg_combine"] if guidance > 0 else []) + ["edm_step"]
        assert [e[0] for e in base] == per_step * 4
    del log[:]
    assert torch.equal(m.generate_samples_from_batch(_batch(pkg), step_cache=0.0, step_cache_max_run=2, **kw), plain)
    assert log == base                                    # no call at all at step_cache = 0
    del log[:]
    assert torch.equal(m.generate_samples_from_batch(_batch(pkg), step_cache=0.25, step_cache_max_run=2, **kw), plain)
    nets = [i for i, e in enumerate(log) if e[0] == "net"]
    begins = [i for i, e in enumerate(log) if e[0] == "cache_begin"]
    ends = [i for i, e in enumerate(log) if e[0] == "cache_end"]
    assert len(begins) == len(ends) == 1 and log[begins[0]] == ("cache_begin", 0.25, 2, 4)
    assert begins[0] < nets[0] and nets[-1] < ends[0] and [e for e in log if not e[0].startswith("cache")] == base
    del log[:]
    m.generate_samples_from_batch(_batch(pkg), step_cache=0.25, **kw)
    assert [e for e in log if e[0] == "cache_begin"] == [("cache_begin", 0.25, 3, 4)]


@pytest.mark.parametrize("sampler", ("euler", "dpmpp_2m"))
def test_cache_end_is_called_when_the_net_raises(pkg, monkeypatch, sampler):
    log = []
    m = _cpu_model(pkg, monkeypatch, log, fail_at=2)
    with pytest.raises(RuntimeError, match="the net failed"):
        m.generate_samples_from_batch(_batch(pkg), state_shape=[16, 2, 4, 4], num_steps=4, sampler=sampler, step_cache=0.5)
    assert [e[0] for e in log if e[0].startswith("cache")] == ["cache_begin", "cache_end"] and log[-1] == ("cache_end",)


def test_model_refusals(pkg, monkeypatch):
    log = []
    m = _cpu_model(pkg, monkeypatch, log)
    for bad in ({"step_cache": -0.1}, {"step_cache": 1.01}, {"step_cache": float("nan")}, {"step_cache": 0.1, "step_cache_max_run": 0}):
        with pytest.raises(ValueError, match="step_cache"):
            m.generate_samples_from_batch(_batch(pkg), state_shape=[16, 2, 4, 4], num_steps=2, **bad)
    tiles = pkg.tiles
    rgb = torch.zeros(1, 3, 9, 48, 64, dtype=BF)
    plan = tiles.plan_tiles(48, 64, 32, 32, 8)
    lat = [tiles.latent_tile(t, 8) for t in plan]
    batches = [{"rgb": rgb[..., t.y:t.y + t.h, t.x:t.x + t.w].contiguous(), "context_index": torch.tensor([[3]])} for t in plan]
    with pytest.raises(ValueError, match="latent"):
        m.generate_samples_joint(batches, lat, (16, 2, 6, 8), num_steps=2, step_cache=0.1)
    assert not log


# ----------------------------------------------------------------------------------------------- the pipeline
class _RecorderModel:
    process_group = None

    def __init__(self):
        self.config = {}
        self.vae = StubVAE()
        self.calls = []
        self.net = type("Net", (), {"step_cache_log": []})()

    def to(self, device):
        return self

    def generate_samples_from_batch(self, data_batch, **kw):
        self.calls.append(kw)
        self.net.step_cache_log = [(True, None), (False, 0.01 * len(self.calls)), (True, None)]
        return self.vae.encode(data_batch["rgb"]).to(BF)

    def decode(self, sample):
        return self.vae.decode(sample)


def _cpu_pipeline(pkg, monkeypatch):
    import window_refs as WR
    mod = pkg.diffusion_renderer_pipeline
    monkeypatch.setattr(mod.N, "postprocess_window_u8",
                        lambda video, prev, ramp, ramp_at, lo, hi, normalize, out=None: WR.blend_postprocess(video, prev, ramp, ramp_at,
                                                                                                              lo, hi, normalize))
    monkeypatch.setattr(mod, "reduce_results", lambda members, flags, reduce, spread=False: (members[0], None))
    model = _RecorderModel()
    p = mod.CleanDiffusionRendererPipeline("/nonexistent", "x.pt", model_type=None, model_instance=model, guidance=0.0, num_steps=3)
    p.device = torch.device("cpu")
    p.set_model_type("inverse")
    return p, model


def test_pipeline_hands_the_cache_on_every_path_and_nothing_when_off(pkg, monkeypatch):
    p, model = _cpu_pipeline(pkg, monkeypatch)
    assert p.step_cache == 0.0 and p.step_cache_max_run == 3 and p.last_step_cache == []
    rgb = pkg.synthetic_weights.synth_tensor("sc.pipe.rgb", (1, 3, 17, 48, 64), torch.float32, scale=0.6)
    batch = {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[3]], dtype=torch.long)}
    plain_keys = {"guidance", "state_shape", "num_steps", "is_negative_prompt", "seed", "init_noise"}
    paths = {"whole clip": ({}, 1), "windows": ({"window_frames": 9, "window_overlap": 2}, None),
             "pixel tiles": ({"tile_height": 32, "tile_width": 32, "tile_overlap": 8}, None), "ensemble": ({"ensemble": 2}, 2)}
    for name, (settings, loops) in paths.items():
        for k, v in settings.items():
            setattr(p, k, v)
        for thr in (0.0, 0.25):
            p.step_cache, p.step_cache_max_run = thr, 2
            del model.calls[:]
            p.generate_video(batch, seed=5)
            assert model.calls, name
            for kw in model.calls:
                assert set(kw) == (plain_keys | {"step_cache", "step_cache_max_run"} if thr else plain_keys), (name, thr)
                if thr:
                    assert (kw["step_cache"], kw["step_cache_max_run"]) == (0.25, 2)
            # one log per sample loop: windows, tiles and ensemble members each begin their own
            assert len(p.last_step_cache) == (len(model.calls) if thr else 0)
            if thr:
                assert len(model.calls) == loops if loops else len(model.calls) > 1
                assert [log[1][1] for log in p.last_step_cache] == [0.01 * (i + 1) for i in range(len(model.calls))]
        for k in settings:
            setattr(p, k, 1 if k == "ensemble" else 0)
    p.step_cache = 0.0


def test_pipeline_refuses_before_any_gpu_work(pkg, monkeypatch):
    p, model = _cpu_pipeline(pkg, monkeypatch)
    rgb = torch.zeros(1, 3, 9, 48, 64)
    batch = {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[3]], dtype=torch.long)}
    for thr, run in ((-0.01, 3), (1.5, 3), (float("nan"), 3), (float("inf"), 3), (0.1, 0), (0.1, -2)):
        p.step_cache, p.step_cache_max_run = thr, run
        with pytest.raises(ValueError, match="step_cache"):
            p.generate_video(batch)
    p.step_cache, p.step_cache_max_run, p.tile_join = 0.1, 3, "latent"
    p.tile_height, p.tile_width, p.tile_overlap = 32, 32, 8
    with pytest.raises(ValueError, match="latent"):
        p.generate_video(batch)
    with pytest.raises(ValueError, match="latent"):
        p.generate_video_ensemble([batch], [False])
    assert not model.calls


# ----------------------------------------------------------------------------------------------- the nodes
class _Recorder:
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
        self.calls.append((self.kind, self.step_cache))
        return self._out(data_batch, to_host)

    def generate_video_passes(self, data_batch, normalize_normal, seed=None, to_host=True):
        self.calls.append((self.kind, self.step_cache))
        return [self._out(data_batch, to_host) for _ in normalize_normal]


def _node_classes(pkg):
    return [pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"], pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"],
            pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]]


def test_node_inputs_and_what_the_nodes_set(pkg):
    classes = _node_classes(pkg)
    returns = [("IMAGE",) * 5, ("IMAGE",), ("IMAGE",) * 6]
    for cls, ret in zip(classes, returns):
        opt = cls.INPUT_TYPES()["optional"]
        kind, o = opt["step_cache"]
        assert kind == "FLOAT" and {k: o[k] for k in ("default", "min", "max", "step")} == {"default": 0.0, "min": 0.0, "max": 1.0, "step": 0.01}
        assert "first-block" in o["tooltip"] and "0 = off" in o["tooltip"]
        keys = list(opt)
        assert keys.index("step_cache") == keys.index("steps") + 1 == keys.index("sampler") + 2
        assert cls.RETURN_TYPES == ret                    # node return types stay pinned
    sw = pkg.synthetic_weights
    image = sw.synth_tensor("sc.node", (1, 9, 48, 64, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("sc.env", (1, 16, 32, 3), torch.float32).abs()
    inv, fwd, rel = (c() for c in classes)
    r = _Recorder()
    inv.run_inverse_pass(r, image)
    inv.run_inverse_pass(r, image, step_cache=0.25)
    inv.run_inverse_pass(r, image)                        # every call sets it: the default switches it off again
    assert r.calls == [("inverse", 0.0), ("inverse", 0.25), ("inverse", 0.0)]
    r = _Recorder()
    g = [image] * 5
    fwd.run_forward_pass(r, *g, env, step_cache=0.5)
    fwd.run_forward_pass(r, *g, env)
    assert r.calls == [("forward", 0.5), ("forward", 0.0)]
    r = _Recorder()
    rel.run_relight(r, r, image, env, step_cache=0.125)   # both stages
    rel.run_relight(r, r, image, env)
    assert r.calls == [("inverse", 0.125), ("forward", 0.125), ("inverse", 0.0), ("forward", 0.0)]


def test_nodes_refuse_before_any_upload(pkg):
    inv, fwd, rel = (c() for c in _node_classes(pkg))
    u8 = torch.zeros(1, 9, 48, 64, 3, dtype=torch.uint8)  # uint8 frames are uploaded by the ingest
    env = torch.ones(1, 16, 32, 3)
    bad = ({"step_cache": -0.5}, {"step_cache": 1.5}, {"step_cache": float("nan")}, {"step_cache": "0.1"},
           {"step_cache": 0.1, "tile_join": "latent", "tile_height": 32, "tile_width": 32, "tile_overlap": 8})
    for kw in bad:
        for call in (lambda r: inv.run_inverse_pass(r, u8, **kw), lambda r: fwd.run_forward_pass(r, *[u8] * 5, env, **kw),
                     lambda r: rel.run_relight(r, r, u8, env, **kw)):
            r = _Recorder()
            with pytest.raises(ValueError, match="step_cache"):
                call(r)
            assert not r.calls and not r.touched, kw


def test_header_documents_the_new_entries(pkg):
    text = open(os.path.join(ROOT, "include", "drn.h")).read()
    for name in ("drn_step_cache_probe", "drn_step_cache_workspace_bytes", "drn_step_cache_residual", "drn_step_cache_apply",
                 "drn_dit_forward_range"):
        assert name in pkg.native.SIGNATURES and re.search(r"\b" + name + r"\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "DRN_DIT_EMBED 1" in text and "DRN_DIT_FINAL 2" in text and (pkg.native.DIT_EMBED, pkg.native.DIT_FINAL) == (1, 2)
    lib = pkg.native.load_library()
    assert lib.drn_step_cache_workspace_bytes(1, 8193) == 32 and lib.drn_step_cache_workspace_bytes(3, 8192) == 48
    assert lib.drn_dit_forward_range(None, 0, 0, 3, None) == -1 and lib.drn_dit_forward(None, None) == -1
