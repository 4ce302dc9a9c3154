"""DPM-Solver++(2M) sampler, on the host: the planner against formulas restated here, the order of convergence of the torch
specification on an analytic Gaussian denoiser, the specification against tests/sampler_refs.py, the proof that the inputs of
tests/test_sampler_gpu.py tell a wrong kernel from a right one, the model's loop with a stub DiT, the pipeline and the nodes with
recorders.  No GPU."""
import math

import numpy as np
import pytest
import torch

import sampler_refs as R
from stub_vae import StubVAE

BF = torch.bfloat16


def to_t(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(BF)


def to_bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _scheduler(pkg, steps):
    s = pkg.model_diffusion_renderer.CleanEDMEulerScheduler(sigma_max=R.SIGMA_MAX, sigma_min=R.SIGMA_MIN, sigma_data=R.SIGMA_DATA)
    s.set_timesteps(steps)
    return s


def _plan(pkg, steps, kind="dpmpp_2m"):
    return pkg.sampler.plan_steps(_scheduler(pkg, steps).sigmas, R.SIGMA_DATA, kind)


def _f32(v):
    return float(np.float32(v))


# ----------------------------------------------------------------------------------------------- the planner
@pytest.mark.parametrize("steps", (1, 2, 8, 15, 35))
def test_plan_on_the_reference_schedule(pkg, steps):
    sched = _scheduler(pkg, steps)
    plan = pkg.sampler.plan_steps(sched.sigmas, sched.sigma_data)
    assert len(plan) == steps and pkg.sampler.SAMPLERS == ("euler", "dpmpp_2m")
    sg = [float(v) for v in sched.sigmas]
    for i, (t, p) in enumerate(zip(sched.timesteps, plan)):
        sched.current_step = i
        assert (p.c_in, p.c_skip, p.c_out) == sched.step_scalars(t)[:3]
        assert p.c_in_next == (None if i == steps - 1 else plan[i + 1].c_in)
        assert p.has_hist == (0 < i < steps - 1)
        if i == steps - 1:
            assert (p.a, p.b1, p.b0) == (0.0, 1.0, 0.0)
            continue
        e = 1.0 - sg[i + 1] / sg[i]
        assert p.a == _f32(sg[i + 1] / sg[i])
        if i == 0:
            assert p.b0 == 0.0 and p.b1 == pytest.approx(e, rel=1e-6)
        else:                                              # the schedule is uniform in log sigma: r = 1 up to the table's fp32 rounding
            assert p.b1 == pytest.approx(1.5 * e, rel=2e-5) and p.b0 == pytest.approx(-0.5 * e, rel=2e-5)
        assert p.a + p.b1 + p.b0 == pytest.approx(1.0, abs=3e-7)          # a constant solution stays where it is


def test_plan_on_a_non_uniform_table_is_k_diffusion(pkg):
    """sample_dpmpp_2m's update, restated in float64: t = -log(sigma), h = t_next - t, h_last = t - t_prev, r = h_last / h,
    x' = (sigma_next / sigma) x - expm1(-h) ((1 + 1 / 2r) D - (1 / 2r) D_prev); first step and sigma_next == 0: - expm1(-h) D."""
    table = [80.0, 31.0, 9.5, 7.0, 1.25, 0.9, 0.11, 0.02, 0.0]
    plan = pkg.sampler.plan_steps(torch.tensor(table), 0.5)
    sg = [float(np.float32(v)) for v in table]
    t_of = lambda s: -math.log(s)
    for i, p in enumerate(plan):
        s, sn = sg[i], sg[i + 1]
        if sn == 0:
            assert (p.a, p.b1, p.b0, p.has_hist) == (0.0, 1.0, 0.0, False)       # exp(-inf) = 0: x' = D
            continue
        h = t_of(sn) - t_of(s)
        a, e = sn / s, -math.expm1(-h)
        if i == 0:
            want = (a, e, 0.0)
        else:
            r = (t_of(s) - t_of(sg[i - 1])) / h
            want = (a, e * (1 + 1 / (2 * r)), -e / (2 * r))
        assert (p.a, p.b1, p.b0) == tuple(_f32(v) for v in want), i
        assert p.has_hist == (i > 0)
    assert len({round(math.log(sg[i - 1] / sg[i]) / math.log(sg[i] / sg[i + 1]), 3) for i in range(1, 7)}) > 3     # r varies
    # "euler": every step first order
    for i, (p, q) in enumerate(zip(pkg.sampler.plan_steps(torch.tensor(table), 0.5, "euler"), plan)):
        assert (p.c_in, p.c_skip, p.c_out, p.a, p.c_in_next, p.has_hist, p.b0) == (q.c_in, q.c_skip, q.c_out, q.a, q.c_in_next, False, 0.0)
        assert p.b1 == _f32(1.0 - sg[i + 1] / sg[i])


def test_plan_refusals(pkg):
    S = pkg.sampler
    with pytest.raises(ValueError, match="sampler"):
        S.plan_steps(torch.tensor([1.0, 0.0]), 0.5, "heun")
    for bad in ([1.0], [1.0, 0.5], [1.0, 1.0, 0.0], [0.5, 1.0, 0.0], [1.0, -1.0, 0.0], [float("nan"), 0.0]):
        with pytest.raises(ValueError, match="decreasing"):
            S.plan_steps(torch.tensor(bad), 0.5)
    with pytest.raises(ValueError, match="sampler"):
        S.check_sampler("dpmpp_3m")
    with pytest.raises(ValueError, match="latent"):
        S.check_sampler("dpmpp_2m", "latent")
    S.check_sampler("euler", "latent"), S.check_sampler("dpmpp_2m", "pixel")


# ----------------------------------------------------------------------------------------------- order of convergence
def _solve(pkg, kind, steps, state=torch.float64):
    """The Gaussian problem sampled with step_reference -> the RMS distance to the exact solution.  The network output is what the
    EDM preconditioning makes the denoiser's answer of: m = (D - c_skip x) / c_out, rounded to bf16 with a bf16 state, as in the loop."""
    x0, std = R.gaussian_problem()
    sched = _scheduler(pkg, steps)
    x = x0.to(state)
    hist = None
    for sigma, coef in zip(sched.timesteps, pkg.sampler.plan_steps(sched.sigmas, R.SIGMA_DATA, kind)):
        xd = x.to(torch.float64)
        m = ((R.gaussian_denoiser(xd, float(sigma), std) - coef.c_skip * xd) / coef.c_out).to(state)
        x, hist, _ = pkg.sampler.step_reference(m, None, 0.0, x, hist, coef, state_dtype=state)
    assert x.dtype == state
    return float((x.to(torch.float64) - R.gaussian_truth(x0, std)).pow(2).mean().sqrt())


def test_order_of_convergence(pkg):
    err = {(k, n): _solve(pkg, k, n) for k, n in (("dpmpp_2m", 8), ("dpmpp_2m", 32), ("dpmpp_2m", 64), ("euler", 32), ("euler", 64))}
    print("fp64 state:", {f"{k}@{n}": f"{v:.3e}" for (k, n), v in err.items()})
    assert err["dpmpp_2m", 64] * 3.5 < err["dpmpp_2m", 32] < err["dpmpp_2m", 64] * 4.5            # second order
    assert err["euler", 64] * 1.8 < err["euler", 32] < err["euler", 64] * 2.2                      # first order
    assert err["dpmpp_2m", 8] < err["euler", 64]


def test_bf16_state_still_wins_at_eight_steps(pkg):
    e2m, eul = _solve(pkg, "dpmpp_2m", 8, BF), _solve(pkg, "euler", 35, BF)
    floor = _solve(pkg, "dpmpp_2m", 64, BF)
    print(f"bf16 state: dpmpp_2m@8 {e2m:.3e}, euler@35 {eul:.3e}, dpmpp_2m@64 (the rounding floor, not asserted) {floor:.3e}")
    assert e2m < eul


# ----------------------------------------------------------------------------------------------- specification == reference
def _spec(pkg, c, u, g, x, h, coef, copies, **kw):
    """sampler.step_reference's torch backend on the reference's inputs -> (x_out bits, hist_out float32, scaled bits or None)."""
    xn, D, xs = pkg.sampler.step_reference(to_t(c)[None], None if u is None else to_t(u)[None], g, to_t(x)[None],
                                           None if h is None else torch.from_numpy(h.copy())[None], coef, copies, backend="torch", **kw)
    assert xn.dtype == BF and D.dtype == torch.float32 and (xs is None or (xs.dtype == BF and xs.shape == (copies, x.size)))
    return to_bits(xn[0]), D[0].numpy(), None if xs is None else to_bits(xs)


def _same(a, b):
    return all((p is None and q is None) or (p.dtype == q.dtype and np.array_equal(p.view(np.uint32 if p.dtype == np.float32 else p.dtype),
                                                                                  q.view(np.uint32 if q.dtype == np.float32 else q.dtype)))
               for p, q in zip(a, b))


def _named_cases(pkg):
    """The inputs the GPU test compares on, by name: the value grid and one random case per kind of step, CFG on and off."""
    plan = _plan(pkg, R.PLAN_STEPS)
    for kind, i in R.KINDS.items():
        for cfg in (False, True):
            c, u, x, h = R.value_grid(plan[i], cfg)
            prior = np.full(x.size, np.nan, dtype=np.float32)
            yield f"grid.{kind}.{'cfg' if cfg else 'plain'}", plan[i], c, u, x, h, prior
            c, u, x, h, prior = R.case_inputs(f"spec.{kind}.{cfg}", 257, plan[i], cfg)
            yield f"random.{kind}.{'cfg' if cfg else 'plain'}", plan[i], c, u, x, h, prior


def test_specification_is_the_reference(pkg):
    n = 0
    for name, coef, c, u, x, h, prior in _named_cases(pkg):
        for copies in (1, 2):
            # a NaN-filled history where the step reads none: it must not be touched
            hh = h if coef.has_hist else np.full_like(h, np.nan)
            assert _same(_spec(pkg, c, u, R.GUIDANCE, x, hh, coef, copies), R.step_ref(c, u, R.GUIDANCE, x, hh, coef, copies)), name
            n += 1
    assert n == 24
    # hist_out receives the denoised estimate, and may be the history itself
    coef = _plan(pkg, R.PLAN_STEPS)[3]
    c, u, x, h, _ = R.case_inputs("spec.alias", 64, coef, True)
    buf = torch.from_numpy(h.copy())[None]
    xn, D, xs = pkg.sampler.step_reference(to_t(c)[None], to_t(u)[None], R.GUIDANCE, to_t(x)[None], buf, coef, 2, hist_out=buf)
    assert D is buf and _same((to_bits(xn[0]), buf[0].numpy(), to_bits(xs)), R.step_ref(c, u, R.GUIDANCE, x, h, coef, 2))


def test_grid_tells_every_wrong_kernel_from_the_reference(pkg):
    """Each stand-in differs from the reference on at least one named input the GPU test uses, so a kernel that equals the
    reference on all of them is none of the stand-ins."""
    caught = {v: [] for v in R.VARIANTS}
    for name, coef, c, u, x, h, prior in _named_cases(pkg):
        ref = R.step_ref(c, u, R.GUIDANCE, x, h, coef, 2, prior=prior)
        for v in R.VARIANTS:
            if not _same(R.step_ref(c, u, R.GUIDANCE, x, h, coef, 2, prior=prior, variant=v), ref):
                caught[v].append(name)
    print("cases that catch each stand-in:", {v: len(names) for v, names in caught.items()})
    assert all(caught.values()), [v for v, names in caught.items() if not names]
    # where each is seen first, by name
    assert "grid.first.plain" in caught["hist_read_on_first"]             # the NaN-filled history is the witness
    assert "grid.last.plain" in caught["last_not_first_order"] and "grid.middle.plain" in caught["b_swapped"]
    assert "grid.middle.cfg" in caught["cfg_on_D"] and "grid.middle.cfg" in caught["cfg_fma"]
    assert "grid.first.plain" in caught["scaled_current_c_in"] and "grid.first.plain" in caught["one_copy"]
    for v in ("fma_s1", "fma_s2", "fma_x"):                                # the cancelling history shows them in the bf16 latent
        assert "grid.middle.plain" in caught[v], v
    assert "grid.first.plain" in caught["fma_x"]                           # and the cancelling network output where there is none
    for v in ("hist_not_updated", "hist_is_m", "hist_is_x", "fma_D1", "fma_D2", "scaled_unrounded"):
        assert "random.middle.plain" in caught[v], v


def test_kernel_cases_reach_what_the_kernel_branches_on():
    seen = set()
    for name, n, offs, cfg, copies, kind, alias in R.kernel_cases():
        moved = [s for s in R.SLOTS if offs[s]]
        used = [s for s in R.SLOTS if not ((s == "uncond" and not cfg) or (s == "hist_in" and kind != "middle")
                                           or (s == "scaled_out" and kind == "last"))]
        vec = all(offs[s] * (4 if s.startswith("hist") else 2) % 16 == 0 for s in used) and not (copies == 2 and kind != "last" and n % 8)
        seen |= {("n", n), ("cfg", cfg), ("copies", copies), ("kind", kind), ("alias", alias), ("vec", vec, cfg, kind)}
        seen |= {("off", s, offs[s]) for s in moved}
        if vec and n > R.SWEEP and n % 8:
            seen.add("vector path past one sweep, with a tail")
        if vec and n > R.SWEEP and copies == 2 and kind != "last":
            seen.add("vector path past one sweep, both copies")
        if not vec and n > 2048 * 256:
            seen.add("scalar path past one sweep")
        if offs["uncond"]:
            assert cfg
        if offs["hist_in"]:
            assert kind == "middle"
        if offs["scaled_out"]:
            assert kind != "last"
    want = {("n", n) for n in R.SIZES + R.BIG} | {("cfg", b) for b in (False, True)} | {("copies", 1), ("copies", 2)}
    want |= {("kind", k) for k in R.KINDS} | {("alias", True), ("alias", False)}
    want |= {("off", s, o) for s in R.SLOTS for o in range(1, 8)}
    want |= {("vec", v, c, k) for v in (False, True) for c in (False, True) for k in R.KINDS}
    want |= {"vector path past one sweep, with a tail", "vector path past one sweep, both copies", "scalar path past one sweep"}
    assert want <= seen, want - seen
    assert R.all_finite_bf16().size == 65280 and np.isfinite(R.f32(R.all_finite_bf16())).all()


def test_step_reference_refusals(pkg):
    S = pkg.sampler
    coef = _plan(pkg, 8)[3]
    x = torch.zeros(1, 4, dtype=BF)
    h = torch.zeros(1, 4)
    with pytest.raises(ValueError, match="backend"):
        S.step_reference(x, None, 0.0, x, h, coef, backend="triton")
    with pytest.raises(ValueError, match="hip"):
        S.step_reference(x, None, 0.0, x, h, coef, backend="hip")
    with pytest.raises(ValueError, match="copies"):
        S.step_reference(x, None, 0.0, x, h, coef, copies=3)
    with pytest.raises(ValueError, match="hist"):
        S.step_reference(x, None, 0.0, x, None, coef)
    with pytest.raises(ValueError, match="one latent"):
        S.step_reference(x, torch.zeros(1, 5, dtype=BF), 1.0, x, h, coef)
    with pytest.raises(ValueError, match="state_dtype"):
        S.step_reference(x, None, 0.0, x, h, coef, state_dtype=torch.float16)


# ----------------------------------------------------------------------------------------------- the model's loop
class _StubNet:
    """Stands in for the DiT: a deterministic function of its inputs; the cond and uncond halves differ through the condition."""

    def __init__(self, log):
        self.log = log

    def prepare_timesteps(self, ts):
        self.prepared = list(ts)

    def __call__(self, x, timesteps, latent_condition, context_index):
        self.log.append(("net", tuple(x.shape), float(timesteps), list(context_index)))
        xf, lf = x.float(), latent_condition[:, :16].float()
        idx = torch.tensor(context_index, dtype=torch.float32).view(-1, 1, 1, 1, 1)
        mixed = xf.roll(1, 3) * 0.25 + xf.roll(-1, 4) * 0.5 + xf.mean((3, 4), keepdim=True) + lf * (0.3 + 0.1 * idx)
        return (mixed / (1.0 + float(timesteps))).to(BF)


def _cpu_model(pkg, monkeypatch, log):
    """A model on the CPU whose native calls are logged torch restatements (the kernels' contracts, tests/test_kernels_gpu.py)."""
    mod = pkg.model_diffusion_renderer

    def scale(x, c_in):
        log.append(("edm_scale_input", c_in))
        return (x.float() * c_in).to(BF)

    def cfg(c, u, g):
        log.append(("cfg_combine", g))
        cf = c.float()
        return (cf + ((cf - u.float()).to(BF).float() * g).to(BF).float()).to(BF)

    def step(mo, x, c_skip, c_out, sigma, dt):
        log.append(("edm_step", c_skip, c_out, sigma, dt))
        sm = x.float()
        den = sm * c_skip + mo.float() * c_out
        return (sm + ((sm - den) / torch.tensor(sigma, dtype=torch.float32)) * dt).to(BF)
    monkeypatch.setattr(mod.N, "edm_scale_input", scale)
    monkeypatch.setattr(mod.N, "cfg_combine", cfg)
    monkeypatch.setattr(mod.N, "edm_step", step)
    real = mod.S.step_reference

    def fused(*a, **kw):
        log.append(("step_reference", a[5], a[6], a[4] is None, kw.get("hist_out") is not None))
        return real(*a, **kw)
    monkeypatch.setattr(mod.S, "step_reference", fused)
    cfgd = pkg.diffusion_renderer_config.get_inverse_renderer_config()
    cfgd["model_type"] = "inverse"
    m = mod.CleanDiffusionRendererModel(cfgd, device="cpu")
    m.net, m.vae = _StubNet(log), StubVAE()
    return m


def _batch(pkg, P):
    rgb = pkg.synthetic_weights.synth_tensor("sampler.cpu.rgb", (1, 3, 9, 32, 32), torch.float32, scale=0.6).to(BF)
    return {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[0], [3], [4]][:P], dtype=torch.long)}


@pytest.mark.parametrize("guidance", (0.0, 1.5))
def test_euler_loop_makes_the_calls_it_made(pkg, monkeypatch, guidance):
    """The list is the parent commit's loop read line by line: per step scale_model_input -> N.edm_scale_input, the DiT (under CFG
    on the two halves as one batch), under CFG N.cfg_combine, then scheduler.step -> N.edm_step.  No other native call, no plan."""
    log = []
    m = _cpu_model(pkg, monkeypatch, log)
    noise = pkg.synthetic_weights.synth_tensor("sampler.cpu.xT", (1, 16, 2, 4, 4), torch.float32, scale=80.0)
    runs = []
    for kw in ({}, {"sampler": "euler"}):
        del log[:]
        runs.append(m.generate_samples_from_batch(_batch(pkg, 2), guidance=guidance, seed=3, state_shape=[16, 2, 4, 4], num_steps=3,
                                                  init_noise=noise, **kw))
        per_step = ["edm_scale_input", "net"] + (["cfg_combine"] if guidance > 0 else []) + ["edm_step"]
        assert [e[0] for e in log] == per_step * 3
        sched = _scheduler(pkg, 3)
        for i, t in enumerate(sched.timesteps):
            sched.current_step = i
            sc = sched.step_scalars(t)
            step_log = log[i * len(per_step):(i + 1) * len(per_step)]
            assert step_log[0] == ("edm_scale_input", sc[0]) and step_log[-1] == ("edm_step", *sc[1:])
            assert step_log[1] == ("net", (4 if guidance > 0 else 2, 16, 2, 4, 4), float(t), [0, 3, 0, 0] if guidance > 0 else [0, 3])
            if guidance > 0:
                assert step_log[2] == ("cfg_combine", 1.5)
        assert m.scheduler.current_step == 3
    assert torch.equal(runs[0], runs[1]) and runs[0].shape == (2, 16, 2, 4, 4)


@pytest.mark.parametrize("steps", (1, 2, 4))
@pytest.mark.parametrize("guidance", (0.0, 1.5))
def test_dpmpp_2m_loop_is_one_scale_then_one_fused_step_per_iteration(pkg, monkeypatch, guidance, steps):
    log = []
    m = _cpu_model(pkg, monkeypatch, log)
    P = 2
    noise = pkg.synthetic_weights.synth_tensor("sampler.cpu.xT", (1, 16, 2, 4, 4), torch.float32, scale=80.0)
    keep = noise.clone()
    got = m.generate_samples_from_batch(_batch(pkg, P), guidance=guidance, seed=3, state_shape=[16, 2, 4, 4], num_steps=steps,
                                        init_noise=noise, sampler="dpmpp_2m")
    assert torch.equal(noise, keep) and got.shape == (P, 16, 2, 4, 4) and got.dtype == BF
    plan = _plan(pkg, steps)
    copies = 2 if guidance > 0 else 1
    assert [e[0] for e in log] == ["edm_scale_input"] + ["net", "step_reference"] * steps
    assert log[0] == ("edm_scale_input", plan[0].c_in)
    for i, coef in enumerate(plan):
        assert log[2 + 2 * i] == ("step_reference", coef, copies, not coef.has_hist, True)
        assert log[1 + 2 * i][1] == (copies * P, 16, 2, 4, 4)
    assert m.scheduler.current_step == steps
    # the composition by hand, with the numpy reference
    log2 = []
    net = _StubNet(log2)
    cond = m.prepare_diffusion_renderer_latent_conditions(_batch(pkg, P), m.condition_keys)
    lat = cond.expand(P, *cond.shape[1:])
    idx = [0, 3]
    if guidance > 0:
        lat, idx = torch.cat([lat, torch.zeros_like(lat)]), idx + [0, 0]
    sched = _scheduler(pkg, steps)
    x = to_bits(noise.to(BF).expand(P, 16, 2, 4, 4)).reshape(-1)
    xs = np.stack([R.bf16_bits(R.f32(x) * np.float32(plan[0].c_in))] * copies)
    h = np.full(x.size, np.nan, dtype=np.float32)
    for t, coef in zip(sched.timesteps, plan):
        out = to_bits(net(to_t(xs).reshape(copies * P, 16, 2, 4, 4), t, lat, idx)).reshape(copies, -1)
        x, h, xs = R.step_ref(out[0], out[1] if guidance > 0 else None, guidance, x, h if coef.has_hist else None, coef, copies)
    assert xs is None and np.array_equal(to_bits(got).reshape(-1), x)
    assert [e[1:] for e in log if e[0] == "net"] == [e[1:] for e in log2]


def test_loops_refuse_what_is_not_built(pkg, monkeypatch):
    m = _cpu_model(pkg, monkeypatch, [])
    with pytest.raises(ValueError, match="sampler"):
        m.generate_samples_from_batch(_batch(pkg, 1), state_shape=[16, 2, 4, 4], num_steps=2, sampler="heun")
    tiles = pkg.tiles
    rgb = torch.zeros(1, 3, 9, 48, 64, dtype=BF)
    plan = tiles.plan_tiles(48, 64, 32, 32, 8)
    lat = [tiles.latent_tile(t, 8) for t in plan]
    batches = [{"rgb": rgb[..., t.y:t.y + t.h, t.x:t.x + t.w].contiguous(), "context_index": torch.tensor([[3]])} for t in plan]
    with pytest.raises(ValueError, match="latent"):
        m.generate_samples_joint(batches, lat, (16, 2, 6, 8), num_steps=2, sampler="dpmpp_2m")
    with pytest.raises(ValueError, match="sampler"):
        m.generate_samples_joint(batches, lat, (16, 2, 6, 8), num_steps=2, sampler="heun")
    assert m.generate_samples_joint(batches, lat, (16, 2, 6, 8), num_steps=2, sampler="euler").shape == (1, 16, 2, 6, 8)


# ----------------------------------------------------------------------------------------------- the pipeline
class _RecorderModel:
    process_group = None
    net = None

    def __init__(self):
        self.config = {}
        self.vae = StubVAE()
        self.calls = []

    def to(self, device):
        return self

    def generate_samples_from_batch(self, data_batch, **kw):
        self.calls.append(kw)
        return self.vae.encode(data_batch["rgb"]).to(BF)

    def decode(self, sample):
        return self.vae.decode(sample)


def test_pipeline_hands_the_sampler_on_every_path_and_euler_as_before(pkg, monkeypatch):
    import window_refs as WR
    mod = pkg.diffusion_renderer_pipeline
    monkeypatch.setattr(mod.N, "postprocess_window_u8",
                        lambda video, prev, ramp, ramp_at, lo, hi, normalize, out=None: WR.blend_postprocess(video, prev, ramp, ramp_at,
                                                                                                              lo, hi, normalize))
    model = _RecorderModel()
    p = mod.CleanDiffusionRendererPipeline("/nonexistent", "x.pt", model_type=None, model_instance=model, guidance=0.0, num_steps=2)
    p.device = torch.device("cpu")
    p.set_model_type("inverse")
    assert p.sampler == "euler"
    rgb = pkg.synthetic_weights.synth_tensor("sampler.pipe.rgb", (1, 3, 17, 48, 64), torch.float32, scale=0.6)
    batch = {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[3]], dtype=torch.long)}
    euler_keys = {"guidance", "state_shape", "num_steps", "is_negative_prompt", "seed", "init_noise"}
    paths = {"whole clip": {}, "windows": {"window_frames": 9, "window_overlap": 2},
             "pixel tiles": {"tile_height": 32, "tile_width": 32, "tile_overlap": 8}}
    for name, settings in paths.items():
        for k, v in settings.items():
            setattr(p, k, v)
        for sampler in ("euler", "dpmpp_2m"):
            p.sampler = sampler
            for call in (lambda: p.generate_video(batch, seed=5), lambda: p.generate_video_passes(batch, [False], seed=5),
                         lambda: p.generate_video_each([batch], [False], seed=5)):
                del model.calls[:]
                call()
                assert model.calls, name
                for kw in model.calls:
                    assert set(kw) == (euler_keys if sampler == "euler" else euler_keys | {"sampler"}), (name, sampler)
                    assert kw.get("sampler", "euler") == sampler
        for k in settings:
            setattr(p, k, 0)
    # refusals come before anything is sampled
    del model.calls[:]
    p.sampler = "heun"
    with pytest.raises(ValueError, match="sampler"):
        p.generate_video(batch)
    p.sampler, p.tile_join = "dpmpp_2m", "latent"
    p.tile_height, p.tile_width, p.tile_overlap = 32, 32, 8
    with pytest.raises(ValueError, match="latent"):
        p.generate_video(batch)
    assert not model.calls


# ----------------------------------------------------------------------------------------------- nodes
class _Recorder:
    """A pipeline that records what the nodes set and hand over, and every look at its device (the uploads go there)."""

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
        self.calls.append((self.kind, self.sampler, self.num_steps))
        return self._out(data_batch, to_host)

    def generate_video_passes(self, data_batch, normalize_normal, seed=None, to_host=True):
        self.calls.append((self.kind, self.sampler, self.num_steps))
        return [self._out(data_batch, to_host) for _ in normalize_normal]


def test_node_inputs_and_what_the_nodes_set(pkg):
    classes = [pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"], pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"],
               pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]]
    required = [{"pipeline", "image"}, {"pipeline", "depth", "normal", "roughness", "metallic", "base_color", "env_map"},
                {"inverse_pipeline", "forward_pipeline", "image", "env_map"}]
    for cls, req in zip(classes, required):
        types = cls.INPUT_TYPES()
        assert set(types["required"]) == req
        opt = types["optional"]
        assert opt["sampler"][0] == ["euler", "dpmpp_2m"] and opt["sampler"][1]["default"] == "euler"
        assert opt["steps"][0] == "INT" and opt["steps"][1]["default"] == 0 and opt["steps"][1]["min"] == 0
        assert "second-order" in opt["sampler"][1]["tooltip"] and "0 =" in opt["steps"][1]["tooltip"]
    assert set(pkg.NODE_CLASS_MAPPINGS) >= {"LoadDiffusionRendererModel", "Cosmos1InverseRenderer", "Cosmos1ForwardRenderer", "LoadHDRImage"}
    sw = pkg.synthetic_weights
    image = sw.synth_tensor("sampler.node", (1, 9, 48, 64, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("sampler.env", (1, 16, 32, 3), torch.float32).abs()
    inv, fwd, rel = (c() for c in classes)
    r = _Recorder()
    inv.run_inverse_pass(r, image)                                               # the defaults: euler, the pipeline's own steps
    inv.run_inverse_pass(r, image, sampler="dpmpp_2m", steps=8)
    inv.run_inverse_pass(r, image, sampler="dpmpp_2m")                           # steps = 0: num_steps is left alone
    inv.run_inverse_pass(r, image, steps=0)                                      # every call sets the sampler
    assert r.calls == [("inverse", "euler", 15), ("inverse", "dpmpp_2m", 8), ("inverse", "dpmpp_2m", 8), ("inverse", "euler", 8)]
    r = _Recorder()
    g = [image] * 5
    fwd.run_forward_pass(r, *g, env, sampler="dpmpp_2m", steps=6)
    fwd.run_forward_pass(r, *g, env)
    assert r.calls == [("forward", "dpmpp_2m", 6), ("forward", "euler", 6)]
    r = _Recorder()
    rel.run_relight(r, r, image, env, sampler="dpmpp_2m", steps=4)
    rel.run_relight(r, r, image, env)
    assert r.calls == [("inverse", "dpmpp_2m", 4), ("forward", "dpmpp_2m", 4), ("inverse", "euler", 4), ("forward", "euler", 4)]


def test_nodes_refuse_before_any_upload(pkg):
    classes = [pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"], pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"],
               pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]]
    inv, fwd, rel = (c() for c in classes)
    u8 = torch.zeros(1, 9, 48, 64, 3, dtype=torch.uint8)                          # uint8 frames are uploaded by the ingest
    env = torch.ones(1, 16, 32, 3)
    bad = ({"sampler": "heun"}, {"sampler": "dpmpp_2m", "tile_join": "latent", "tile_height": 32, "tile_width": 32, "tile_overlap": 8},
           {"steps": -1})
    for kw in bad:
        r = _Recorder()
        for run in (lambda: inv.run_inverse_pass(r, u8, **kw), lambda: fwd.run_forward_pass(r, *[u8] * 5, env, **kw),
                    lambda: rel.run_relight(r, r, u8, env, **kw)):
            with pytest.raises(ValueError, match="sampler|latent|steps"):
                run()
        assert not r.calls and not r.touched and r.num_steps == 15 and not hasattr(r, "sampler"), kw
    # and the same inputs without the fault do reach the upload
    r = _Recorder()
    inv.run_inverse_pass(r, u8, sampler="dpmpp_2m", tile_join="pixel", tile_height=32, tile_width=32, tile_overlap=8)
    assert r.calls and "device" in r.touched
