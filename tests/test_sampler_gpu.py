"""DPM-Solver++(2M) sampler, on the GPU: drn_sampler_step_2m bit for bit against tests/sampler_refs.py on the case grid that
tests/test_sampler_cpu.py shows to separate every wrong stand-in, its refusals, the dispatch of sampler.step_reference, and the
model's loop, the pipeline and the nodes under sampler = "dpmpp_2m" against the composition by hand (the DiT with the Euler loop's
own kernels for the scaling and the CFG combine, and the torch specification of the step)."""
import functools

import numpy as np
import pytest
import torch

import sampler_refs as R
from conftest import tiny_net
from stub_vae import StubVAE

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GUARD = 16                       # elements of sentinel on both sides of every tensor: 32 bytes of bf16, 64 of fp32
SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5          # NaN patterns no arithmetic produces


def to_t(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(BF)


def to_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _plan(pkg, steps=R.PLAN_STEPS):
    s = pkg.model_diffusion_renderer.CleanEDMEulerScheduler(sigma_max=R.SIGMA_MAX, sigma_min=R.SIGMA_MIN, sigma_data=R.SIGMA_DATA)
    s.set_timesteps(steps)
    return pkg.sampler.plan_steps(s.sigmas, R.SIGMA_DATA)


class _Buf:
    """A tensor of `n` elements at element offset `off` inside guard bands, on the device; `whole()` brings everything back."""

    def __init__(self, gpu, payload, n, off, fp32=False):
        self.np_dtype, self.sent = (np.uint32, SENT32) if fp32 else (np.uint16, SENT16)
        self.lo, self.n, self.size = GUARD + off, n, 4 if fp32 else 2
        host = np.full(GUARD + off + n + GUARD, self.sent, dtype=self.np_dtype)
        if payload is not None:
            host[self.lo:self.lo + n] = np.ascontiguousarray(payload).view(self.np_dtype)
        self.host = host
        self.dev = torch.from_numpy(host.view(np.int32 if fp32 else np.int16)).to(gpu)
        assert self.dev.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.lo * self.size

    def restore(self):
        self.dev.copy_(torch.from_numpy(self.host.view(np.int32 if self.size == 4 else np.int16)))

    def whole(self):
        return self.dev.cpu().numpy().view(self.np_dtype)

    def expect(self, payload):
        want = self.host.copy()
        if payload is not None:
            want[self.lo:self.lo + self.n] = np.ascontiguousarray(payload).reshape(-1).view(self.np_dtype)
        return want


def _launch_and_compare(pkg, gpu, name, c, u, x, h, prior, coef, copies, offs, alias):
    """One case: every tensor inside guard bands at its element offset, the launch twice (the aliased history restored in
    between), every buffer - inputs included - compared whole with what the reference says it holds afterwards."""
    lib = pkg.native.load_library()
    n = x.size
    last = coef.c_in_next is None
    hist = h if coef.has_hist else None
    want_x, want_h, want_s = R.step_ref(c, u, R.GUIDANCE, x, hist, coef, copies)
    bc, bx = _Buf(gpu, c, n, offs["cond"]), _Buf(gpu, x, n, offs["x"])
    bu = _Buf(gpu, u, n, offs["uncond"]) if u is not None else None
    if alias:
        assert coef.has_hist and offs["hist_in"] == offs["hist_out"]
        bhi = bho = _Buf(gpu, h, n, offs["hist_in"], fp32=True)
    else:
        bhi = _Buf(gpu, h, n, offs["hist_in"], fp32=True) if coef.has_hist else None
        bho = _Buf(gpu, prior, n, offs["hist_out"], fp32=True)
    bo = _Buf(gpu, None, n, offs["x_out"])
    bs = None if last else _Buf(gpu, None, copies * n, offs["scaled_out"])
    for run in range(2):
        rc = lib.drn_sampler_step_2m(bc.ptr, bu.ptr if bu else None, R.GUIDANCE, bx.ptr, bhi.ptr if bhi else None, bho.ptr, bo.ptr,
                                     bs.ptr if bs else None, copies, n, coef.c_skip, coef.c_out, coef.a, coef.b1, coef.b0,
                                     0.0 if last else coef.c_in_next, _stream())
        assert rc == 0, (name, rc)
        torch.cuda.synchronize()
        tag = (name, "run", run)
        assert np.array_equal(bo.whole(), bo.expect(want_x)), tag
        assert np.array_equal(bho.whole(), bho.expect(want_h)), tag
        if bs is not None:
            assert np.array_equal(bs.whole(), bs.expect(want_s)), tag
        for b in (bc, bx, bu, None if alias else bhi):
            if b is not None:
                assert np.array_equal(b.whole(), b.host), tag
        if alias:
            bho.restore()


# ----------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("size", R.SIZES + ("big",))
def test_kernel_is_the_reference_on_the_geometry_grid(pkg, gpu, size):
    plan = _plan(pkg)
    ran = 0
    for name, n, offs, cfg, copies, kind, alias in R.kernel_cases():
        if (n if n in R.SIZES else "big") != size:
            continue
        coef = plan[R.KINDS[kind]]
        c, u, x, h, prior = R.case_inputs("gpu." + name, n, coef, cfg)
        if not coef.has_hist:
            prior = np.full(n, np.nan, dtype=np.float32)          # a history that must not be read
        _launch_and_compare(pkg, gpu, name, c, u, x, h, prior, coef, copies, offs, alias)
        ran += 1
    assert ran == (4 if size == "big" else 56)


@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "cfg"))
@pytest.mark.parametrize("kind", tuple(R.KINDS))
def test_kernel_is_the_reference_on_every_bf16_value(pkg, gpu, kind, cfg):
    """Every finite bf16 value of x against network outputs and histories built so that a contracted multiply-add is seen
    (sampler_refs.value_grid), on the 8-per-lane path and, moved by one element, on the one-per-lane path."""
    coef = _plan(pkg)[R.KINDS[kind]]
    c, u, x, h = R.value_grid(coef, cfg)
    prior = np.full(x.size, np.nan, dtype=np.float32)
    zero = {s: 0 for s in R.SLOTS}
    _launch_and_compare(pkg, gpu, f"grid.{kind}", c, u, x, h, prior, coef, 2, zero, coef.has_hist)
    _launch_and_compare(pkg, gpu, f"grid.{kind}.scalar", c, u, x, h, prior, coef, 1, dict(zero, cond=1), False)


def test_kernel_refusals(pkg, gpu):
    lib = pkg.native.load_library()
    coef = _plan(pkg)[3]
    n = 64
    c, u, x, h, prior = R.case_inputs("gpu.refuse", n, coef, True)
    zero = {s: 0 for s in R.SLOTS}
    bc, bu, bx = _Buf(gpu, c, n, 0), _Buf(gpu, u, n, 0), _Buf(gpu, x, n, 0)
    bh, bho = _Buf(gpu, h, n, 0, fp32=True), _Buf(gpu, prior, n, 0, fp32=True)
    bo, bs = _Buf(gpu, None, n, 0), _Buf(gpu, None, 2 * n, 0)
    good = dict(cond=bc.ptr, uncond=bu.ptr, g=R.GUIDANCE, x=bx.ptr, hist_in=bh.ptr, hist_out=bho.ptr, x_out=bo.ptr, scaled_out=bs.ptr,
                copies=2, n=n, c_skip=coef.c_skip, c_out=coef.c_out, a=coef.a, b1=coef.b1, b0=coef.b0, c_in_next=coef.c_in_next)

    def call(**kw):
        rc = lib.drn_sampler_step_2m(*{**good, **kw}.values(), _stream())
        torch.cuda.synchronize()
        return rc
    bad = [dict(cond=None), dict(x=None), dict(hist_out=None), dict(x_out=None), dict(copies=0), dict(copies=3), dict(n=-1),
           dict(hist_in=None), dict(hist_in=None, b0=float("nan")),
           dict(cond=bc.ptr + 1), dict(uncond=bu.ptr + 1), dict(x=bx.ptr + 1), dict(x_out=bo.ptr + 1), dict(scaled_out=bs.ptr + 1),
           dict(hist_in=bh.ptr + 2), dict(hist_out=bho.ptr + 2)]
    for kw in bad:
        assert call(**kw) == -1, kw                               # DRN_EINVAL
    # nothing was launched: every output still holds what it held
    for b in (bo, bs, bho):
        assert np.array_equal(b.whole(), b.host)
    assert call(n=0) == 0 and call(n=0, scaled_out=None, copies=7) == 0
    for b in (bo, bs, bho):
        assert np.array_equal(b.whole(), b.host)
    # what is NOT refused: copies is not looked at without scaled_out; no history with b0 = 0; no uncond
    assert call(scaled_out=None, copies=7) == 0 and call(hist_in=None, b0=0.0) == 0 and call(uncond=None) == 0 and call() == 0
    want_x, want_h, want_s = R.step_ref(c, u, R.GUIDANCE, x, h, coef, 2)
    assert np.array_equal(bo.whole(), bo.expect(want_x)) and np.array_equal(bs.whole(), bs.expect(want_s))
    assert np.array_equal(bho.whole(), bho.expect(want_h))


def test_step_reference_dispatch(pkg, gpu):
    S = pkg.sampler
    plan = _plan(pkg)
    for kind, cfg, copies in (("first", True, 2), ("middle", False, 1), ("middle", True, 2), ("last", True, 2)):
        coef = plan[R.KINDS[kind]]
        c, u, x, h, _ = R.case_inputs(f"gpu.dispatch.{kind}", 3 * 40, coef, cfg)
        if not coef.has_hist:
            h = np.full_like(h, np.nan)                           # handed over all the same: never read
        want = R.step_ref(c, u, R.GUIDANCE, x, h if coef.has_hist else None, coef, copies)
        shaped = lambda bits: to_t(bits).reshape(3, 40)
        for backend in ("auto", "hip", "torch"):
            for own_out in (False, True):
                hist = torch.from_numpy(h.copy()).reshape(3, 40).to(gpu)
                xn, D, xs = S.step_reference(shaped(c).to(gpu), None if u is None else shaped(u).to(gpu), R.GUIDANCE, shaped(x).to(gpu),
                                             hist, coef, copies, backend=backend, hist_out=hist if own_out else None)
                assert (D is hist) == own_out and xn.shape == (3, 40) and xn.is_cuda and D.dtype == torch.float32
                assert np.array_equal(to_bits(xn).reshape(-1), want[0]), (kind, backend)
                assert np.array_equal(D.cpu().numpy().reshape(-1).view(np.uint32), want[1].view(np.uint32)), (kind, backend)
                if want[2] is None:
                    assert xs is None
                else:
                    assert xs.shape == (3 * copies, 40) and np.array_equal(to_bits(xs).reshape(copies, -1), want[2]), (kind, backend)
    coef = plan[3]
    z = torch.zeros(1, 8, dtype=BF)
    with pytest.raises(ValueError, match="hip"):
        S.step_reference(z, None, 0.0, z, torch.zeros(1, 8), coef, backend="hip")
    with pytest.raises(ValueError, match="hip"):
        S.step_reference(z.double().to(gpu), None, 0.0, z.double().to(gpu), torch.zeros(1, 8, dtype=torch.float64, device=gpu), coef,
                         state_dtype=torch.float64, backend="hip")
    with pytest.raises(ValueError, match="one latent"):
        S.step_reference(z.to(gpu), None, 0.0, z.to(gpu), torch.zeros(1, 8), coef)


# ----------------------------------------------------------------------------------------------- the model's loop
def _by_hand(pkg, model, data_batch, guidance=0.0, seed=1000, state_shape=None, num_steps=15, init_noise=None, sampler=None, **_):
    """generate_samples_from_batch(sampler="dpmpp_2m") written out: the loop's own preamble, then per step the Euler loop's
    kernels for the model input (N.edm_scale_input, torch.cat) and the CFG combine (N.cfg_combine), and the torch specification
    of the step on the combined output."""
    N, S = pkg.native, pkg.sampler
    with torch.no_grad():
        torch.manual_seed(seed)
        condition, _ = model._get_conditions(data_batch)
        sched = model.scheduler
        sched.set_timesteps(num_steps)
        model.net.prepare_timesteps([float(t) for t in sched.timesteps])
        if init_noise is not None:
            xt = init_noise.to(device=model.device, dtype=BF).contiguous()
        else:
            xt = torch.randn(size=(1, *state_shape), device=model.device, dtype=BF) * sched.sigmas[0]
        cond = condition.to_dict()
        cis = [int(v) for v in cond["context_index"].flatten().tolist()] if "context_index" in cond else [0]
        P = len(cis)
        if xt.shape[0] == 1 and P > 1:
            xt = xt.expand(P, *xt.shape[1:]).contiguous()
        lat = cond["latent_condition"]
        lat = lat.expand(P, *lat.shape[1:]) if P > 1 else lat
        idx = cis
        if guidance > 0:
            lat, idx = torch.cat([lat, torch.zeros_like(lat)], 0), cis + [0] * P
        hist = None
        for t, coef in zip(sched.timesteps, S.plan_steps(sched.sigmas, sched.sigma_data)):
            xs = N.edm_scale_input(xt, coef.c_in)
            if guidance > 0:
                both = model.net(x=torch.cat([xs, xs], 0), timesteps=t, latent_condition=lat, context_index=idx)
                m = N.cfg_combine(both[:P].contiguous(), both[P:].contiguous(), float(guidance))
            else:
                m = model.net(x=xs, timesteps=t, latent_condition=lat, context_index=idx)
            xt, hist, _ = S.step_reference(m, None, 0.0, xt, hist, coef, backend="torch")
        return xt


H, W = 48, 64


def _pipeline(pkg, gpu):
    sw = pkg.synthetic_weights
    models = {}
    for kind, fw in (("inverse", False), ("forward", True)):
        net = tiny_net(pkg, 256, 1, 2, forward=fw)
        cfgm = pkg.diffusion_renderer_config
        cfg = cfgm.get_forward_renderer_config() if fw else cfgm.get_inverse_renderer_config()
        cfg["net"] = dict(net)
        cfg["model_type"] = kind
        m = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=gpu)
        m.load_state_dict(sw.synth_state_dict(net, BF, device=gpu), strict=True)
        models[kind] = m
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=StubVAE(), model_instance=models, guidance=0.0, num_steps=2)
    p.device = gpu
    p.set_model_type("inverse")
    return p


@pytest.fixture(scope="module")
def pipe(pkg, gpu):
    return _pipeline(pkg, gpu)


def _reset(p):
    p.set_model_type("inverse")
    p.guidance, p.restore_plan, p.num_steps, p.sampler = 0.0, None, 2, "euler"
    p.window_frames, p.window_overlap, p.tile_height, p.tile_width, p.tile_overlap, p.tile_join = 0, 8, 0, 0, 64, "pixel"


@pytest.mark.parametrize("steps", (1, 2, 8))
@pytest.mark.parametrize("guidance", (0.0, 2.0))
@pytest.mark.parametrize("P", (1, 5))
def test_model_loop_is_the_composition_by_hand(pkg, gpu, pipe, P, guidance, steps):
    model = pipe.pre_loaded_model_instance["inverse"]
    model.vae = StubVAE()
    sw = pkg.synthetic_weights
    rgb = sw.synth_tensor("sampler.gpu.rgb", (1, 3, 9, 32, 32), torch.float32, scale=0.6).to(BF).to(gpu)
    noise = sw.synth_tensor("sampler.gpu.xT", (1, 16, 2, 4, 4), torch.float32, scale=80.0)
    batch = lambda: {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[0], [3], [4], [1], [2]][:P], dtype=torch.long, device=gpu)}
    kw = dict(guidance=guidance, seed=7, state_shape=[16, 2, 4, 4], num_steps=steps)
    got = model.generate_samples_from_batch(batch(), init_noise=noise, sampler="dpmpp_2m", **kw)
    assert model.scheduler.current_step == steps
    want = _by_hand(pkg, model, batch(), init_noise=noise, **kw)
    assert got.shape == (P, 16, 2, 4, 4) and got.dtype == BF and torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
    # drawn from the seed where no noise is handed over
    a = model.generate_samples_from_batch(batch(), sampler="dpmpp_2m", **kw)
    assert torch.equal(a, _by_hand(pkg, model, batch(), **kw)) and not torch.equal(a, got)
    # the two samplers are different samplers from the first step that reads a history on (up to two steps 2M's steps are
    # Euler's: a first-order step, then the step to sigma = 0)
    euler = model.generate_samples_from_batch(batch(), init_noise=noise, **kw)
    assert torch.equal(euler, model.generate_samples_from_batch(batch(), init_noise=noise, sampler="euler", **kw))
    if steps > 2:
        assert not torch.equal(euler, got)


def _patched(pkg, p, monkeypatch):
    for model in p.pre_loaded_model_instance.values():
        monkeypatch.setattr(model, "generate_samples_from_batch", functools.partial(_by_hand, pkg, model))


@pytest.mark.parametrize("path", ("whole_clip", "windowed", "pixel_tiled"))
def test_generate_video_is_the_composition_by_hand(pkg, gpu, pipe, monkeypatch, path):
    p = pipe
    _reset(p)
    sw = pkg.synthetic_weights
    T = 17 if path == "windowed" else 9
    if path == "windowed":
        p.window_frames, p.window_overlap = 9, 2
    if path == "pixel_tiled":
        p.tile_height, p.tile_width, p.tile_overlap = 32, 32, 8
    p.guidance, p.num_steps = 1.5, 3
    rgb = sw.synth_tensor(f"sampler.gpu.clip{T}", (1, 3, T, H, W), torch.float32, scale=1.0)
    ci = torch.tensor([[0], [3]], dtype=torch.long)
    batch = {"rgb": rgb, "video": rgb, "context_index": ci}
    one = dict(batch, context_index=ci[1:2])
    euler = p.generate_video(one, normalize_normal=True, seed=5)
    p.sampler = "dpmpp_2m"
    got = [p.generate_video(one, normalize_normal=True, seed=5), *p.generate_video_passes(batch, [False, True], seed=5),
           *p.generate_video_each([dict(batch, context_index=ci[0:1]), one], [False, True], seed=5)]
    _patched(pkg, p, monkeypatch)
    want = [p.generate_video(one, normalize_normal=True, seed=5), *p.generate_video_passes(batch, [False, True], seed=5),
            *p.generate_video_each([dict(batch, context_index=ci[0:1]), one], [False, True], seed=5)]
    monkeypatch.undo()
    assert all(g.shape == (1, T, H, W, 3) and g.dtype == np.uint8 for g in got)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (path, k, int((g != w).sum()))
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], euler)
    # the sampler set explicitly to "euler" is the default call
    p.sampler = "euler"
    assert np.array_equal(p.generate_video(one, normalize_normal=True, seed=5), euler)
    p.tile_join = "latent"
    p.sampler = "dpmpp_2m"
    with pytest.raises(ValueError, match="latent"):
        p.generate_video(one, normalize_normal=True, seed=5)
    _reset(p)


def test_nodes_under_dpmpp_2m_are_the_composition_by_hand(pkg, gpu, pipe, monkeypatch):
    p = pipe
    _reset(p)
    sw = pkg.synthetic_weights
    T = 9
    image = sw.synth_tensor("sampler.node.img", (1, T, H, W, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("sampler.node.env", (1, 32, 64, 3), torch.float32).abs() * 4.0
    inv = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    fwd = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    rel = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    kw = dict(seed=3, sampler="dpmpp_2m", steps=3)

    def run():
        g = inv.run_inverse_pass(p, image, guidance=1.0, **kw)
        assert (p.sampler, p.num_steps) == ("dpmpp_2m", 3)
        g5 = [o.reshape(1, T, H, W, 3) for o in g]
        (lit,) = fwd.run_forward_pass(p, g5[4], g5[3], g5[2], g5[1], g5[0], env, guidance=0.0, env_spin=45.0, **kw)
        return [*g, lit, *rel.run_relight(p, p, image, env, env_spin=45.0, **kw)]
    got = run()
    _patched(pkg, p, monkeypatch)
    want = run()
    monkeypatch.undo()
    assert len(got) == 12
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), k
    # the defaults are the Euler nodes: the sampler goes back, the steps stay (0 = leave them alone)
    e = inv.run_inverse_pass(p, image, guidance=1.0, seed=3)
    assert (p.sampler, p.num_steps) == ("euler", 3) and not torch.equal(e[0], got[0])
    assert all(torch.equal(a, b) for a, b in zip(e, inv.run_inverse_pass(p, image, guidance=1.0, seed=3, sampler="euler", steps=3)))
    _reset(p)
