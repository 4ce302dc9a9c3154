"""The step cache on the GPU (step_cache.py, csrc/step_cache.hip, drn_dit_forward_range): the three kernels bit for
bit against tests/step_cache_refs.py, the forward in parts against drn_dit_forward, the engine's loop against the composition by
hand from range calls and torch, and the model loop, the pipeline and the nodes against that composition."""
import ctypes

import numpy as np
import pytest
import torch

import step_cache_refs as R
from conftest import tiny_net
from stub_vae import StubVAE

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 64                    # elements of poison in front of and behind every tensor a kernel writes


def to_t(bits, device=None):
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(BF)
    return t if device is None else t.to(device)


def to_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _at(bits, off, gpu, fill=0x7FC0):
    """`bits` on the device at element offset `off` of a 16-byte aligned allocation, guard bands of `fill` around it ->
    (the whole allocation, the view)."""
    flat = np.full(GUARD + off + bits.size + GUARD + 8, fill, dtype=np.uint16)
    flat[GUARD + off:GUARD + off + bits.size] = bits.reshape(-1)
    whole = to_t(flat, gpu)
    return whole, whole[GUARD + off:GUARD + off + bits.size]


def _guards_intact(whole, off, size, fill=0x7FC0):
    b = to_bits(whole)
    return bool((b[:GUARD + off] == fill).all() and (b[GUARD + off + size:] == fill).all())


# ----------------------------------------------------------------------------------------------- the probe
def _probe(pkg, gpu, xb, rb, xo=0, ro=0, so=0):
    lib = pkg.native.load_library()
    B, n = xb.shape
    _, x = _at(xb, xo, gpu)
    _, r = _at(rb, ro, gpu)
    nbytes = lib.drn_step_cache_workspace_bytes(B, n)
    assert nbytes == B * -(-n // 8192) * 2 * 8
    poison = float(np.array([0x7FF4DEADBEEF0001], dtype=np.uint64).view(np.float64)[0])
    results = []
    for _ in range(2):                                    # every launch twice: the same bits
        stats = torch.full((4 + so + 2 * B + 4,), poison, dtype=torch.float64, device=gpu)
        ws = torch.full((nbytes // 8 + 4,), poison, dtype=torch.float64, device=gpu)
        rc = lib.drn_step_cache_probe(x.data_ptr(), r.data_ptr(), stats[4 + so:].data_ptr(), ws.data_ptr(), nbytes, B, n, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        s = stats.cpu().numpy().view(np.uint64)
        w = ws.cpu().numpy().view(np.uint64)
        pb = np.array([poison]).view(np.uint64)[0]
        assert (s[:4 + so] == pb).all() and (s[4 + so + 2 * B:] == pb).all() and (w[nbytes // 8:] == pb).all()
        results.append(s[4 + so:4 + so + 2 * B].reshape(B, 2).copy())
    assert np.array_equal(results[0], results[1])
    return results[0]


@pytest.mark.parametrize("case", R.probe_cases(), ids=lambda c: c[0])
def test_probe_is_the_reference_bit_for_bit(pkg, gpu, case):
    name, B, n, xo, ro, so = case
    rb = R.rand_bits("probe.ref." + name, (B, n), 1.5)
    xb = R.bf16_bits(R.f32(rb) + R.f32(R.rand_bits("probe.d." + name, (B, n), 0.05)))
    got = _probe(pkg, gpu, xb, rb, xo, ro, so)
    want = R.probe_ref(xb, rb).view(np.uint64)
    assert np.array_equal(got, want), (name, got, want)
    assert np.isfinite(want.view(np.float64)).all() and (want.view(np.float64)[:, 1] > 0).all()


def test_probe_special_values(pkg, gpu):
    n = 8192 + 9
    rb = R.rand_bits("probe.sp.ref", (3, n), 1.0)
    xb = R.rand_bits("probe.sp.x", (3, n), 1.0)
    # clip 0: an all-zero ref (den = 0); clip 1: inf - inf and a NaN in x; clip 2: inf in ref only
    rb[0] = 0
    xb[1, 5], rb[1, 5] = 0x7F80, 0x7F80
    xb[1, 8200] = 0xFFC0
    rb[2, 17] = 0xFF80
    for xo, ro in ((0, 0), (3, 5)):
        got = _probe(pkg, gpu, xb, rb, xo, ro)
        want = R.probe_ref(xb, rb)
        assert np.array_equal(got, want.view(np.uint64))
        assert want[0, 1] == 0.0 and np.isnan(want[1, 0]) and np.isinf(want[2]).all()
        assert got[1, 0] == R.QNAN64
    assert R.delta_ref(R.probe_ref(xb, rb)) == float("inf")


def test_probe_refusals_launch_nothing(pkg, gpu):
    lib = pkg.native.load_library()
    B, n = 2, 8200
    x = torch.zeros(B * n + 8, dtype=BF, device=gpu)
    ref = torch.ones(B * n + 8, dtype=BF, device=gpu)
    nbytes = lib.drn_step_cache_workspace_bytes(B, n)
    stats = torch.full((2 * B + 1,), -7.0, dtype=torch.float64, device=gpu)
    ws = torch.full((nbytes // 8 + 1,), -7.0, dtype=torch.float64, device=gpu)
    good = [x.data_ptr(), ref.data_ptr(), stats.data_ptr(), ws.data_ptr(), nbytes, B, n]
    bad = {"null x": {0: None}, "null ref": {1: None}, "null stats": {2: None}, "null workspace": {3: None},
           "short workspace": {4: nbytes - 8}, "B = 0": {5: 0}, "B < 0": {5: -1}, "n = 0": {6: 0}, "n < 0": {6: -5},
           "x off 2 bytes": {0: x.data_ptr() + 1}, "ref off 2 bytes": {1: ref.data_ptr() + 1},
           "stats off 8 bytes": {2: stats.data_ptr() + 4}, "workspace off 8 bytes": {3: ws.data_ptr() + 4}}
    for what, change in bad.items():
        a = list(good)
        for k, v in change.items():
            a[k] = v
        assert lib.drn_step_cache_probe(*a, _stream()) == -1, what
    torch.cuda.synchronize()
    assert bool((stats == -7.0).all()) and bool((ws == -7.0).all())
    assert lib.drn_step_cache_workspace_bytes(0, 5) == 0 and lib.drn_step_cache_workspace_bytes(2, 0) == 0
    assert lib.drn_step_cache_workspace_bytes(10, 18432 * 4096) == 10 * 9216 * 16
    assert lib.drn_step_cache_probe(*good, _stream()) == 0
    torch.cuda.synchronize()
    assert stats[:2 * B].tolist() == [float(n), float(n)] * B and float(stats[-1]) == -7.0


# ----------------------------------------------------------------------------------------------- residual and apply
def _combine(pkg, gpu, which, ab, bb, ao=0, bo=0, oo=0):
    """which: "residual" (out = a - b into a third tensor) or "apply" (a = a + b in place), twice each."""
    lib = pkg.native.load_library()
    n = ab.size
    want = R.residual_ref(ab, bb) if which == "residual" else R.apply_ref(ab, bb)
    for _ in range(2):
        wa, a = _at(ab, ao, gpu, 0x4111)
        wb, b = _at(bb, bo, gpu, 0x4222)
        if which == "residual":
            wo, o = _at(np.full(n, 0x4333, dtype=np.uint16), oo, gpu, 0x4333)
            rc = lib.drn_step_cache_residual(a.data_ptr(), b.data_ptr(), o.data_ptr(), n, _stream())
        else:
            wo, o, oo = wa, a, ao
            rc = lib.drn_step_cache_apply(a.data_ptr(), b.data_ptr(), n, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        got = to_bits(o)
        assert np.array_equal(got, want.reshape(-1)), (which, n, ao, bo, oo, int((got != want.reshape(-1)).sum()))
        assert _guards_intact(wo, oo, n, 0x4333 if which == "residual" else 0x4111)
        assert np.array_equal(to_bits(b), bb.reshape(-1)) and _guards_intact(wb, bo, n, 0x4222)
        if which == "residual":
            assert np.array_equal(to_bits(a), ab.reshape(-1)) and _guards_intact(wa, ao, n, 0x4111)


@pytest.mark.parametrize("which", ("residual", "apply"))
@pytest.mark.parametrize("n", R.EW_SIZES)
def test_residual_and_apply_on_the_geometry_grid(pkg, gpu, which, n):
    ab = R.rand_bits(f"ew.a.{n}", (n,), 2.0)
    bb = R.rand_bits(f"ew.b.{n}", (n,), 2.0)
    _combine(pkg, gpu, which, ab, bb)
    if n == 8193:
        for off in range(1, 8):                           # every tensor off the 16-byte grid, alone and together
            for offs in ((off, 0, 0), (0, off, 0), (0, 0, off), (off, off, off)):
                _combine(pkg, gpu, which, ab, bb, *offs)


@pytest.mark.parametrize("which", ("residual", "apply"))
def test_residual_and_apply_on_every_bf16_value(pkg, gpu, which):
    """Every finite bf16 x against a handful of partners, and inf / NaN against each other: torch's (a.float() -/+ b.float())
    .bfloat16() bit for bit, a NaN as 0x7FC0 (the reference is held against torch here as well: step_cache_refs.same_as_torch)."""
    xs = R.all_finite_bf16()
    assert xs.size == 65280
    partners = np.array([0x0000, 0x8000, 0x3F80, 0xBF80, 0x0001, 0x7F7F, 0xFF7F, 0x3C00, 0x4049, 0x0080], dtype=np.uint16)
    special = np.array([0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7FFF, 0x3F80, 0x0000], dtype=np.uint16)
    ab = np.concatenate([np.repeat(xs, partners.size), np.repeat(special, special.size)])
    bb = np.concatenate([np.tile(partners, xs.size), np.tile(special, special.size)])
    _combine(pkg, gpu, which, ab, bb)
    ta, tb = to_t(ab), to_t(bb)
    tref = (ta.float() - tb.float()).bfloat16() if which == "residual" else (ta.float() + tb.float()).bfloat16()
    assert R.same_as_torch(R.residual_ref(ab, bb) if which == "residual" else R.apply_ref(ab, bb), to_bits(tref))


def test_residual_and_apply_refusals_launch_nothing(pkg, gpu):
    lib = pkg.native.load_library()
    a = torch.full((64,), 3.0, dtype=BF, device=gpu)
    b = torch.full((64,), 1.0, dtype=BF, device=gpu)
    o = torch.full((64,), 9.0, dtype=BF, device=gpu)
    pa, pb, po = a.data_ptr(), b.data_ptr(), o.data_ptr()
    for args in ((None, pb, po, 64), (pa, None, po, 64), (pa, pb, None, 64), (pa, pb, po, 0), (pa, pb, po, -1),
                 (pa + 1, pb, po, 32), (pa, pb + 1, po, 32), (pa, pb, po + 1, 32)):
        assert lib.drn_step_cache_residual(*args, _stream()) == -1, args
    for args in ((None, pb, 64), (pa, None, 64), (pa, pb, 0), (pa + 1, pb, 32), (pa, pb + 1, 32)):
        assert lib.drn_step_cache_apply(*args, _stream()) == -1, args
    torch.cuda.synchronize()
    assert bool((a == 3.0).all()) and bool((b == 1.0).all()) and bool((o == 9.0).all())


# ----------------------------------------------------------------------------------------------- the forward in parts
def _engine(pkg, gpu, D, L, heads, **kw):
    net = tiny_net(pkg, D, L, heads)
    sd = pkg.synthetic_weights.synth_state_dict(net, BF, device=gpu)
    return pkg.dit_engine.HipDiT(net, sd, device=gpu, **kw), net


def _inputs(pkg, gpu, lat, B, name="sc"):
    sw = pkg.synthetic_weights
    x = sw.synth_tensor(name + ".x", (B, 16) + lat, torch.float32, device=gpu, scale=2.0).to(BF)
    cond = sw.synth_tensor(name + ".c", (B, 16) + lat, torch.float32, device=gpu, scale=1.0).to(BF)
    return x, cond, [3, 0, 4][:B]


def _with_body(pkg, monkeypatch, eng, body, call):
    """Run `call()` with the engine's one-call forward replaced by body(args, X): X = the engine's residual stream [B S, D]."""
    with monkeypatch.context() as m:
        m.setattr(pkg.native, "dit_forward", lambda args: body(args, next(iter(eng._ws.values()))["x"]))
        return call()


@pytest.mark.parametrize("precision,fused", [("bf16", "1"), ("mxfp8", "0"), ("mxfp8", "1")])
@pytest.mark.parametrize("D,L,heads,lat,B", [(256, 2, 2, (2, 16, 16), 1), (256, 2, 2, (2, 16, 16), 3), (2048, 2, 16, (1, 32, 32), 1),
                                               (2048, 2, 16, (1, 32, 32), 3)])
def test_three_parts_are_the_forward_bit_for_bit(pkg, gpu, monkeypatch, D, L, heads, lat, B, precision, fused):
    """[0, 3) EMBED, [3, n_sub), FINAL in three calls == drn_dit_forward.  At D = 2048 the out-projection and MLP-down defer
    their split-K sums inside drn_dit_forward; the head's last linear does not (X is complete when the call returns)."""
    monkeypatch.setenv("DRN_MX_FUSED", fused)
    N = pkg.native
    eng, _ = _engine(pkg, gpu, D, L, heads, precision=precision)
    x, cond, ci = _inputs(pkg, gpu, lat, B)
    n_sub = len(eng._subs_c)
    assert n_sub == 3 * L and [k for k in eng.kinds] == ["fa", "ca", "mlp"]
    eng.prepare_timesteps([80.0, 1.7])
    calls = []

    def parts(args, X):
        N.dit_forward_range(args, 0, 3, N.DIT_EMBED)
        N.dit_forward_range(args, 3, n_sub, 0)
        N.dit_forward_range(args, n_sub, n_sub, N.DIT_FINAL)
        calls.append(n_sub)
    for sigma in (1.7, 80.0):
        want = eng(x, torch.tensor(sigma), cond, ci).clone()
        got = _with_body(pkg, monkeypatch, eng, parts, lambda: eng(x, torch.tensor(sigma), cond, ci).clone())
        torch.cuda.synchronize()
        assert torch.isfinite(want.float()).all()
        assert torch.equal(got, want), f"sigma {sigma}: max |diff| {(got.float() - want.float()).abs().max().item()}"
    assert len(calls) == 2


def test_range_refusals_launch_nothing(pkg, gpu, monkeypatch):
    N = pkg.native
    lib = N.load_library()
    eng, _ = _engine(pkg, gpu, 256, 2, 2)
    x, cond, ci = _inputs(pkg, gpu, (2, 16, 16), 1)
    seen = {}

    def body(args, X):
        ws = next(iter(eng._ws.values()))
        for k in ("x", "y", "h"):
            ws[k].fill_(7.0)
        args.struct_bytes = ctypes.sizeof(N.DitForwardArgs)
        args.timer = None
        st = _stream()
        bad = {"lo > hi": (2, 1, 0), "lo < 0": (-1, 2, 0), "hi > n_sub": (0, 7, 3), "lo > n_sub": (7, 7, 2), "unknown flag": (0, 6, 4),
               "ends on a CA without FINAL": (0, 2, 1), "a CA alone": (1, 2, 0)}
        for what, (lo, hi, flags) in bad.items():
            assert lib.drn_dit_forward_range(ctypes.byref(args), lo, hi, flags, st) == -1, what
        args.struct_bytes -= 8
        assert lib.drn_dit_forward_range(ctypes.byref(args), 0, 6, 3, st) == -1
        args.struct_bytes += 8
        torch.cuda.synchronize()
        seen["untouched"] = all(bool((ws[k] == 7.0).all()) for k in ("x", "y", "h"))
        # the empty part launches nothing and is no error; a part that ends on a CA is fine where the final layer follows it
        assert lib.drn_dit_forward_range(ctypes.byref(args), 3, 3, 0, st) == 0
        torch.cuda.synchronize()
        seen["empty"] = all(bool((ws[k] == 7.0).all()) for k in ("x", "y", "h"))
        assert lib.drn_dit_forward_range(ctypes.byref(args), 0, 2, 3, st) == 0
    _with_body(pkg, monkeypatch, eng, body, lambda: eng(x, torch.tensor(1.7), cond, ci))
    torch.cuda.synchronize()
    assert seen == {"untouched": True, "empty": True}


# ----------------------------------------------------------------------------------------------- the engine
class HandCache:
    """The step cache of one engine composed by hand: range calls for the three parts, torch for copy, residual and apply, the
    numpy reference for the probe on the tensors read back.  Stands where the engine stands (net(...), prepare_timesteps,
    cache_begin / cache_end)."""

    def __init__(self, pkg, monkeypatch, eng):
        self.pkg, self.mp, self.eng = pkg, monkeypatch, eng
        self.loop = None
        self.step_cache_log = []
        self.x1 = []                                      # per step (X1 bits, ref bits or None): what the probe saw

    def prepare_timesteps(self, ts):
        self.eng.prepare_timesteps(ts)

    def cache_begin(self, thr, max_run, n_steps):
        self.loop = dict(thr=thr, max_run=max_run, n=n_steps, i=0, run=0, ref=None, R=None)
        self.step_cache_log = []
        self.x1 = []

    def cache_end(self):
        self.loop = None

    def __call__(self, x, timesteps, latent_condition, context_index=None):
        N, eng, c = self.pkg.native, self.eng, self.loop
        if c is None:
            return eng(x, timesteps, latent_condition, context_index)
        B, n_sub = x.shape[0], len(eng._subs_c)

        def body(args, X):
            N.dit_forward_range(args, 0, 3, N.DIT_EMBED)
            forced = c["i"] == 0 or c["i"] == c["n"] - 1 or c["run"] >= c["max_run"]
            delta = None
            x1 = X.clone()
            self.x1.append((to_bits(x1).reshape(B, -1), None if c["ref"] is None else to_bits(c["ref"]).reshape(B, -1)))
            if not forced:
                delta = R.delta_ref(R.probe_ref(*self.x1[-1]))
            if not forced and delta < c["thr"]:
                X.copy_((x1.float() + c["R"].float()).bfloat16())
                c["run"] += 1
            else:
                c["ref"] = x1
                N.dit_forward_range(args, 3, n_sub, 0)
                c["R"] = (X.float() - x1.float()).bfloat16()
                c["run"] = 0
            self.step_cache_log.append((forced or not delta < c["thr"], delta))
            c["i"] += 1
            N.dit_forward_range(args, n_sub, n_sub, N.DIT_FINAL)
        return _with_body(self.pkg, self.mp, eng, body, lambda: eng(x, timesteps, latent_condition, context_index))


SIGMAS = (80.0, 20.0, 5.0, 1.7, 0.3)


@pytest.mark.parametrize("B", (1, 3))
def test_engine_loop_is_the_composition_by_hand(pkg, gpu, monkeypatch, B):
    eng, _ = _engine(pkg, gpu, 256, 2, 2)
    hand_eng, _ = _engine(pkg, gpu, 256, 2, 2)
    x, cond, ci = _inputs(pkg, gpu, (2, 16, 16), B)
    xs = [(x.float() * (1.0 - 0.04 * i)).to(BF) for i in range(5)]            # a moving x
    eng.prepare_timesteps(SIGMAS)
    hand_eng.prepare_timesteps(SIGMAS)
    plain = [eng(xi, torch.tensor(s), cond, ci).clone() for xi, s in zip(xs, SIGMAS)]
    assert eng.step_cache_log == []

    # thr = 1e-30: every step is computed, and each output is the plain forward's
    eng.cache_begin(1e-30, 3, 5)
    try:
        got = [eng(xi, torch.tensor(s), cond, ci).clone() for xi, s in zip(xs, SIGMAS)]
    finally:
        eng.cache_end()
    assert eng._cache is None
    assert [c for c, _ in eng.step_cache_log] == [True] * 5
    assert [d is None for _, d in eng.step_cache_log] == [True, False, False, False, True]
    for g, w in zip(got, plain):
        assert torch.equal(g, w)
    # outside a begin / end pair the forward is untouched
    assert torch.equal(eng(xs[2], torch.tensor(SIGMAS[2]), cond, ci), plain[2])

    # thr = 1.0, max_run = 2: the controller's pattern, every output the composition by hand, the logged deltas the reference's
    hand = HandCache(pkg, monkeypatch, hand_eng)
    hand.cache_begin(1.0, 2, 5)
    want = [hand(xi, torch.tensor(s), cond, ci).clone() for xi, s in zip(xs, SIGMAS)]
    eng.cache_begin(1.0, 2, 5)
    try:
        got = [eng(xi, torch.tensor(s), cond, ci).clone() for xi, s in zip(xs, SIGMAS)]
    finally:
        eng.cache_end()
    torch.cuda.synchronize()
    assert eng.step_cache_log == hand.step_cache_log and _rule_holds(eng.step_cache_log, 2)
    skipped = [i for i, (c, _) in enumerate(eng.step_cache_log) if not c]
    assert skipped, eng.step_cache_log
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), i
    assert torch.equal(got[0], plain[0]) and all(not torch.equal(got[i], plain[i]) for i in skipped)
    for (computed, delta), (x1, ref) in zip(eng.step_cache_log, hand.x1):
        if delta is not None:
            assert delta == R.delta_ref(R.probe_ref(x1, ref)) and delta > 0 and computed == (delta >= 1.0)


def test_engine_refusals(pkg, gpu):
    eng, _ = _engine(pkg, gpu, 256, 2, 2)
    x, cond, ci = _inputs(pkg, gpu, (2, 16, 16), 1)
    for thr, run in ((0.0, 3), (-0.1, 3), (float("nan"), 3), (2.0, 3), (0.1, 0)):
        with pytest.raises(ValueError):
            eng.cache_begin(thr, run, 4)
        assert eng._cache is None
    eng.trace = {}
    with pytest.raises(ValueError, match="trace"):
        eng.cache_begin(0.1, 3, 4)
    eng.trace = None
    eng._per_launch = True
    with pytest.raises(ValueError, match="DRN_PER_LAUNCH"):
        eng.cache_begin(0.1, 3, 4)
    eng._per_launch = False
    eng.cache_begin(0.1, 3, 4)
    try:
        with pytest.raises(RuntimeError, match="cache_end"):
            eng.cache_begin(0.1, 3, 4)
        eng(x, torch.tensor(1.7), cond, ci)
        with pytest.raises(ValueError, match="shape"):
            eng(torch.cat([x, x]), torch.tensor(1.7), cond, [3, 3])
        eng.trace = {}
        with pytest.raises(ValueError, match="trace"):
            eng(x, torch.tensor(1.7), cond, ci)
        eng.trace = None
    finally:
        eng.cache_end()
    eng.pg = object()
    with pytest.raises(NotImplementedError, match="sequence parallelism"):
        eng.cache_begin(0.1, 3, 4)
    eng.pg = None
    # fewer than 2 blocks: the setting is ignored
    one, _ = _engine(pkg, gpu, 256, 1, 2)
    plain = one(x, torch.tensor(1.7), cond, ci).clone()
    one.cache_begin(1.0, 3, 2)
    assert one._cache is None and torch.equal(one(x, torch.tensor(1.7), cond, ci), plain)
    one.cache_end()
    assert one.step_cache_log == []


# ----------------------------------------------------------------------------------------------- model, pipeline, nodes
H, W = 48, 64


@pytest.fixture(scope="module")
def pipe(pkg, gpu):
    sw = pkg.synthetic_weights
    models = {}
    for kind, fw in (("inverse", False), ("forward", True)):
        net = tiny_net(pkg, 256, 2, 2, forward=fw)
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


def _reset(p):
    p.set_model_type("inverse")
    p.guidance, p.restore_plan, p.num_steps, p.sampler, p.step_cache, p.step_cache_max_run = 0.0, None, 2, "euler", 0.0, 3
    p.window_frames, p.window_overlap, p.tile_height, p.tile_width, p.tile_overlap, p.tile_join = 0, 8, 0, 0, 64, "pixel"
    p.ensemble = 1


def _rule_holds(log, max_run):
    """What the rule forces, whatever the probe said: first and last step computed, never more than max_run skipped in a row."""
    computed = [c for c, _ in log]
    runs = "".join("c" if c else "s" for c in computed).split("c")
    return computed[0] and computed[-1] and max(len(r) for r in runs) <= max_run and log[0][1] is None and log[-1][1] is None


def _by_hand(pkg, models, monkeypatch):
    """Every model's net replaced by the composition by hand over that net (undone by monkeypatch.undo())."""
    hands = []
    for model in models:
        hands.append(HandCache(pkg, monkeypatch, model.net))
        monkeypatch.setattr(model, "net", hands[-1])
    return hands


@pytest.mark.parametrize("sampler", ("euler", "dpmpp_2m"))
@pytest.mark.parametrize("guidance", (0.0, 2.0))
def test_model_loop(pkg, gpu, pipe, monkeypatch, sampler, guidance):
    model = pipe.pre_loaded_model_instance["inverse"]
    model.vae = StubVAE()
    sw = pkg.synthetic_weights
    rgb = sw.synth_tensor("sc.gpu.rgb", (1, 3, 9, 32, 32), torch.float32, scale=0.6).to(BF).to(gpu)
    noise = sw.synth_tensor("sc.gpu.xT", (1, 16, 2, 4, 4), torch.float32, scale=80.0)
    batch = lambda: {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[0], [3]], dtype=torch.long, device=gpu)}
    kw = dict(guidance=guidance, seed=7, state_shape=[16, 2, 4, 4], num_steps=6, init_noise=noise, sampler=sampler)
    default = model.generate_samples_from_batch(batch(), **kw)
    assert torch.equal(model.generate_samples_from_batch(batch(), step_cache=0.0, **kw), default)
    assert torch.equal(model.generate_samples_from_batch(batch(), step_cache=1e-30, **kw), default)
    assert [c for c, _ in model.net.step_cache_log] == [True] * 6
    got = model.generate_samples_from_batch(batch(), step_cache=1.0, **kw)
    log = list(model.net.step_cache_log)
    assert len(log) == 6 and _rule_holds(log, 3) and not all(c for c, _ in log) and model.net._cache is None
    (hand,) = _by_hand(pkg, [model], monkeypatch)
    want = model.generate_samples_from_batch(batch(), step_cache=1.0, **kw)
    monkeypatch.undo()
    assert torch.equal(got, want) and hand.step_cache_log == log and not torch.equal(got, default)
    assert torch.isfinite(got.float()).all()


@pytest.mark.parametrize("path", ("whole_clip", "windowed", "pixel_tiled", "ensemble"))
def test_pipeline(pkg, gpu, pipe, monkeypatch, path):
    p = pipe
    _reset(p)
    sw = pkg.synthetic_weights
    T = 17 if path == "windowed" else 9
    if path == "windowed":
        p.window_frames, p.window_overlap = 9, 2
    if path == "pixel_tiled":
        p.tile_height, p.tile_width, p.tile_overlap = 32, 32, 8
    if path == "ensemble":
        p.ensemble = 2
    p.guidance, p.num_steps = 1.5, 5
    rgb = sw.synth_tensor(f"sc.gpu.clip{T}", (1, 3, T, H, W), torch.float32, scale=1.0)
    batch = {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[0], [3]], dtype=torch.long)}
    run = lambda: p.generate_video_passes(batch, [False, True], seed=5)
    default = run()
    assert p.last_step_cache == []
    p.step_cache = 1e-30
    tiny = run()
    loops = len(p.last_step_cache)                       # windows, pixel tiles and ensemble members each run their own loop
    assert (loops == 1) if path == "whole_clip" else (loops == 2) if path == "ensemble" else (loops > 1)
    assert all([c for c, _ in log] == [True] * 5 for log in p.last_step_cache)
    p.step_cache = 1.0
    got = run()
    logs = [list(log) for log in p.last_step_cache]
    assert len(logs) == loops and all(len(log) == 5 and _rule_holds(log, 3) and not all(c for c, _ in log) for log in logs)
    _by_hand(pkg, p.pre_loaded_model_instance.values(), monkeypatch)
    want = run()
    assert [list(log) for log in p.last_step_cache] == logs
    monkeypatch.undo()
    p.step_cache = 0.0
    zero = run()
    for d, t, z, g, w in zip(default, tiny, zero, got, want):
        assert d.shape == (1, T, H, W, 3) and np.array_equal(t, d) and np.array_equal(z, d)
        assert np.array_equal(g, w) and not np.array_equal(g, d)
    p.step_cache, p.tile_join = 0.5, "latent"
    with pytest.raises(ValueError, match="latent"):
        run()
    _reset(p)


def test_nodes(pkg, gpu, pipe, monkeypatch):
    p = pipe
    _reset(p)
    sw = pkg.synthetic_weights
    T = 9
    image = sw.synth_tensor("sc.node.img", (1, T, H, W, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("sc.node.env", (1, 32, 64, 3), torch.float32).abs() * 4.0
    inv = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    fwd = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    rel = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()

    def run(**kw):
        kw = dict(seed=3, steps=5, **kw)
        g = inv.run_inverse_pass(p, image, guidance=1.0, **kw)
        assert p.step_cache == kw.get("step_cache", 0.0)
        g5 = [o.reshape(1, T, H, W, 3) for o in g]
        (lit,) = fwd.run_forward_pass(p, g5[4], g5[3], g5[2], g5[1], g5[0], env, guidance=0.0, env_spin=45.0, **kw)
        return [*g, lit, *rel.run_relight(p, p, image, env, env_spin=45.0, **kw)]
    default = run()
    for a, b in zip(run(step_cache=0.0), default):
        assert torch.equal(a, b)
    for a, b in zip(run(step_cache=1e-30), default):
        assert torch.equal(a, b)
    got = run(step_cache=1.0)
    assert _rule_holds(p.last_step_cache[-1], 3) and not all(c for c, _ in p.last_step_cache[-1])
    _by_hand(pkg, p.pre_loaded_model_instance.values(), monkeypatch)
    want = run(step_cache=1.0)
    monkeypatch.undo()
    assert len(got) == 12
    for k, (a, b, d) in enumerate(zip(got, want, default)):
        assert torch.equal(a, b), k
    assert not torch.equal(got[0], default[0]) and not torch.equal(got[5], default[5])
    _reset(p)
