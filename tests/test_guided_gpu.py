"""drn_restore_guided_u8 (csrc/restore_guided.hip, on csrc/resample_core.h) on the GPU: the kernel against the float64 reference
under the bound of tests/guided_refs.py (whose wrong stand-ins tests/test_guided_cpu.py shows to miss it) at the issue's geometries
x batch x guide batch x time, the sweep, fallback and flat cases, every byte alignment of the four tensors, scattered taps, its
argument checks, the dispatch of fit.restore_frames_guided, the pipeline whole, windowed and tiled, and the inverse and relight nodes
with `restore_guide = "source"` against the composition done by hand.  Every launch writes into a guard-banded buffer and is issued
twice."""
import dataclasses
import itertools

import pytest
import torch

import guided_refs as G
import restore_refs as R
from test_relight_gpu import pipe          # noqa: F401  (the fixture: one pipeline that holds both renderers)
from test_restore_gpu import GUARD, SENTINEL, _pipeline, _shifted

pytestmark = pytest.mark.gpu
DRN_EINVAL = -1


def _launch(pkg, gpu, src, p, hi, lo, t0=0, dst_off=0):
    """The kernel into a buffer with 64-byte sentinel bands in front and behind (dst_off: further bytes of sentinel in front, to
    move the output's base off its alignment), issued twice (the rerun changes nothing) -> the result on the CPU; the bands are
    checked here."""
    shape = (src.shape[0], p.T, p.H, p.W, 3)
    n = src.shape[0] * p.T * p.H * p.W * 3
    at = GUARD + dst_off
    buf = torch.full((at + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    out = buf[at:at + n].view(shape)
    assert out.data_ptr() % 16 == dst_off % 16
    args = (src, lo, hi, p.T, p.y_lo_n, p.y_w, p.x_lo_n, p.x_w, p.tab, p.eps)
    pkg.native.restore_guided(*args, t0=t0, out=out)
    first = buf.cpu()
    pkg.native.restore_guided(*args, t0=t0, out=out)
    host = buf.cpu()
    assert torch.equal(first, host), "a rerun changed the result"
    assert (host[:at] == SENTINEL).all() and (host[at + n:] == SENTINEL).all(), "wrote outside its output"
    return host[at:at + n].view(shape)


def _check(pkg, gpu, c):
    got = _launch(pkg, gpu, c["src"].to(gpu), c["gplan"], c["hi"].to(gpu), c["lo"].to(gpu), c["t0"])
    ok, ratio = G.bound_excess(got, c["ref64"], c["e_ref"])
    differ = int((got != c["spec"]).sum())
    print(f"guided-frame {c['name']}: E_ref {c['e_ref']:.3e}, max((|hip - ref64| - 0.5)+ / E_ref) = {ratio:.3f} of {G.M_BOUND} "
          f"({100.0 * ratio / G.M_BOUND:.1f} % of the allowance), {differ} of {got.numel()} bytes differ from the specification")
    assert ok, (c["name"], ratio)
    return got


@pytest.mark.parametrize("g", G.GEOMETRIES, ids=[G.geometry_id(g) for g in G.GEOMETRIES])
def test_kernel_meets_the_bound(pkg, gpu, g):
    for key in G.grid([g]):
        _check(pkg, gpu, G.case(pkg, *key))


@pytest.mark.parametrize("name", list(G.NAMED))
def test_named_cases(pkg, gpu, name):
    _check(pkg, gpu, G.NAMED[name](pkg))


def test_flat_frames_come_back_flat(pkg, gpu):
    src, gplan, hi, lo = G.flat_case(pkg)
    got = _launch(pkg, gpu, src.to(gpu), gplan, hi.to(gpu), lo.to(gpu))
    assert got.shape == (1, 256, 27, 40, 3)
    assert torch.equal(got, torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1, 1).expand_as(got))


def test_every_byte_alignment_of_the_four_tensors(pkg, gpu):
    """src, guide_lo, guide_hi and dst each at byte offsets 0..3 past a 16-byte boundary, all 256 combinations, at 183-byte output
    rows and 48-byte source rows: the same bytes as the aligned launch."""
    c = G.case(pkg, G.GEOMETRIES[2], 2, 2, 3, 2, 5, 2)
    aligned = _check(pkg, gpu, c)
    moved = {name: [_shifted(c[name], off, gpu) for off in range(4)] for name in ("src", "hi", "lo")}
    for a, b, d, e in itertools.product(range(4), repeat=4):
        got = _launch(pkg, gpu, moved["src"][a], c["gplan"], moved["hi"][b], moved["lo"][d], c["t0"], dst_off=e)
        assert torch.equal(got, aligned), (a, b, d, e)


def _hand_tables():
    """Tables no resize produces, dyadic weights: column taps at both ends of a 3600-pixel row (10800 bytes: more than a raw
    buffer holds, the kernel reads the sources directly) and 8 row taps."""
    x_lo_n = torch.tensor([[0, 2], [3598, 2], [5, 2], [3590, 1], [1500, 2], [3598, 2], [0, 1], [7, 2]], dtype=torch.int32)
    x_w = torch.tensor([[0.25, 0.75]] * 8, dtype=torch.float32)
    x_w[x_lo_n[:, 1] == 1] = torch.tensor([1.0, 0.0])
    y_lo_n = torch.tensor([[0, 8], [1, 1], [0, 2]], dtype=torch.int32)
    y_w = torch.zeros(3, 8)
    y_w[0], y_w[1, 0], y_w[2, :2] = 0.125, 1.0, 0.5
    return y_lo_n, y_w, x_lo_n, x_w


def test_scattered_taps_read_the_sources_directly(pkg, gpu):
    fit = G.fit_module(pkg)
    y_lo_n, y_w, x_lo_n, x_w = _hand_tables()
    Hs, Ws, Hd, Wd = 8, 3600, 3, 8
    p = fit.GuidedPlan(1, Hs, Ws, Hd, Wd, y_lo_n, y_w, x_lo_n, x_w, fit.range_table(40.0), fit.GUIDED_EPS, 40.0)
    src, lo, hi = R.source(1, 1, Hs, Ws, seed=81), R.source(1, 1, Hs, Ws, seed=82), R.source(1, 1, Hd, Wd, seed=83)
    lo[0, 0, :, :8] = hi[0, 0, 0]                                               # some taps that resemble the guide
    ref64 = G.reference64(src, p, hi, lo)
    e_ref = float((fit._restore_guided_torch(src, p, hi, lo, rounded=False).double() - ref64).abs().max())
    got = _launch(pkg, gpu, src.to(gpu), p, hi.to(gpu), lo.to(gpu))
    ok, ratio = G.bound_excess(got, ref64, e_ref)
    print(f"guided-frame scattered: E_ref {e_ref:.3e}, ratio {ratio:.3f}")
    assert ok


def test_row_taps_cut_a_tile_into_chunks(pkg, gpu):
    """Row taps far apart on 1698-byte spans: a raw buffer holds three source rows, so the 16-row tile is cut into chunks."""
    fit = G.fit_module(pkg)
    Hs, Ws, Hd, Wd = 40, 600, 16, 64
    x_lo_n = torch.stack([torch.arange(64, dtype=torch.int32) * 17 % 500, torch.full((64,), 2, dtype=torch.int32)], dim=1)
    x_lo_n[0, 0], x_lo_n[1, 0] = 0, 564                                         # the span: 566 pixels
    x_w = torch.tensor([[0.375, 0.625]] * 64, dtype=torch.float32)
    y_lo_n = torch.stack([torch.arange(16, dtype=torch.int32) * 7 % 38, torch.full((16,), 2, dtype=torch.int32)], dim=1)
    y_w = torch.tensor([[0.5, 0.5]] * 16, dtype=torch.float32)
    p = fit.GuidedPlan(2, Hs, Ws, Hd, Wd, y_lo_n, y_w, x_lo_n, x_w, fit.range_table(40.0), fit.GUIDED_EPS, 40.0)
    src, lo, hi = R.source(2, 2, Hs, Ws, seed=84), R.source(1, 3, Hs, Ws, seed=85), R.source(1, 3, Hd, Wd, seed=86)
    ref64 = G.reference64(src, p, hi, lo, 1)
    e_ref = float((fit._restore_guided_torch(src, p, hi, lo, 1, rounded=False).double() - ref64).abs().max())
    got = _launch(pkg, gpu, src.to(gpu), p, hi.to(gpu), lo.to(gpu), t0=1)
    ok, ratio = G.bound_excess(got, ref64, e_ref)
    print(f"guided-frame chunks: E_ref {e_ref:.3e}, ratio {ratio:.3f}")
    assert ok


def _raw_call(lib, a):
    return lib.drn_restore_guided_u8(a["src"], a["guide_lo"], a["guide_hi"], a["dst"], a["B"], a["Bg"], a["Ts"], a["Hs"], a["Ws"],
                                     a["Tg"], a["t0"], a["Td"], a["Hd"], a["Wd"], a["y_lo_n"], a["y_w"], a["Ky"], a["x_lo_n"],
                                     a["x_w"], a["Kx"], a["range_tab"], a["eps"], torch.cuda.current_stream().cuda_stream)


def test_kernel_argument_checks(pkg, gpu):
    lib = pkg.native.load_library()
    c = G.case(pkg, G.GEOMETRIES[0], 2, 2, 3, 2, 5, 2)
    p = c["gplan"]
    src, hi, lo = (c[k].to(gpu) for k in ("src", "hi", "lo"))
    tabs = [t.to(gpu) for t in (p.y_lo_n, p.y_w, p.x_lo_n, p.x_w, p.tab)]
    n = 2 * p.T * p.H * p.W * 3
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    base = dict(src=src.data_ptr(), guide_lo=lo.data_ptr(), guide_hi=hi.data_ptr(), dst=buf[GUARD:].data_ptr(), B=2, Bg=2, Ts=3,
                Hs=p.H_model, Ws=p.W_model, Tg=5, t0=2, Td=2, Hd=p.H, Wd=p.W, y_lo_n=tabs[0].data_ptr(), y_w=tabs[1].data_ptr(),
                Ky=p.y_w.shape[1], x_lo_n=tabs[2].data_ptr(), x_w=tabs[3].data_ptr(), Kx=p.x_w.shape[1],
                range_tab=tabs[4].data_ptr(), eps=p.eps)
    bad = {f"null {k}": {k: None} for k in ("src", "guide_lo", "guide_hi", "dst", "y_lo_n", "y_w", "x_lo_n", "x_w", "range_tab")}
    bad.update({f"{k} = 0": {k: 0} for k in ("B", "Bg", "Ts", "Hs", "Ws", "Tg", "Td", "Hd", "Wd")})
    big = dict(B=1, Bg=1, Ts=1, Tg=1, Td=1, t0=0, Hs=1, Ws=1, Hd=1, Wd=1)
    bad.update({"B < 0": dict(B=-1), "Bg = 3": dict(Bg=3), "Bg = B + 1 with B = 1": dict(B=1, Bg=2), "Td > Ts": dict(Td=4, Tg=9),
                "t0 < 0": dict(t0=-1), "t0 + Td > Tg": dict(t0=4), "t0 + Td overflows": dict(t0=2 ** 31 - 1),
                "Ky = 0": dict(Ky=0), "Ky = 9": dict(Ky=9), "Kx = 0": dict(Kx=0), "Kx = 9": dict(Kx=9),
                "src of 2^31 bytes": dict(big, B=1 << 12, Ts=1 << 8, Hs=1 << 8, Ws=1 << 4),          # 3 * 2^32
                "guide_lo of 2^31 bytes": dict(big, Tg=1 << 20, Hs=1 << 8, Ws=1 << 4),
                "guide_hi of 2^31 bytes": dict(big, Tg=1 << 20, Hd=1 << 8, Wd=1 << 4),
                "dst of 2^31 bytes": dict(big, B=1 << 12, Ts=1 << 8, Tg=1 << 8, Td=1 << 8, Hd=1 << 8, Wd=1 << 4),
                "sizes whose product wraps": dict(big, B=2 ** 31 - 1, Ts=2 ** 31 - 1, Hs=2 ** 31 - 1, Ws=2 ** 31 - 1),
                "y_lo_n 2 bytes off": dict(y_lo_n=tabs[0].data_ptr() + 2), "y_w 1 byte off": dict(y_w=tabs[1].data_ptr() + 1),
                "x_lo_n 1 byte off": dict(x_lo_n=tabs[2].data_ptr() + 1), "x_w 2 bytes off": dict(x_w=tabs[3].data_ptr() + 2),
                "range_tab 2 bytes off": dict(range_tab=tabs[4].data_ptr() + 2),
                "eps = 0": dict(eps=0.0), "eps < 0": dict(eps=-1.0), "eps NaN": dict(eps=float("nan"))})
    for name, kw in bad.items():
        assert _raw_call(lib, dict(base, **kw)) == DRN_EINVAL, name
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all(), "a rejected call wrote"
    assert _raw_call(lib, base) == 0
    host = buf.cpu()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all()
    assert G.bound_excess(host[GUARD:GUARD + n].view(2, p.T, p.H, p.W, 3), c["ref64"], c["e_ref"])[0]
    # the wrapper reads the tables where their contents can be read
    good = dict(y_lo_n=p.y_lo_n, y_w=p.y_w, x_lo_n=p.x_lo_n, x_w=p.x_w)
    for name in ("y_lo_n", "x_lo_n"):
        kw = dict(good, **{name: good[name].clone()})
        kw[name][-1, 0] += 40
        with pytest.raises(AssertionError, match="taps outside the source"):
            pkg.native.restore_guided(src, lo, hi, p.T, range_tab=p.tab, eps=p.eps, t0=2, **kw)
    with pytest.raises(AssertionError, match="at most 8 taps"):
        pkg.native.restore_guided(src, lo, hi, p.T, range_tab=p.tab, eps=p.eps, t0=2,
                                  **dict(good, y_w=torch.cat([p.y_w, torch.zeros(p.H, 5)], dim=1)))
    with pytest.raises(AssertionError, match="outside the clip or the guide"):
        pkg.native.restore_guided(src, lo, hi, p.T, range_tab=p.tab, eps=p.eps, t0=4, **good)
    with pytest.raises(AssertionError, match="guide shapes"):
        pkg.native.restore_guided(src, lo[:, :4].contiguous(), hi, p.T, range_tab=p.tab, eps=p.eps, t0=2, **good)


def test_restore_frames_guided_dispatch(pkg, gpu):
    fit = G.fit_module(pkg)
    c = G.case(pkg, G.GEOMETRIES[1], 2, 1, 3, 2, 5, 2)
    src, hi, lo = (c[k].to(gpu) for k in ("src", "hi", "lo"))
    with pytest.raises(ValueError, match="needs a GPU tensor"):
        fit.restore_frames_guided(c["src"], c["gplan"], c["hi"], c["lo"], 2, backend="hip")
    with pytest.raises(ValueError, match="the frames on"):
        fit.restore_frames_guided(src, c["gplan"], c["hi"], lo, 2)
    hip = fit.restore_frames_guided(src, c["gplan"], hi, lo, 2, backend="hip")
    assert hip.is_cuda and hip.dtype == torch.uint8 and hip.shape == (2, 2, 37, 23, 3)
    assert G.bound_excess(hip.cpu(), c["ref64"], c["e_ref"])[0]
    assert torch.equal(fit.restore_frames_guided(src, c["gplan"], hi, lo, 2), hip)                 # auto = the kernel on a GPU tensor
    on_device = fit.restore_frames_guided(src, c["gplan"], hi, lo, 2, backend="torch")             # the specification, on the device
    assert on_device.is_cuda and G.bound_excess(on_device.cpu(), c["ref64"], c["e_ref"])[0]
    assert torch.equal(fit.restore_frames_guided(c["src"], c["gplan"], c["hi"], c["lo"], 2), c["spec"])    # auto on the CPU


# ----------------------------------------------------------------------------------------------- pipeline and nodes
def _guide(pkg, gpu, image, sigma=12.0, **fit_kw):
    fit = G.fit_module(pkg)
    T, H, W = image.shape[1:4]
    plan = fit.plan_fit(T, H, W, "stretch", **fit_kw)
    return plan, fit.source_guide(plan, image, sigma, gpu)


def _picture(pkg, T, H, W, seed):
    """A uint8 clip [1, T, H, W, 3] of palette regions: a guide whose range term matters."""
    fit = G.fit_module(pkg)
    return G.scene(pkg, fit.plan_fit(T, H, W, "stretch", windowed=True), 1, T, seed=seed)[0]


def _by_hand(pkg, guide, small):
    """Outputs at the model's size (floats, exact multiples of 1 / 255, any leading shape) through the guided way back by hand."""
    fit = G.fit_module(pkg)
    p = guide.plan
    s5 = small.reshape(1, -1, p.H_model, p.W_model, 3)
    u8 = (s5 * 255.0).round().to(torch.uint8)
    assert torch.equal(u8.float() / 255.0, s5)
    plan = dataclasses.replace(p, T=u8.shape[1])
    return fit.restore_frames_guided(u8.to(guide.hi.device), plan, guide.hi, guide.lo, backend="hip").cpu().float() / 255.0


@pytest.mark.parametrize("how", ("whole", "windowed", "tiled"))
def test_generate_video_with_a_guide(pkg, gpu, how):
    """generate_video on tiny nets with restore_plan and restore_guide set against the unrestored outputs brought back by hand:
    a whole clip (time padding cut), windows (the guide read at each window's place), tiles (restored once, on the joined canvas)."""
    fit = G.fit_module(pkg)
    p = _pipeline(pkg, gpu)
    p.set_model_type("inverse")
    T, (H, W) = {"whole": 5, "windowed": 21, "tiled": 9}[how], ((40, 36) if how != "tiled" else (40, 70))
    image = _picture(pkg, T, H, W, seed=11)
    if how == "windowed":
        p.window_frames, p.window_overlap = 9, 2
    if how == "tiled":
        p.tile_height, p.tile_width, p.tile_overlap = 32, 48, 16
    plan = fit.plan_fit(T, H, W, "stretch", windowed=how == "windowed")
    guide = fit.source_guide(plan, image, 12.0, gpu)
    clip = fit.fit_frames(image, plan, device=gpu)
    batch = {"rgb": clip, "video": clip, "context_index": torch.full((1, 1), 3, dtype=torch.long)}
    small = torch.from_numpy(p.generate_video(batch, seed=3))
    assert small.shape == (1, plan.T_out, plan.H_out, plan.W_out, 3)
    p.restore_plan, p.restore_guide = fit.plan_restore(plan), guide
    got = torch.from_numpy(p.generate_video(batch, seed=3))
    want = fit.restore_frames_guided(small[:, :T].to(gpu), guide.plan, guide.hi, guide.lo, backend="hip").cpu()
    assert got.shape == (1, T, H, W, 3) and torch.equal(got, want)
    p.restore_guide = None
    plain = torch.from_numpy(p.generate_video(batch, seed=3))
    assert torch.equal(plain, fit.restore_frames(small.to(gpu), p.restore_plan).cpu()) and not torch.equal(plain, got)


@pytest.mark.parametrize("as_bytes", (True, False), ids=("uint8", "fp32"))
def test_inverse_node_with_a_guide(pkg, gpu, as_bytes):
    p = _pipeline(pkg, gpu)
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    u8 = _picture(pkg, 10, 40, 36, seed=12)
    image = u8 if as_bytes else u8.float() / 255.0
    kw = dict(guidance=0.0, seed=3, fit="stretch")
    outs = node.run_inverse_pass(p, image, fit_restore=True, restore_guide="source", restore_sigma=16.0, **kw)
    assert p.restore_guide is not None and torch.equal(p.restore_guide.hi.cpu(), u8) and len(outs) == 5
    small = node.run_inverse_pass(p, image, **kw)
    assert p.restore_guide is None and p.restore_plan is None                      # cleared by a call without it
    _, guide = _guide(pkg, gpu, u8, 16.0)
    for o, s in zip(outs, small):
        assert o.shape == (10, 40, 36, 3) and s.shape == (10, 32, 32, 3)
        assert torch.equal(o, _by_hand(pkg, guide, s)[0])
    plain = node.run_inverse_pass(p, image, fit_restore=True, **kw)
    assert p.restore_guide is None and not torch.equal(plain[0], outs[0])
    if as_bytes:                                                                   # windows, passes one after the other
        clip = _picture(pkg, 21, 40, 36, seed=13)
        win = dict(kw, window_frames=9, window_overlap=2)
        p.batch_passes = False
        outs = node.run_inverse_pass(p, clip, fit_restore=True, restore_guide="source", **win)
        small = node.run_inverse_pass(p, clip, **win)
        _, guide = _guide(pkg, gpu, clip)
        for o, s in zip(outs, small):
            assert o.shape == (21, 40, 36, 3) and torch.equal(o, _by_hand(pkg, guide, s)[0])


@pytest.mark.parametrize("as_bytes", (True, False), ids=("uint8", "fp32"))
def test_relight_node_with_a_guide(pkg, gpu, pipe, as_bytes):          # noqa: F811
    inv = fwd = pipe
    node = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    u8 = _picture(pkg, 10, 40, 36, seed=14)
    image = u8 if as_bytes else u8.float() / 255.0
    env = pkg.synthetic_weights.synth_tensor("guided.env", (1, 32, 64, 3), torch.float32).abs() * 4.0
    kw = dict(guidance=0.0, seed=3, env_format="proj", env_rotation=180.0, env_spin=90.0, fit="stretch")
    got = node.run_relight(inv, fwd, image, env, fit_restore=True, restore_guide="source", **kw)
    small = node.run_relight(inv, fwd, image, env, **kw)
    assert inv.restore_guide is None and fwd.restore_guide is None
    _, guide = _guide(pkg, gpu, u8)
    assert got[0].shape == (1, 10, 40, 36, 3) and small[0].shape == (1, 10, 32, 32, 3)
    for a, s in zip(got, small):
        assert torch.equal(a.reshape(1, 10, 40, 36, 3), _by_hand(pkg, guide, s))
