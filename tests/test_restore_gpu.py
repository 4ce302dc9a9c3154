"""drn_restore_frames_u8 (csrc/restore.hip, on csrc/resample_core.h) on the GPU: the kernel against the float64 reference under
the bound of tests/restore_refs.py (whose wrong stand-ins tests/test_restore_cpu.py shows to miss it), bit for bit where the weights
are dyadic, flat frames, every byte alignment of src and dst, scattered column and row taps, its argument checks, the dispatch of
fit.restore_frames, and both renderer nodes with `fit_restore` against the composition done by hand.  Every launch writes into a
guard-banded buffer and is issued twice."""
import pytest
import torch

import restore_refs as R
from conftest import tiny_net
from fit_refs import scattered_rows

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD, SENTINEL = 64, 0xA5
DRN_EINVAL = -1


def _launch(pkg, gpu, src, rplan, dst_off=0):
    """The kernel into a buffer with 64-byte sentinel bands in front and behind (dst_off: further bytes of sentinel in front, to move
    the output's base off its alignment), issued twice (the rerun changes nothing) -> the result on the CPU; the bands are checked
    here."""
    shape = (src.shape[0], rplan.T, rplan.H, rplan.W, 3)
    n = src.shape[0] * rplan.T * rplan.H * rplan.W * 3
    at = GUARD + dst_off
    buf = torch.full((at + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    out = buf[at:at + n].view(shape)
    assert out.data_ptr() % 16 == dst_off % 16
    pkg.native.restore_frames(src, rplan.T, rplan.y_lo_n, rplan.y_w, rplan.x_lo_n, rplan.x_w, out=out)
    first = buf.cpu()
    pkg.native.restore_frames(src, rplan.T, rplan.y_lo_n, rplan.y_w, rplan.x_lo_n, rplan.x_w, out=out)
    host = buf.cpu()
    assert torch.equal(first, host), "a rerun changed the result"
    assert (host[:at] == SENTINEL).all() and (host[at + n:] == SENTINEL).all(), "wrote outside its output"
    return host[at:at + n].view(shape)


def _shifted(t, off, gpu):
    """A copy of t on the GPU whose base address is `off` bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 16, dtype=torch.uint8, device=gpu)
    assert flat.data_ptr() % 16 == 0
    flat[off:off + t.numel()] = t.reshape(-1).to(gpu)
    out = flat[off:off + t.numel()].view(t.shape)
    assert out.data_ptr() % 16 == off % 16 and out.is_contiguous()
    return out


ALL = R.GEOMETRIES + R.EXTRA


@pytest.mark.parametrize("g", ALL, ids=[R.geometry_id(g) for g in ALL])
def test_kernel_meets_the_bound(pkg, gpu, g):
    worst = 0.0
    for _, B, Ts, Td in R.grid([g]):
        c = R.case(pkg, g, B, Ts, Td)
        got = _launch(pkg, gpu, c["src"].to(gpu), c["rplan"])
        ok, ratio = R.bound_excess(got, c["ref64"], c["e_ref"])
        differ = int((got != c["spec"]).sum())
        print(f"restore-frame {c['name']}: E_ref {c['e_ref']:.3e}, max((|hip - ref64| - 0.5)+ / E_ref) = {ratio:.3f}, "
              f"{differ} of {got.numel()} bytes differ from the specification")
        assert ok, (c["name"], ratio)
        worst = max(worst, ratio)
    print(f"restore-frame {R.geometry_id(g)}: worst ratio {worst:.3f} (bound {R.M_BOUND})")


@pytest.mark.parametrize("g", R.DYADIC, ids=[R.geometry_id(g) for g in R.DYADIC])
def test_kernel_is_bit_exact_where_the_weights_are_dyadic(pkg, gpu, g):
    """Round-half-even of ref64, bit for bit, wherever every tap weight is dyadic: everywhere but the x2 shrink's first and last
    row and column (taps of 3/7, 3/7, 1/7 there: tests/test_restore_cpu.py), which are held to the bound."""
    for B in R.BATCHES:
        for Ts, Td in R.TIMES:
            c = R.case(pkg, g, B, Ts, Td)
            got = _launch(pkg, gpu, c["src"].to(gpu), c["rplan"])           # the identity too: launched directly, a copy
            mask = R.dyadic_mask(c["rplan"])[None, None, :, :, None].expand_as(c["ref64"])
            want = R.round_u8(c["ref64"])
            assert torch.equal(got[mask], want[mask]), c["name"]
            assert R.bound_excess(got, c["ref64"], c["e_ref"])[0], c["name"]
            if c["rplan"].identity:
                assert torch.equal(got, c["src"][:, :Td])
            print(f"restore-frame {c['name']}: bit for bit at {int(mask.sum())} of {mask.numel()} bytes, "
                  f"{int((got != want).sum())} of the others differ from round(ref64)")


def test_flat_frames_come_back_flat(pkg, gpu):
    fit = R.fit_module(pkg)
    clip = R.flat_clip()
    r = fit.plan_restore(fit.plan_fit(256, *R.FLAT[1], "stretch", *R.FLAT[0], windowed=True))
    got = _launch(pkg, gpu, clip.to(gpu), r)
    assert got.shape == (1, 256, 27, 40, 3)
    assert torch.equal(got, torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1, 1).expand_as(got))


@pytest.mark.parametrize("off", [1, 2, 3, 5])
def test_kernel_bases_off_a_16_byte_boundary(pkg, gpu, off):
    for g in (R.GEOMETRIES[0], R.GEOMETRIES[2], R.GEOMETRIES[4]):
        c = R.case(pkg, g, 2, 3, 2)
        aligned = _launch(pkg, gpu, c["src"].to(gpu), c["rplan"])
        assert torch.equal(_launch(pkg, gpu, _shifted(c["src"], off, gpu), c["rplan"]), aligned), (c["name"], "src")
        assert torch.equal(_launch(pkg, gpu, c["src"].to(gpu), c["rplan"], dst_off=off), aligned), (c["name"], "dst")
        assert torch.equal(_launch(pkg, gpu, _shifted(c["src"], off, gpu), c["rplan"], dst_off=4 - off % 4), aligned), c["name"]


def _raw_call(lib, a):
    return lib.drn_restore_frames_u8(a["src"], a["dst"], a["B"], a["Ts"], a["Hs"], a["Ws"], a["Td"], a["Hd"], a["Wd"],
                                     a["y_lo_n"], a["y_w"], a["Ky"], a["x_lo_n"], a["x_w"], a["Kx"],
                                     torch.cuda.current_stream().cuda_stream)


def test_scattered_taps_read_the_source_directly(pkg, gpu):
    """Column taps at both ends of a 3000-pixel row: the 9000 bytes they span do not fit the kernel's raw buffer, so it reads
    the source directly.  No resize produces such a table; the result is still the table's."""
    Hs, Ws, Hd, Wd = 2, 3000, 3, 8
    src = R.source(1, 1, Hs, Ws, seed=77)
    x_lo_n = torch.tensor([[0, 2], [2998, 2], [5, 2], [2990, 1], [1500, 2], [2998, 2], [0, 1], [7, 2]], dtype=torch.int32)
    x_w = torch.tensor([[0.25, 0.75]] * 8, dtype=torch.float32)
    x_w[x_lo_n[:, 1] == 1] = torch.tensor([1.0, 0.0])
    y_lo_n = torch.tensor([[0, 2], [0, 1], [1, 1]], dtype=torch.int32)
    y_w = torch.tensor([[0.5, 0.5], [1.0, 0.0], [1.0, 0.0]], dtype=torch.float32)
    want = R.round_u8(R.apply64(src, R.dense(y_lo_n, y_w, Hs), R.dense(x_lo_n, x_w, Ws), 1))      # dyadic: exact
    n = Hd * Wd * 3
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    out = buf[GUARD:GUARD + n].view(1, 1, Hd, Wd, 3)
    for _ in range(2):
        pkg.native.restore_frames(src.to(gpu), 1, y_lo_n, y_w, x_lo_n, x_w, out=out)
    host = buf.cpu()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all()
    assert torch.equal(host[GUARD:GUARD + n].view(1, 1, Hd, Wd, 3), want)


def test_scattered_row_taps_cut_a_tile_into_one_chunk_per_row(pkg, gpu):
    """No grid case has a tile whose source rows overflow the stage (its 32 rows at most).  Here no two consecutive output rows
    fit it together (fit_refs.scattered_rows): the 16-row tile is 16 chunks.  Dyadic weights: exact, ties real, bit for bit."""
    rplan, my, mx = scattered_rows()
    rplan.T, rplan.H, rplan.W = 2, 16, 32
    src = R.source(2, 3, 120, 40, seed=78)
    got = _launch(pkg, gpu, src.to(gpu), rplan)
    assert torch.equal(got, R.round_u8(R.apply64(src, my, mx, 2)))


def test_kernel_argument_checks(pkg, gpu):
    lib = pkg.native.load_library()
    c = R.case(pkg, R.GEOMETRIES[0], 1, 3, 2)
    p = c["rplan"]
    src = c["src"].to(gpu)
    tabs = [t.to(gpu) for t in (p.y_lo_n, p.y_w, p.x_lo_n, p.x_w)]
    n = p.T * p.H * p.W * 3
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    out = buf[GUARD:].data_ptr()
    base = dict(src=src.data_ptr(), dst=out, B=1, Ts=3, Hs=p.H_model, Ws=p.W_model, Td=p.T, Hd=p.H, Wd=p.W,
                y_lo_n=tabs[0].data_ptr(), y_w=tabs[1].data_ptr(), Ky=p.y_w.shape[1],
                x_lo_n=tabs[2].data_ptr(), x_w=tabs[3].data_ptr(), Kx=p.x_w.shape[1])
    bad = {f"null {k}": {k: None} for k in ("src", "dst", "y_lo_n", "y_w", "x_lo_n", "x_w")}
    bad.update({f"{k} = 0": {k: 0} for k in ("B", "Ts", "Hs", "Ws", "Td", "Hd", "Wd")})
    bad.update({"B < 0": dict(B=-1), "Td > Ts": dict(Td=4), "Ky = 0": dict(Ky=0), "Ky = 33": dict(Ky=33), "Kx = 0": dict(Kx=0),
                "Kx = 33": dict(Kx=33),
                "output of 2^31 bytes": dict(B=1 << 12, Ts=1 << 8, Td=1 << 8, Hd=1 << 8, Wd=1 << 4, Hs=1, Ws=1),     # 3 * 2^32
                "source of 2^31 bytes": dict(B=1 << 12, Ts=1 << 8, Hs=1 << 8, Ws=1 << 4, Td=1, Hd=1, Wd=1),
                "y_lo_n 2 bytes off": dict(y_lo_n=tabs[0].data_ptr() + 2), "y_w 1 byte off": dict(y_w=tabs[1].data_ptr() + 1),
                "x_lo_n 1 byte off": dict(x_lo_n=tabs[2].data_ptr() + 1), "x_w 2 bytes off": dict(x_w=tabs[3].data_ptr() + 2)})
    for name, kw in bad.items():
        assert _raw_call(lib, dict(base, **kw)) == DRN_EINVAL, name
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all(), "a rejected call wrote"
    assert _raw_call(lib, base) == 0
    host = buf.cpu()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all()
    assert R.bound_excess(host[GUARD:GUARD + n].view(1, p.T, p.H, p.W, 3), c["ref64"], c["e_ref"])[0]
    # the wrapper reads the tables where their contents can be read
    for name in ("y_lo_n", "x_lo_n"):
        kw = dict(y_lo_n=p.y_lo_n, y_w=p.y_w, x_lo_n=p.x_lo_n, x_w=p.x_w)
        kw[name] = kw[name].clone()
        kw[name][-1, 0] += 40
        with pytest.raises(AssertionError, match="taps outside the source"):
            pkg.native.restore_frames(src, p.T, **kw)
    with pytest.raises(AssertionError, match="frames to return outside the clip"):
        pkg.native.restore_frames(src, 4, p.y_lo_n, p.y_w, p.x_lo_n, p.x_w)


def test_restore_frames_dispatch(pkg, gpu, monkeypatch):
    fit = R.fit_module(pkg)
    c = R.case(pkg, R.GEOMETRIES[1], 2, 3, 2)
    src = c["src"].to(gpu)
    with pytest.raises(ValueError, match="needs a GPU tensor"):
        fit.restore_frames(c["src"], c["rplan"], backend="hip")
    hip = fit.restore_frames(src, c["rplan"], backend="hip")
    assert hip.is_cuda and hip.dtype == torch.uint8 and hip.shape == (2, 2, 37, 23, 3)
    assert R.bound_excess(hip.cpu(), c["ref64"], c["e_ref"])[0]
    assert torch.equal(fit.restore_frames(src, c["rplan"]), hip)                      # auto = the kernel on a GPU tensor
    assert torch.equal(fit.restore_frames(src, c["rplan"], backend="torch").cpu(), c["spec"])      # the specification, on the device
    # an identity plan launches nothing and returns the cut input
    calls = []
    monkeypatch.setattr(pkg.native, "restore_frames", lambda *a, **k: calls.append(a))
    ident = R.restore_plan(pkg, R.DYADIC[3], 2)
    u8 = R.source(1, 3, 16, 32).to(gpu)
    for backend in ("auto", "hip", "torch"):
        out = fit.restore_frames(u8, ident, backend=backend)
        assert out.shape == (1, 2, 16, 32, 3) and out.data_ptr() == u8.data_ptr() and torch.equal(out, u8[:, :2])
    assert not calls


# ----------------------------------------------------------------------------------------------- nodes
def _pipeline(pkg, gpu, forward=False):
    sw = pkg.synthetic_weights
    net = tiny_net(pkg, 256, 1, 2, forward=True) if forward else tiny_net(pkg, 256, 1, 2)
    C = pkg.diffusion_renderer_config
    cfg = C.get_forward_renderer_config() if forward else C.get_inverse_renderer_config()
    cfg["net"] = dict(net)
    if forward:
        cfg["model_type"] = "forward"
    model = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=gpu)
    model.load_state_dict(sw.synth_state_dict(net, BF, device=gpu), strict=True)
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=gpu), device=gpu)
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=vae, model_instance={"forward": model} if forward else model,
        guidance=0.0, num_steps=2)
    p.device = gpu
    return p


def _by_hand(pkg, gpu, image, T, H, W):
    """A node output at the model's size ([T, 32, 32, 3] or [1, T, 32, 32, 3] floats, exact multiples of 1 / 255) through
    restore_frames by hand."""
    fit = R.fit_module(pkg)
    u8 = (image.reshape(1, T, 32, 32, 3) * 255.0).round().to(torch.uint8)
    assert torch.equal(u8.float() / 255.0, image.reshape(1, T, 32, 32, 3))
    r = fit.plan_restore(fit.plan_fit(T, H, W, "stretch", windowed=True))
    assert (r.T, r.H_model, r.W_model, r.H, r.W) == (T, 32, 32, H, W)
    return fit.restore_frames(u8.to(gpu), r, backend="hip").cpu().float() / 255.0


def test_inverse_node_with_fit_restore(pkg, gpu):
    p = _pipeline(pkg, gpu)
    assert p.restore_plan is None
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    image = R.source(1, 10, 40, 36).float() / 255.0
    outs = node.run_inverse_pass(p, image, guidance=0.0, seed=3, fit="stretch", fit_restore=True)
    assert p.restore_plan is not None and len(outs) == 5
    small = node.run_inverse_pass(p, image, guidance=0.0, seed=3, fit="stretch", fit_restore=False)
    assert p.restore_plan is None                                                  # cleared by a call with restore off
    for o, s in zip(outs, small):
        assert o.shape == (10, 40, 36, 3) and s.shape == (10, 32, 32, 3) and o.dtype == torch.float32
        assert torch.equal(o, _by_hand(pkg, gpu, s, 10, 40, 36)[0])
    assert not torch.equal(outs[0], outs[3])
    # the passes one after the other (generate_video) instead of batched
    p.batch_passes = False
    each = node.run_inverse_pass(p, image, guidance=0.0, seed=3, fit="stretch", fit_restore=True)
    small_each = node.run_inverse_pass(p, image, guidance=0.0, seed=3, fit="stretch")
    for o, s in zip(each, small_each):
        assert torch.equal(o, _by_hand(pkg, gpu, s, 10, 40, 36)[0])
    p.batch_passes = True
    with pytest.raises(ValueError, match="crop cannot be undone"):
        node.run_inverse_pass(p, image, guidance=0.0, seed=3, fit="crop", fit_restore=True)
    assert p.restore_plan is None


def test_inverse_node_with_fit_restore_in_windows(pkg, gpu):
    p = _pipeline(pkg, gpu)
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    clip = R.source(1, 21, 40, 36, seed=1).float() / 255.0
    kw = dict(guidance=0.0, seed=3, window_frames=9, window_overlap=2, fit="stretch")
    assert len(pkg.windows.plan_windows(21, 9, 2)) == 3
    outs = node.run_inverse_pass(p, clip, fit_restore=True, **kw)
    small = node.run_inverse_pass(p, clip, **kw)
    for o, s in zip(outs, small):
        assert o.shape == (21, 40, 36, 3) and s.shape == (21, 32, 32, 3)
        assert torch.equal(o, _by_hand(pkg, gpu, s, 21, 40, 36)[0])               # window by window = the whole clip
    p.batch_passes = False                                                         # generate_video_each: windows outside
    each = node.run_inverse_pass(p, clip, fit_restore=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(each, outs))


def test_forward_node_with_fit_restore(pkg, gpu):
    p = _pipeline(pkg, gpu, forward=True)
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    names = ("depth", "normal", "roughness", "metallic", "base_color")
    g = {k: R.source(1, 10, 40, 36, seed=i).float() / 255.0 for i, k in enumerate(names)}
    env = pkg.synthetic_weights.synth_tensor("restorefw.env", (1, 32, 64, 3), torch.float32).abs() * 4.0

    def run(**kw):
        return node.run_forward_pass(p, *(g[k] for k in names), env, guidance=0.0, seed=5, env_format="proj", env_rotation=180.0,
                                     env_spin=90.0, fit="stretch", **kw)[0]
    out = run(fit_restore=True)
    assert p.restore_plan is not None
    small = run()
    assert p.restore_plan is None
    assert out.shape == (1, 10, 40, 36, 3) and small.shape == (1, 10, 32, 32, 3)
    assert torch.equal(out, _by_hand(pkg, gpu, small, 10, 40, 36))
