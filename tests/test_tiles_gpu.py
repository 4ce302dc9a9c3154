"""Spatial tiles on the GPU: drn_tile_blend_u8 bit for bit against tests/tile_refs.py (whose inputs tests/test_tiles_cpu.py shows
to separate the wrong kernels), its argument checks, and the tiled pipeline and nodes against the composition done by hand.

The kernel works in place, so the canvas lives inside guard bands and the WHOLE canvas is compared: bytes outside the written
rectangle must keep what they held.  Frame bases beyond 32 bits are NOT tested: that needs a canvas of more than 2 GiB."""
import importlib

import numpy as np
import pytest
import torch

import tile_refs as R
from conftest import tiny_net
from stub_vae import StubVAE

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD, SENTINEL = 64, 0xA5
DRN_EINVAL = -1


def _tiles(pkg):
    return importlib.import_module(pkg.__name__ + ".tiles")


def _banded(gpu, a, off=0):
    """The bytes of `a` on the GPU, `off` bytes past a 64-byte guard band and in front of another -> (buffer, view, start)."""
    n = a.size
    buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    view = buf[GUARD + off:GUARD + off + n].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return buf, view, GUARD + off


def _launch(pkg, gpu, canvas, tile, geo, frames, c_off=0, t_off=0):
    """The kernel on a guard-banded canvas (and a tile at its own byte offset), issued twice with the canvas refilled in between:
    both results must agree -> the whole canvas on the CPU; the guard bands are checked here."""
    y_at, x_at, ry, rx, Oy, Ox = geo
    shape5 = lambda a: (*frames, *a.shape[1:])
    tbuf, tview, _ = _banded(gpu, tile, t_off)
    wy = torch.from_numpy(pkg.windows.ramp_weights(Oy)).to(gpu) if Oy else None
    wx = torch.from_numpy(pkg.windows.ramp_weights(Ox)).to(gpu) if Ox else None
    runs = []
    for _ in range(2):
        cbuf, cview, at = _banded(gpu, canvas, c_off)
        assert cview.data_ptr() % 4 == c_off % 4 and tview.data_ptr() % 4 == t_off % 4
        pkg.native.tile_blend_u8(cview.view(shape5(canvas)), tview.view(shape5(tile)), wy, wx, y_at, x_at, ry, rx)
        runs.append(cbuf.cpu())
    assert torch.equal(runs[0], runs[1]), "two launches of one case disagree"
    host = runs[0]
    assert (host[:at] == SENTINEL).all() and (host[at + canvas.size:] == SENTINEL).all(), "wrote outside the canvas"
    assert (tbuf.cpu()[GUARD + t_off:GUARD + t_off + tile.size].view(tile.shape) == torch.from_numpy(tile)).all()
    return host[at:at + canvas.size].view(canvas.shape).numpy()


@pytest.mark.parametrize("W", R.WIDTHS)
def test_tile_kernel_geometry_grid_bit_exact(pkg, gpu, W):
    cases = R.geometry_cases(W)
    for i, case in enumerate(cases):
        frames, H, h, w, geo = case
        canvas, tile = R.case_inputs(W, i, case)
        got = _launch(pkg, gpu, canvas, tile, geo, frames)
        ref = R.blend_ref(canvas, tile, geo)
        assert np.array_equal(got, ref), f"W={W} case {i} {case}: {int((got != ref).sum())} of {ref.size} bytes differ"
    print(f"tile kernel W={W}: {len(cases)} cases bit-exact")


def test_tile_kernel_at_every_base_alignment(pkg, gpu):
    """Canvas base and tile base each at byte offsets 0..3, at a pitch of 57 bytes and one of 12."""
    for W, pick in ((19, lambda c: c[4][4] == 2 and c[4][5] == 5 and c[3] == 11), (4, lambda c: c[4][4:] == (1, 1))):
        i, case = next((i, c) for i, c in enumerate(R.geometry_cases(W)) if pick(c))
        frames, H, h, w, geo = case
        canvas, tile = R.case_inputs(W, i, case)
        ref = R.blend_ref(canvas, tile, geo)
        for c_off in range(4):
            for t_off in range(4):
                got = _launch(pkg, gpu, canvas, tile, geo, frames, c_off, t_off)
                assert np.array_equal(got, ref), (W, c_off, t_off, int((got != ref).sum()))


@pytest.mark.parametrize("Ov", R.GRID_OVERLAPS)
def test_tile_kernel_value_grid(pkg, gpu, Ov):
    """All 65 536 byte pairs under every weight of the overlap pair, one launch: the pairs ride the frame axis."""
    canvas, tile, geo = R.value_grid(*Ov)
    got = _launch(pkg, gpu, canvas, tile, geo, (1, R.GRID_FRAMES))
    ref = R.blend_ref(canvas, tile, geo)
    assert np.array_equal(got, ref), f"O={Ov}: {int((got != ref).sum())} of {ref.size} bytes differ"


def test_tile_kernel_more_than_one_block_per_axis(pkg, gpu):
    """A written rectangle wider than one workgroup's 128 pixels and taller than its 16 rows, ramps crossing both block edges."""
    canvas, tile = R.case_bytes("big.c", (2, 40, 300, 3)), R.case_bytes("big.t", (2, 37, 290, 3))
    geo = (2, 7, 3, 5, 18, 17)
    got = _launch(pkg, gpu, canvas, tile, geo, (1, 2), 1, 3)
    ref = R.blend_ref(canvas, tile, geo)
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {ref.size} bytes differ"
    t = _tiles(pkg).Tile(2, 7, 37, 290, 3, 5, 18, 17)
    c5 = torch.from_numpy(canvas.copy())[None].to(gpu)
    _tiles(pkg).blend_tile(c5, torch.from_numpy(tile)[None].to(gpu), t, backend="torch")       # the torch path on the device
    assert np.array_equal(c5[0].cpu().numpy(), ref)


def test_tile_kernel_argument_checks(pkg, gpu):
    lib = pkg.native.load_library()
    F, H, W, h, w, Oy, Ox = 2, 9, 10, 6, 5, 2, 3
    n = F * H * W * 3
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    tile = torch.zeros((F, h, w, 3), dtype=torch.uint8, device=gpu)
    wy = torch.from_numpy(pkg.windows.ramp_weights(Oy)).to(gpu)
    wxb = torch.from_numpy(pkg.windows.ramp_weights(Ox + 1)).to(gpu)
    c, t, y, x = buf[GUARD:].data_ptr(), tile.data_ptr(), wy.data_ptr(), wxb.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream

    def call(canvas=c, tile=t, wy=y, wx=x, frames=F, H=H, W=W, h=h, w=w, y_at=1, x_at=2, ry=1, rx=1, Oy=Oy, Ox=Ox):
        return lib.drn_tile_blend_u8(canvas, tile, wy, wx, frames, H, W, h, w, y_at, x_at, ry, rx, Oy, Ox, stream)
    bad = {
        "null canvas": dict(canvas=None), "null tile": dict(tile=None),
        "frames < 1": dict(frames=0), "H < 1": dict(H=0), "W < 1": dict(W=0), "h < 1": dict(h=0), "w < 1": dict(w=0),
        "y_at < 0": dict(y_at=-1), "x_at < 0": dict(x_at=-1), "y_at + h > H": dict(y_at=4), "x_at + w > W": dict(x_at=6),
        "ry < 0": dict(ry=-1), "ry >= h": dict(ry=6, Oy=0, wy=None), "rx < 0": dict(rx=-1), "rx >= w": dict(rx=5, Ox=0, wx=None),
        "ry + Oy > h": dict(ry=5), "rx + Ox > w": dict(rx=3),
        "Oy < 0": dict(Oy=-1), "Ox < 0": dict(Ox=-1),
        "weights without a ramp (y)": dict(Oy=0), "a ramp without weights (y)": dict(wy=None),
        "weights without a ramp (x)": dict(Ox=0), "a ramp without weights (x)": dict(wx=None),
        "wy off a 4-byte boundary": dict(wy=y + 2), "wx off a 4-byte boundary": dict(wx=x + 1),
        "a canvas frame of 2^31 bytes": dict(H=1 << 15, W=1 << 15), "a tile frame of 2^31 bytes": dict(H=1 << 16, W=1 << 16,
                                                                                                    h=1 << 15, w=1 << 15),
    }
    for name, kw in bad.items():
        assert call(**kw) == DRN_EINVAL, name
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all(), "a rejected call wrote"
    # the neighbours of the rejected values are accepted
    assert call() == 0 and call(y_at=3, x_at=5) == 0 and call(ry=4) == 0 and call(rx=2) == 0 and call(wx=x + 4) == 0
    assert call(Oy=0, wy=None, Ox=0, wx=None, ry=5, rx=4) == 0
    torch.cuda.synchronize()
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all()


def test_blend_tile_dispatch(pkg, gpu):
    tiles = _tiles(pkg)
    canvas, tile = R.case_bytes("disp.c", (3, 21, 19, 3)), R.case_bytes("disp.t", (3, 12, 11, 3))
    t = tiles.Tile(5, 6, 12, 11, 1, 4, 5, 3)
    ref = R.blend_ref(canvas, tile, (5, 6, 1, 4, 5, 3))
    for backend in ("auto", "hip", "torch"):
        c5 = torch.from_numpy(canvas.copy())[None].to(gpu)
        assert tiles.blend_tile(c5, torch.from_numpy(tile)[None].to(gpu), t, backend=backend) is c5
        assert np.array_equal(c5[0].cpu().numpy(), ref), backend
    with pytest.raises(ValueError, match="hip"):
        tiles.blend_tile(torch.from_numpy(canvas.copy())[None], torch.from_numpy(tile)[None], t, backend="hip")


# ----------------------------------------------------------------------------------------------- pipeline
H, W, ARGS = 48, 64, (32, 32, 8)


def _pipeline(pkg, gpu, forward=False):
    sw = pkg.synthetic_weights
    models = {}
    for kind, fw in (("inverse", False), ("forward", True)):
        if fw and not forward:
            continue
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
    return _pipeline(pkg, gpu, forward=True)


def _compose(pkg, p, call, batches_of, H, W, args):
    """The tiled result composed outside the pipeline: `call(batches)` with tiles off and no restore plan on every crop (its
    results on the host), joined by the numpy reference -> one canvas per result."""
    keep = (p.tile_height, p.tile_width, p.restore_plan)
    p.tile_height = p.tile_width = 0
    p.restore_plan = None
    canvases = None
    for t in _tiles(pkg).plan_tiles(H, W, *args):
        outs = call(batches_of(lambda v: v[..., t.y:t.y + t.h, t.x:t.x + t.w].contiguous()))
        if canvases is None:
            canvases = [np.zeros(o.shape[:2] + (H, W, 3), dtype=np.uint8) for o in outs]
        for k, o in enumerate(outs):
            B, T = o.shape[:2]
            c = R.blend_ref(canvases[k].reshape(B * T, H, W, 3), np.ascontiguousarray(o).reshape(B * T, t.h, t.w, 3),
                            (t.y, t.x, t.ry, t.rx, t.Oy, t.Ox))
            canvases[k] = c.reshape(B, T, H, W, 3)
    p.tile_height, p.tile_width, p.restore_plan = keep
    return canvases


def _setup(pkg, pipe, T, windows=False):
    sw = pkg.synthetic_weights
    pipe.set_model_type("inverse")
    pipe.guidance, pipe.restore_plan = 0.0, None
    pipe.window_frames, pipe.window_overlap = (9, 2) if windows else (0, 8)
    pipe.tile_height, pipe.tile_width, pipe.tile_overlap = ARGS
    rgb = sw.synth_tensor(f"tiles.gpu.rgb{T}", (1, 3, T, H, W), torch.float32, scale=1.0)
    noise = sw.synth_tensor("tiles.gpu.xT", (1, 16, 2, 4, 4), torch.float32, scale=80.0)        # one tile's, one window's
    ci = torch.tensor([[0], [3]], dtype=torch.long)
    return rgb, noise, ci


@pytest.mark.parametrize("windows", (False, True), ids=("whole_clip", "windowed"))
def test_tiled_pipeline_is_the_composition_by_hand(pkg, gpu, pipe, windows):
    """9 x 48 x 64 in 32 x 32 tiles at overlap 8 (2 x 3 tiles); with windows on the clip has 17 frames (windows of 9 at overlap 2),
    so that every tile is itself three windows."""
    p = pipe
    T = 17 if windows else 9
    rgb, noise, ci = _setup(pkg, p, T, windows)
    whole = lambda v: v
    flags = [False, True]

    def batch(crop, idx):
        c = crop(rgb)
        return {"rgb": c, "video": c, "context_index": idx}
    got = p.generate_video(batch(whole, ci[1:2]), normalize_normal=True, seed=5, init_noise=noise)
    (ref,) = _compose(pkg, p, lambda b: [p.generate_video(b, normalize_normal=True, seed=5, init_noise=noise)],
                      lambda crop: batch(crop, ci[1:2]), H, W, ARGS)
    assert got.shape == (1, T, H, W, 3) and got.dtype == np.uint8
    assert np.array_equal(got, ref), f"{(got != ref).sum()} bytes differ"
    # without init_noise every tile draws the same start noise from the seed
    a = p.generate_video(batch(whole, ci[1:2]), normalize_normal=True, seed=5)
    (b,) = _compose(pkg, p, lambda bb: [p.generate_video(bb, normalize_normal=True, seed=5)], lambda crop: batch(crop, ci[1:2]),
                    H, W, ARGS)
    assert np.array_equal(a, b)
    # the join is a real cross-fade: hard cuts give other bytes
    p.tile_overlap = 0
    assert not np.array_equal(p.generate_video(batch(whole, ci[1:2]), normalize_normal=True, seed=5, init_noise=noise), ref)
    p.tile_overlap = ARGS[2]
    # passes stepped together, and batches one after the other
    both = p.generate_video_passes(batch(whole, ci), normalize_normal=flags, seed=5, init_noise=noise)
    refs = _compose(pkg, p, lambda b: p.generate_video_passes(b, normalize_normal=flags, seed=5, init_noise=noise),
                    lambda crop: batch(crop, ci), H, W, ARGS)
    assert len(both) == 2 and all(np.array_equal(x, y) for x, y in zip(both, refs))
    assert np.array_equal(both[1], ref) and not np.array_equal(both[0], both[1])
    each = p.generate_video_each([batch(whole, ci[0:1]), batch(whole, ci[1:2])], flags, seed=5, init_noise=noise)
    assert all(np.array_equal(x, y) for x, y in zip(each, refs))
    # to_host=False: the same bytes, on the device
    dev = p.generate_video(batch(whole, ci[1:2]), normalize_normal=True, seed=5, init_noise=noise, to_host=False)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), ref)
    devs = p.generate_video_passes(batch(whole, ci), normalize_normal=flags, seed=5, init_noise=noise, to_host=False)
    assert all(d.is_cuda and np.array_equal(d.cpu().numpy(), r) for d, r in zip(devs, refs))


def test_tiled_pipeline_with_a_stretch_restore_plan(pkg, gpu, pipe):
    """The restore plan runs once, on the joined picture, and cuts the time padding (7 -> 9 frames by the fit)."""
    fit = importlib.import_module(pkg.__name__ + ".fit")
    p = pipe
    _, noise, ci = _setup(pkg, p, 9)
    image = pkg.synthetic_weights.synth_tensor("tiles.gpu.img", (1, 7, 60, 56, 3), torch.float32).abs().clamp(max=1.0)
    plan = fit.plan_fit(7, 60, 56, "stretch", H, W)
    clip = fit.fit_frames(image, plan, device=gpu)
    assert clip.shape == (1, 3, 9, H, W)

    def batch(crop):
        c = crop(clip)
        return {"rgb": c, "video": c, "context_index": ci[1:2]}
    (small,) = _compose(pkg, p, lambda b: [p.generate_video(b, normalize_normal=True, seed=5, init_noise=noise)], batch, H, W, ARGS)
    p.restore_plan = fit.plan_restore(plan)
    want = fit.restore_frames(torch.from_numpy(small).to(gpu), p.restore_plan).cpu().numpy()
    got = p.generate_video(batch(lambda v: v), normalize_normal=True, seed=5, init_noise=noise)
    assert got.shape == want.shape == (1, 7, 60, 56, 3) and np.array_equal(got, want)
    assert p.restore_plan is not None
    dev = p.generate_video(batch(lambda v: v), normalize_normal=True, seed=5, init_noise=noise, to_host=False)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    # the other two entry points: the normal pass of both is the same restored canvas
    whole = batch(lambda v: v)
    both = p.generate_video_passes(dict(whole, context_index=ci), normalize_normal=[False, True], seed=5, init_noise=noise)
    each = p.generate_video_each([dict(whole, context_index=ci[0:1]), whole], [False, True], seed=5, init_noise=noise)
    assert np.array_equal(both[1], want) and np.array_equal(each[1], want)
    assert both[0].shape == want.shape and np.array_equal(both[0], each[0]) and not np.array_equal(both[0], want)
    p.restore_plan = None


def test_tiles_off_and_one_tile_are_the_untiled_call(pkg, gpu, pipe):
    p = pipe
    rgb, _, ci = _setup(pkg, p, 9)
    noise = pkg.synthetic_weights.synth_tensor("tiles.gpu.xTw", (1, 16, 2, H // 8, W // 8), torch.float32, scale=80.0)
    batch = {"rgb": rgb, "video": rgb, "context_index": ci[1:2]}
    p.tile_height = p.tile_width = 0
    off = torch.from_numpy(p.generate_video(batch, normalize_normal=True, seed=5, init_noise=noise))
    for th, tw in ((48, 64), (64, 64), (576, 1024), (0, 64), (48, 0)):
        p.tile_height, p.tile_width = th, tw
        assert torch.equal(torch.from_numpy(p.generate_video(batch, normalize_normal=True, seed=5, init_noise=noise)), off), (th, tw)
    p.tile_height, p.tile_width = 32, 32
    assert not torch.equal(torch.from_numpy(p.generate_video(batch, normalize_normal=True, seed=5)), off)


# ----------------------------------------------------------------------------------------------- nodes
NAMES = ("base_color", "metallic", "roughness", "normal", "depth")          # the inverse node's order
TILE_KW = dict(tile_height=ARGS[0], tile_width=ARGS[1], tile_overlap=ARGS[2])


def _bytes(image):
    u8 = (image * 255.0).round().to(torch.uint8)
    assert torch.equal(u8.float() / 255.0, image)
    return u8.numpy()


def test_inverse_node_tiled_is_the_crops_composed_by_hand(pkg, gpu, pipe):
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    tiles = _tiles(pkg)
    T = 9
    image = pkg.synthetic_weights.synth_tensor("tiles.node.img", (1, T, H, W, 3), torch.float32).abs().clamp(max=1.0)
    got = node.run_inverse_pass(pipe, image, guidance=0.0, seed=3, **TILE_KW)
    assert len(got) == 5 and all(o.shape == (T, H, W, 3) and o.dtype == torch.float32 for o in got)
    canvases = [np.zeros((T, H, W, 3), dtype=np.uint8) for _ in got]
    for t in tiles.plan_tiles(H, W, *ARGS):
        outs = node.run_inverse_pass(pipe, image[:, :, t.y:t.y + t.h, t.x:t.x + t.w].contiguous(), guidance=0.0, seed=3)
        assert (pipe.tile_height, pipe.tile_width) == (0, 0)
        for k, o in enumerate(outs):
            canvases[k] = R.blend_ref(canvases[k], _bytes(o), (t.y, t.x, t.ry, t.rx, t.Oy, t.Ox))
    for name, a, c in zip(NAMES, got, canvases):
        assert np.array_equal(_bytes(a), c), name
    assert not torch.equal(got[0], got[3])
    # passes one after the other: the same bits
    pipe.batch_passes = False
    seq = node.run_inverse_pass(pipe, image, guidance=0.0, seed=3, **TILE_KW)
    pipe.batch_passes = True
    assert all(torch.equal(a, b) for a, b in zip(got, seq))
    with pytest.raises(ValueError, match="tile_overlap"):
        node.run_inverse_pass(pipe, image, guidance=0.0, seed=3, tile_height=32, tile_width=32, tile_overlap=17)


def _gbuffers(pkg, T):
    sw = pkg.synthetic_weights
    names = ("depth", "normal", "roughness", "metallic", "base_color")
    g = {k: sw.synth_tensor("tiles.fw." + k, (1, T, H, W, 3), torch.float32).abs().clamp(max=1.0) for k in names}
    env = sw.synth_tensor("tiles.fw.env", (1, 32, 64, 3), torch.float32).abs() * 4.0
    return names, g, env


def test_forward_node_tiled_is_the_crops_composed_by_hand(pkg, gpu, pipe, monkeypatch):
    """The node builds the environment conditions for the whole picture; the pipeline crops them per tile like the G-buffers.
    By hand: the batch the node handed over, every picture-sized tensor cropped, rendered with tiles off, joined by the reference."""
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    names, g, env = _gbuffers(pkg, 9)
    handed = {}
    real = pipe.generate_video

    def spy(data_batch, **kw):
        handed["batch"], handed["kw"] = data_batch, kw
        return real(data_batch=data_batch, **kw)
    monkeypatch.setattr(pipe, "generate_video", spy)
    (got,) = node.run_forward_pass(pipe, *(g[k] for k in names), env, guidance=0.0, seed=5, env_format="proj", env_rotation=180.0,
                                   env_spin=90.0, **TILE_KW)
    monkeypatch.undo()
    assert got.shape == (1, 9, H, W, 3) and (pipe.tile_height, pipe.tile_width, pipe.tile_overlap) == ARGS
    full = handed["batch"]
    assert all(full[k].shape[3:] == (H, W) for k in ("env_ldr", "env_log", "env_nrm", "depth", "basecolor"))

    def batches_of(crop):
        cache = {}
        out = {}
        for k, v in full.items():
            if isinstance(v, torch.Tensor) and v.ndim == 5 and tuple(v.shape[3:]) == (H, W):
                if id(v) not in cache:
                    cache[id(v)] = crop(v)
                v = cache[id(v)]
            out[k] = v
        return out
    (ref,) = _compose(pkg, pipe, lambda b: [pipe.generate_video(data_batch=b, **handed["kw"])], batches_of, H, W, ARGS)
    assert np.array_equal(_bytes(got), ref), f"{(_bytes(got) != ref).sum()} bytes differ"
    (off,) = node.run_forward_pass(pipe, *(g[k] for k in names), env, guidance=0.0, seed=5, env_format="proj", env_rotation=180.0,
                                   env_spin=90.0)
    assert (pipe.tile_height, pipe.tile_width) == (0, 0) and not torch.equal(off, got)


def test_relight_tiled_is_the_two_tiled_nodes_chained(pkg, gpu, pipe):
    """Cosmos1Relight tiles both stages: its bits are those of the two tiled nodes (each checked against the crops composed by hand
    above) chained through the host."""
    sw = pkg.synthetic_weights
    T = 9
    image = sw.synth_tensor("tiles.rl.img", (1, T, H, W, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("tiles.rl.env", (1, 32, 64, 3), torch.float32).abs() * 4.0
    relight = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    got = relight.run_relight(pipe, pipe, image, env, seed=3, env_spin=45.0, **TILE_KW)
    assert len(got) == 6 and got[0].shape == (1, T, H, W, 3)
    g = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]().run_inverse_pass(pipe, image, seed=3, **TILE_KW)
    g5 = dict(zip(NAMES, (o.reshape(1, -1, *o.shape[1:]) for o in g)))
    (relit,) = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]().run_forward_pass(
        pipe, g5["depth"], g5["normal"], g5["roughness"], g5["metallic"], g5["base_color"], env, seed=3, env_spin=45.0, fit="crop",
        **TILE_KW)
    for name, a, b in zip(("image",) + NAMES, got, (relit, *g)):
        assert torch.equal(a, b), name
    off = relight.run_relight(pipe, pipe, image, env, seed=3, env_spin=45.0)
    assert not torch.equal(off[0], got[0]) and not torch.equal(off[1], got[1])
