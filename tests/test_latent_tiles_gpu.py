"""Tiles joined in latent space, on the GPU: drn_latent_tile_gather / drn_latent_tile_step_join bit for bit against
tests/latent_tile_refs.py (whose inputs tests/test_latent_tiles_cpu.py shows to separate the wrong kernels), their argument checks,
and the pipeline and nodes with tile_join = "latent" against the composition done by hand from the existing bit-exact pieces.

The step-join works in place, so both canvases and the tile live inside guard bands and are compared WHOLE: elements outside the
written rectangle must keep what they held, and the current canvas must come back unchanged.  Every comparison is an equality.
Plane bases beyond 32 bits are NOT tested: that needs a canvas of more than 4 GiB."""
import importlib

import numpy as np
import pytest
import torch

import latent_tile_refs as L
import tile_refs as R
from conftest import tiny_net
from stub_vae import StubVAE

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD, SENTINEL = 64, 0xA5A5
DRN_EINVAL = -1


def _tiles(pkg):
    return importlib.import_module(pkg.__name__ + ".tiles")


def _banded(gpu, bits, off=0):
    """The bf16 bits of `bits` on the GPU, `off` elements past a 64-element guard band and in front of another ->
    (buffer as int16, bf16 view, start)."""
    n = bits.size
    buf = torch.full((GUARD + off + n + GUARD,), SENTINEL - 0x10000, dtype=torch.int16, device=gpu)
    buf[GUARD + off:GUARD + off + n].copy_(torch.from_numpy(np.ascontiguousarray(bits).reshape(-1).view(np.int16)))
    return buf, buf[GUARD + off:GUARD + off + n].view(BF).view(bits.shape), GUARD + off


def _unband(buf, at, like):
    host = buf.cpu().numpy().view(np.uint16)
    assert (host[:at] == SENTINEL).all() and (host[at + like.size:] == SENTINEL).all(), "wrote outside the tensor"
    return host[at:at + like.size].reshape(like.shape)


def _step_join(pkg, gpu, mo, un, g, cur, nxt, geo, scal, offs=(0, 0, 0, 0)):
    """The kernel on guard-banded tensors at their own element offsets, issued twice, the second time on a fresh copy of the next
    canvas: both results must agree -> the whole next canvas on the CPU.  The inputs must come back unchanged."""
    y_at, x_at, ry, rx, Oy, Ox = geo
    wy = torch.from_numpy(L.ramp_table(Oy)).to(gpu) if Oy else None
    wx = torch.from_numpy(L.ramp_table(Ox)).to(gpu) if Ox else None
    mbuf, mview, m_at = _banded(gpu, mo, offs[0])
    ubuf, uview, u_at = _banded(gpu, un, offs[1]) if un is not None else (None, None, 0)
    cbuf, cview, c_at = _banded(gpu, cur, offs[2])
    runs = []
    for _ in range(2):
        nbuf, nview, n_at = _banded(gpu, nxt, offs[3])
        out = pkg.native.latent_tile_step_join(mview, uview, g, cview, nview, wy, wx, y_at, x_at, ry, rx, *scal)
        assert out is nview
        runs.append(_unband(nbuf, n_at, nxt))
    assert np.array_equal(runs[0], runs[1]), "two launches of one case disagree"
    assert np.array_equal(_unband(cbuf, c_at, cur), cur), "the current canvas was written"
    assert np.array_equal(_unband(mbuf, m_at, mo), mo) and (un is None or np.array_equal(_unband(ubuf, u_at, un), un))
    return runs[0]


def _gather(pkg, gpu, canvas, h, w, y_at, x_at, c_in, copies, offs=(0, 0)):
    """drn_latent_tile_gather into a guard-banded output, twice -> the output on the CPU [copies, planes, h, w]."""
    lib = pkg.native.load_library()
    planes, Hc, Wc = canvas.shape
    cbuf, cview, c_at = _banded(gpu, canvas, offs[0])
    blank = np.full((copies, planes, h, w), 0x7FC0, dtype=np.uint16)
    runs = []
    for _ in range(2):
        obuf, oview, o_at = _banded(gpu, blank, offs[1])
        rc = lib.drn_latent_tile_gather(cview.data_ptr(), oview.data_ptr(), planes, Hc, Wc, h, w, y_at, x_at, c_in, copies,
                                        torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        runs.append(_unband(obuf, o_at, blank))
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(_unband(cbuf, c_at, canvas), canvas)
    return runs[0]


@pytest.mark.parametrize("canvas", L.CANVASES)
def test_kernels_geometry_grid_bit_exact(pkg, gpu, canvas):
    cases = L.geometry_cases(canvas)
    for i, case in enumerate(cases):
        planes, cfg, h, w, geo, _ = case
        mo, un, cur, nxt, scal = L.case_inputs(canvas, i, case)
        got = _step_join(pkg, gpu, mo, un, L.GUIDANCE, cur, nxt, geo, scal[1:])
        ref = L.step_join_ref(mo, un, L.GUIDANCE, cur, nxt, geo, scal[1:])
        assert np.array_equal(got, ref), f"{canvas} case {i} {case}: {int((got != ref).sum())} of {ref.size} elements differ"
        copies = 1 + i % 2
        x = _gather(pkg, gpu, cur, h, w, geo[0], geo[1], scal[0], copies)
        assert np.array_equal(x, L.gather_ref(cur, h, w, geo[0], geo[1], scal[0], copies)), f"gather {canvas} case {i} {case}"
    print(f"latent tile kernels {canvas}: {len(cases)} cases bit-exact")


def test_kernels_at_every_base_alignment(pkg, gpu):
    """Every tensor's base at element offsets 0..7, the two canvases and the tile at offsets of their own, at a canvas pitch of 19
    elements and one of 8."""
    for canvas, pick in (((9, 19), lambda c: c[4][4:] == (2, 5) and c[4][3] == 1 and c[1]), ((6, 8), lambda c: c[4][4:] == (1, 1))):
        i, case = next((i, c) for i, c in enumerate(L.geometry_cases(canvas)) if pick(c))
        planes, cfg, h, w, geo, _ = case
        mo, un, cur, nxt, scal = L.case_inputs(canvas, i, case)
        ref = L.step_join_ref(mo, un, L.GUIDANCE, cur, nxt, geo, scal[1:])
        gref = L.gather_ref(cur, h, w, geo[0], geo[1], scal[0], 2)
        for n_off in range(8):
            for t_off in range(8):
                offs = (t_off, (t_off + 3) % 8, (n_off + 5) % 8, n_off)
                got = _step_join(pkg, gpu, mo, un, L.GUIDANCE, cur, nxt, geo, scal[1:], offs)
                assert np.array_equal(got, ref), (canvas, offs, int((got != ref).sum()))
                assert np.array_equal(_gather(pkg, gpu, cur, h, w, geo[0], geo[1], scal[0], 2, (n_off, t_off)), gref), (canvas, n_off, t_off)


@pytest.mark.parametrize("kind", ("bf16", "random"))
@pytest.mark.parametrize("O,axis", L.GRIDS)
def test_step_join_value_grid(pkg, gpu, kind, O, axis):
    """Every finite bf16 in [-4, 4] against rolled copies of itself, and 2^20 random pairs at scale 80, under every weight of a
    single-axis ramp: where a fused multiply-add blend differs from the contract (tests/test_latent_tiles_cpu.py)."""
    mo, cur, nxt, geo, scal = L.value_grid(kind, O, axis)
    got = _step_join(pkg, gpu, mo, None, 0.0, cur, nxt, geo, scal)
    ref = L.step_join_ref(mo, None, 0.0, cur, nxt, geo, scal)
    assert np.array_equal(got, ref), f"{kind} O={O} {axis}: {int((got != ref).sum())} of {ref.size} elements differ"


def test_kernels_more_than_one_block_per_axis(pkg, gpu):
    """A written rectangle wider than one workgroup's 128 elements and taller than its 16 rows, with and without CFG, ramps
    crossing a block edge; the torch path on the device agrees."""
    tiles = _tiles(pkg)
    planes, (Hc, Wc), (h, w), geo = L.BIG["planes"], L.BIG["canvas"], L.BIG["tile"], L.BIG["geo"]
    mo, un = L.case_bits("big.m", (planes, h, w), 1.0), L.case_bits("big.u", (planes, h, w), 1.0)
    cur, nxt = L.case_bits("big.c", (planes, Hc, Wc), 2.0), L.case_bits("big.n", (planes, Hc, Wc), 2.0)
    scal = L.scalars(L.SIGMAS[1], L.SIGMAS[2])
    for u in (None, un):
        got = _step_join(pkg, gpu, mo, u, L.GUIDANCE, cur, nxt, geo, scal[1:], (1, 3, 5, 7))
        ref = L.step_join_ref(mo, u, L.GUIDANCE, cur, nxt, geo, scal[1:])
        assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {ref.size} elements differ"
    five = lambda b: torch.from_numpy(b.view(np.int16)).to(gpu).view(BF)[:, None, None].contiguous()
    t = tiles.Tile(geo[0], geo[1], h, w, *geo[2:])
    n5 = five(nxt)
    tiles.latent_step_join(five(mo), five(un), L.GUIDANCE, five(cur), n5, t, *scal[1:], backend="torch")
    assert np.array_equal(n5[:, 0, 0].cpu().view(torch.int16).numpy().view(np.uint16), ref)       # (ref: the CFG case's)
    for copies in (1, 2):
        x = _gather(pkg, gpu, cur, h, w, geo[0], geo[1], scal[0], copies, (3, 1))
        assert np.array_equal(x, L.gather_ref(cur, h, w, geo[0], geo[1], scal[0], copies))
        y = tiles.latent_gather(five(cur), t, scal[0], copies)                                   # the wrapper, 5-D
        assert y.shape == (copies * planes, 1, 1, h, w)
        assert np.array_equal(y.cpu().view(torch.int16).numpy().view(np.uint16).reshape(x.shape), x)


def test_kernel_argument_checks(pkg, gpu):
    lib = pkg.native.load_library()
    P, Hc, Wc, h, w, Oy, Ox = 2, 9, 10, 6, 5, 2, 3
    n = P * Hc * Wc
    new = lambda: torch.full((GUARD + n + GUARD,), SENTINEL - 0x10000, dtype=torch.int16, device=gpu)
    cur, nxt, out = new(), new(), new()
    tile = torch.zeros((2, P, h, w), dtype=BF, device=gpu)
    wy = torch.from_numpy(L.ramp_table(Oy)).to(gpu)
    wxb = torch.from_numpy(L.ramp_table(Ox + 1)).to(gpu)
    c, nx, o, t, y, x = cur[GUARD:].data_ptr(), nxt[GUARD:].data_ptr(), out[GUARD:].data_ptr(), tile.data_ptr(), wy.data_ptr(), wxb.data_ptr()
    u = tile[1].data_ptr()
    stream = torch.cuda.current_stream().cuda_stream

    def join(model_out=t, uncond=u, cur=c, nxt=nx, wy=y, wx=x, planes=P, Hc=Hc, Wc=Wc, h=h, w=w, y_at=1, x_at=2, ry=1, rx=1, Oy=Oy,
             Ox=Ox, sigma=1.5):
        return lib.drn_latent_tile_step_join(model_out, uncond, 1.5, cur, nxt, wy, wx, planes, Hc, Wc, h, w, y_at, x_at, ry, rx, Oy,
                                             Ox, 0.25, 0.5, sigma, -0.5, stream)

    def gather(canvas=c, out=o, planes=P, Hc=Hc, Wc=Wc, h=h, w=w, y_at=1, x_at=2, copies=2):
        return lib.drn_latent_tile_gather(canvas, out, planes, Hc, Wc, h, w, y_at, x_at, 0.5, copies, stream)
    bad_join = {
        "null model_out": dict(model_out=None), "null cur": dict(cur=None), "null next": dict(nxt=None),
        "one buffer": dict(nxt=c), "odd pointer": dict(model_out=t + 1), "odd canvas": dict(nxt=nx + 1),
        "planes < 1": dict(planes=0), "Hc < 1": dict(Hc=0), "Wc < 1": dict(Wc=0), "h < 1": dict(h=0), "w < 1": dict(w=0),
        "y_at < 0": dict(y_at=-1), "x_at < 0": dict(x_at=-1), "y_at + h > Hc": dict(y_at=4), "x_at + w > Wc": dict(x_at=6),
        "ry < 0": dict(ry=-1), "ry >= h": dict(ry=6, Oy=0, wy=None), "rx < 0": dict(rx=-1), "rx >= w": dict(rx=5, Ox=0, wx=None),
        "ry + Oy > h": dict(ry=5), "rx + Ox > w": dict(rx=3), "Oy < 0": dict(Oy=-1), "Ox < 0": dict(Ox=-1),
        "weights without a ramp (y)": dict(Oy=0), "a ramp without weights (y)": dict(wy=None),
        "weights without a ramp (x)": dict(Ox=0), "a ramp without weights (x)": dict(wx=None),
        "wy off a 4-byte boundary": dict(wy=y + 2), "wx off a 4-byte boundary": dict(wx=x + 1),
        "sigma == 0": dict(sigma=0.0),
        "a canvas plane of 2^31 elements": dict(Hc=1 << 16, Wc=1 << 15),
        "a tile plane of 2^31 elements": dict(Hc=1 << 16, Wc=1 << 16, h=1 << 16, w=1 << 15),
    }
    for name, kw in bad_join.items():
        assert join(**kw) == DRN_EINVAL, name
    bad_gather = {
        "null canvas": dict(canvas=None), "null out": dict(out=None), "odd pointer": dict(out=o + 1),
        "planes < 1": dict(planes=0), "Hc < 1": dict(Hc=0), "Wc < 1": dict(Wc=0), "h < 1": dict(h=0), "w < 1": dict(w=0),
        "y_at < 0": dict(y_at=-1), "x_at < 0": dict(x_at=-1), "y_at + h > Hc": dict(y_at=4), "x_at + w > Wc": dict(x_at=6),
        "copies 0": dict(copies=0), "copies 3": dict(copies=3),
        "a canvas plane of 2^31 elements": dict(Hc=1 << 16, Wc=1 << 15),
    }
    for name, kw in bad_gather.items():
        assert gather(**kw) == DRN_EINVAL, name
    torch.cuda.synchronize()
    want = SENTINEL - 0x10000
    assert (cur == want).all() and (nxt == want).all() and (out == want).all(), "a rejected call wrote"
    # the neighbours of the rejected values are accepted
    assert join() == 0 and join(y_at=3, x_at=5) == 0 and join(ry=4) == 0 and join(rx=2) == 0 and join(wx=x + 4) == 0
    assert join(uncond=None) == 0 and join(Oy=0, wy=None, Ox=0, wx=None, ry=5, rx=4) == 0
    assert gather() == 0 and gather(copies=1) == 0 and gather(y_at=3, x_at=5) == 0
    torch.cuda.synchronize()
    for b in (cur, nxt, out):
        assert (b[:GUARD] == want).all() and (b[GUARD + n:] == want).all()
    assert (cur == want).all(), "the current canvas was written"


# ----------------------------------------------------------------------------------------------- pipeline
H, W, ARGS = 48, 64, (32, 32, 8)
STEPS = 2


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
        "/nonexistent", "x.pt", model_type=None, vae_instance=StubVAE(), model_instance=models, guidance=0.0, num_steps=STEPS)
    p.device = gpu
    p.set_model_type("inverse")
    return p


@pytest.fixture(scope="module")
def pipe(pkg, gpu):
    return _pipeline(pkg, gpu)


def _setup(pkg, pipe, T, windows=False, overlap=ARGS[2], kind="inverse"):
    sw = pkg.synthetic_weights
    pipe.set_model_type(kind)
    pipe.guidance, pipe.restore_plan, pipe.num_steps = 0.0, None, STEPS
    pipe.window_frames, pipe.window_overlap = (9, 2) if windows else (0, 8)
    pipe.tile_height, pipe.tile_width, pipe.tile_overlap, pipe.tile_join = ARGS[0], ARGS[1], overlap, "latent"
    rgb = sw.synth_tensor(f"lt.gpu.rgb{T}", (1, 3, T, H, W), torch.float32, scale=1.0)
    noise = sw.synth_tensor("lt.gpu.xT", (1, 16, 2, H // 8, W // 8), torch.float32, scale=80.0)     # the canvas's, one window's
    ci = torch.tensor([[0], [3]], dtype=torch.long)
    return rgb, noise, ci


def _torch_join(nxt, b, tl, gpu):
    """The blend on a torch canvas, written out: eager torch device ops, one rounding each."""
    dst = nxt[..., tl.y + tl.ry:tl.y + tl.h, tl.x + tl.rx:tl.x + tl.w]
    src = b[..., tl.ry:, tl.rx:].float()
    fy, fx = np.ones(tl.h - tl.ry, dtype=np.float32), np.ones(tl.w - tl.rx, dtype=np.float32)
    fy[:tl.Oy], fx[:tl.Ox] = L.ramp_table(tl.Oy), L.ramp_table(tl.Ox)
    wgt = torch.from_numpy(fy[:, None] * fx[None, :]).to(gpu)
    a = dst.float()
    d = src - a
    m = wgt * d
    dst.copy_(torch.where(wgt == 1.0, src, a + m).to(BF))


def _hand(pkg, p, batches, flags, noise, kind="inverse"):
    """tile_join = "latent" composed outside the pipeline from the existing pieces.  Per window: per tile the crops (cut, cropped,
    uploaded as the pipeline uploads) and their condition latents; the joint loop with model.net, N.edm_scale_input /
    N.cfg_combine / N.edm_step on contiguous crops and the torch blend on a torch canvas; then tiles outside, windows inside:
    model.decode, N.postprocess_window_u8 with the window's carry, joined by tile_refs.blend_ref -> per batch, per pass uint8."""
    N, tiles, gpu = pkg.native, _tiles(pkg), p.device
    ref = next(b[k] for b in batches[:1] for k in ("rgb", "depth") if k in b)
    T = ref.shape[2]
    plan = tiles.plan_tiles(H, W, p.tile_height, p.tile_width, p.tile_overlap)
    lat = [tiles.latent_tile(t, 8) for t in plan]
    wins = pkg.windows.plan_windows(T, p.window_frames, p.window_overlap) if p.window_frames else [pkg.windows.Window(0, 0, 0, 0, 0)]
    Wf = p.window_frames or T
    p._ensure_model_loaded((1, ref.shape[1], Wf, plan[0].h, plan[0].w))
    model = p.model
    sched = model.scheduler
    canvases = []                                                                # [window][batch]: [P, 16, F, 6, 8]
    for win in wins:
        per_batch = []
        for b in batches:
            conds = []
            for t in plan:
                cache = {}

                def part(v):
                    if not isinstance(v, torch.Tensor):
                        return v
                    if id(v) not in cache:
                        q = v
                        if q.ndim == 5 and tuple(q.shape[3:]) == (H, W):
                            q = q[..., t.y:t.y + t.h, t.x:t.x + t.w]
                        if len(wins) > 1 and q.ndim == 5 and q.shape[2] == T:
                            q = q[:, :, win.start:win.start + Wf]
                        cache[id(v)] = q.contiguous().to(device=gpu, dtype=BF)
                    return cache[id(v)]
                tb = {k: part(v) for k, v in b.items()}
                model._get_conditions(tb)
                conds.append(tb["latent_condition"])
            cis = [int(v) for v in b["context_index"].flatten().tolist()]
            P = len(cis)
            sched.set_timesteps(p.num_steps)
            model.net.prepare_timesteps([float(s) for s in sched.timesteps])
            cur = noise.to(device=gpu, dtype=BF).expand(P, *noise.shape[1:]).contiguous()
            for k, ts in enumerate(sched.timesteps):
                sg = torch.as_tensor(ts, dtype=torch.float32)                     # the oracle's expressions (oracle/dit_oracle.py)
                c_in = float(1 / torch.sqrt(sg ** 2 + 0.5 ** 2))
                c_skip, c_out = float(0.5 ** 2 / (sg ** 2 + 0.5 ** 2)), float((sg * 0.5) / torch.sqrt(sg ** 2 + 0.5 ** 2))
                dt = float(sched.sigmas[k + 1] - sg)
                nxt = torch.full_like(cur, float("nan"))
                for cond, tl in zip(conds, lat):
                    crop = cur[..., tl.y:tl.y + tl.h, tl.x:tl.x + tl.w].contiguous()
                    xs = N.edm_scale_input(crop, c_in)
                    lc = cond.expand(P, *cond.shape[1:])
                    if p.guidance > 0:
                        both = model.net(x=torch.cat([xs, xs], 0), timesteps=ts, latent_condition=torch.cat([lc, torch.zeros_like(lc)], 0),
                                         context_index=cis + [0] * P)
                        out = N.cfg_combine(both[:P].contiguous(), both[P:].contiguous(), float(p.guidance))
                    else:
                        out = model.net(x=xs, timesteps=ts, latent_condition=lc, context_index=cis)
                    _torch_join(nxt, N.edm_step(out.contiguous(), crop, c_skip, c_out, float(sg), dt), tl, gpu)
                cur = nxt
            assert not cur.float().isnan().any()
            per_batch.append(cur)
        canvases.append(per_batch)
    O = p.window_overlap if len(wins) > 1 else 0
    ramp = torch.from_numpy(pkg.windows.ramp_weights(O)).to(gpu) if O else None
    outs = [[np.zeros((1, T, H, W, 3), dtype=np.uint8) for _ in fl] for fl in flags]
    for t, tl in zip(plan, lat):
        for c, fl in enumerate(flags):
            for k, flag in enumerate(fl):
                frames = np.zeros((T, t.h, t.w, 3), dtype=np.uint8)
                carry = None
                for i, win in enumerate(wins):
                    z = canvases[i][c][k:k + 1, ..., tl.y:tl.y + tl.h, tl.x:tl.x + tl.w].contiguous()
                    video = model.decode(z).to(BF).contiguous()
                    u8 = N.postprocess_window_u8(video, carry, ramp if carry is not None else None, win.ramp_at, win.write_lo,
                                                 win.write_hi or video.shape[2], flag)
                    frames[win.out_at:win.out_at + u8.shape[1]] = u8[0].cpu().numpy()
                    carry = video[:, :, Wf - O:].contiguous() if O and i + 1 < len(wins) else None
                outs[c][k] = R.blend_ref(outs[c][k][0], frames, (t.y, t.x, t.ry, t.rx, t.Oy, t.Ox))[None]
    return outs


@pytest.mark.parametrize("guidance", (0.0, 1.5))
@pytest.mark.parametrize("windows", (False, True), ids=("whole_clip", "windowed"))
def test_latent_joined_pipeline_is_the_composition_by_hand(pkg, gpu, pipe, windows, guidance):
    """9 x 48 x 64 in 32 x 32 tiles at overlap 8: 2 x 3 tiles at latent offsets 0 / 2 and 0 / 3 / 4 of a 6 x 8 canvas, rx = 2, ramps
    of 1; with windows on the clip has 17 frames (windows of 9 at overlap 2)."""
    p = pipe
    T = 17 if windows else 9
    rgb, noise, ci = _setup(pkg, p, T, windows)
    p.guidance = guidance
    flags = [False, True]
    batch = lambda idx: {"rgb": rgb, "video": rgb, "context_index": idx}
    got = p.generate_video(batch(ci[1:2]), normalize_normal=True, seed=5, init_noise=noise)
    ((ref,),) = _hand(pkg, p, [batch(ci[1:2])], [[True]], noise)
    assert got.shape == (1, T, H, W, 3) and got.dtype == np.uint8
    assert np.array_equal(got, ref), f"{(got != ref).sum()} bytes differ"
    # the join is real: independent tiles give other bytes (tile-shaped noise: the canvas's top left corner)
    p.tile_join = "pixel"
    pixel = p.generate_video(batch(ci[1:2]), normalize_normal=True, seed=5, init_noise=noise[..., :4, :4].contiguous())
    p.tile_join = "latent"
    assert pixel.shape == got.shape and not np.array_equal(pixel, got)
    # two passes stepped together, and batches one after the other
    both = p.generate_video_passes(batch(ci), normalize_normal=flags, seed=5, init_noise=noise)
    (refs,) = _hand(pkg, p, [batch(ci)], [flags], noise)
    assert len(both) == 2 and all(np.array_equal(x, y) for x, y in zip(both, refs))
    assert np.array_equal(both[1], ref) and not np.array_equal(both[0], both[1])
    each = p.generate_video_each([batch(ci[0:1]), batch(ci[1:2])], flags, seed=5, init_noise=noise)
    assert all(np.array_equal(x, y) for x, y in zip(each, refs))
    # to_host=False: the same bytes, on the device
    dev = p.generate_video(batch(ci[1:2]), normalize_normal=True, seed=5, init_noise=noise, to_host=False)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), ref)
    # without init_noise: one randn of the canvas shape under the seed, times sigma_0
    a = p.generate_video(batch(ci[1:2]), normalize_normal=True, seed=5)
    torch.manual_seed(5)
    drawn = torch.randn(size=(1, 16, 2, H // 8, W // 8), device=gpu, dtype=BF) * p.model.scheduler.sigmas[0]
    assert np.array_equal(a, p.generate_video(batch(ci[1:2]), normalize_normal=True, seed=5, init_noise=drawn))
    with pytest.raises(ValueError, match="canvas-shaped"):
        p.generate_video(batch(ci[1:2]), normalize_normal=True, seed=5, init_noise=noise[..., :4, :4].contiguous())


def test_latent_joined_pipeline_with_a_stretch_restore_plan(pkg, gpu, pipe):
    """The restore plan runs once, on the joined picture, and cuts the time padding (7 -> 9 frames by the fit)."""
    fit = importlib.import_module(pkg.__name__ + ".fit")
    p = pipe
    _, noise, ci = _setup(pkg, p, 9)
    image = pkg.synthetic_weights.synth_tensor("lt.gpu.img", (1, 7, 60, 56, 3), torch.float32).abs().clamp(max=1.0)
    plan = fit.plan_fit(7, 60, 56, "stretch", H, W)
    clip = fit.fit_frames(image, plan, device=gpu)
    batch = {"rgb": clip, "video": clip, "context_index": ci[1:2]}
    ((small,),) = _hand(pkg, p, [batch], [[True]], noise)
    p.restore_plan = fit.plan_restore(plan)
    want = fit.restore_frames(torch.from_numpy(small).to(gpu), p.restore_plan).cpu().numpy()
    got = p.generate_video(batch, normalize_normal=True, seed=5, init_noise=noise)
    assert got.shape == want.shape == (1, 7, 60, 56, 3) and np.array_equal(got, want)
    assert p.restore_plan is not None
    dev = p.generate_video(batch, normalize_normal=True, seed=5, init_noise=noise, to_host=False)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    p.restore_plan = None


@pytest.mark.parametrize("Hp,Wp,steps", ((48, 64, STEPS), (48, 64, 1), (64, 64, STEPS)),
                         ids=("the_issues_case", "one_step", "no_tile_shifted_back"))
def test_overlap_0_is_the_hard_cut_pixel_tiling(pkg, gpu, pipe, Hp, Wp, steps):
    """"latent" at tile_overlap 0 against "pixel" at overlap 0 composed by hand, each tile started from its crop of the canvas
    noise: 9 x 48 x 64 in 32 x 32 tiles (2 x 2 tiles, the second row shifted back by 16 rows), and 9 x 64 x 64 (no tile shifted
    back).

    Tiles that share no latent are sampled on their own (`_tile_noises`, DESIGN.md 4i "Overlap 0"): the equality holds for any
    plan and any number of steps.  Without init_noise the canvas noise is the joint loop's: the seed, one randn, times sigma_0."""
    tiles = _tiles(pkg)
    p = pipe
    _setup(pkg, p, 9, overlap=0)
    sw = pkg.synthetic_weights
    rgb = sw.synth_tensor(f"lt.gpu.o0.rgb{Hp}", (1, 3, 9, Hp, Wp), torch.float32, scale=1.0)
    noise = sw.synth_tensor(f"lt.gpu.o0.xT{Hp}", (1, 16, 2, Hp // 8, Wp // 8), torch.float32, scale=80.0)
    ci = torch.tensor([[3]], dtype=torch.long)
    p.num_steps = steps
    batch = lambda crop: {"rgb": crop(rgb), "video": crop(rgb), "context_index": ci}
    got = p.generate_video(batch(lambda v: v), normalize_normal=True, seed=5, init_noise=noise)
    p.tile_join, p.tile_height, p.tile_width = "pixel", 0, 0
    canvas = np.zeros((9, Hp, Wp, 3), dtype=np.uint8)
    plan = tiles.plan_tiles(Hp, Wp, 32, 32, 0)
    assert len(plan) == 4
    for t in plan:
        tl = tiles.latent_tile(t, 8)
        o = p.generate_video(batch(lambda v: v[..., t.y:t.y + t.h, t.x:t.x + t.w].contiguous()), normalize_normal=True, seed=5,
                             init_noise=noise[..., tl.y:tl.y + tl.h, tl.x:tl.x + tl.w].contiguous())
        canvas = R.blend_ref(canvas, o[0], (t.y, t.x, t.ry, t.rx, t.Oy, t.Ox))
    p.num_steps = STEPS
    print(f"overlap 0, {Hp} x {Wp}, {steps} step(s): {int((got[0] != canvas).sum())} of {canvas.size} bytes differ")
    assert np.array_equal(got[0], canvas)
    p.tile_join, p.tile_height, p.tile_width, p.num_steps = "latent", 32, 32, steps
    a = p.generate_video(batch(lambda v: v), normalize_normal=True, seed=5)
    torch.manual_seed(5)
    drawn = torch.randn(size=(1, 16, 2, Hp // 8, Wp // 8), device=gpu, dtype=BF) * p.model.scheduler.sigmas[0]
    assert np.array_equal(a, p.generate_video(batch(lambda v: v), normalize_normal=True, seed=5, init_noise=drawn))
    assert not np.array_equal(a, got)
    with pytest.raises(ValueError, match="canvas-shaped"):
        p.generate_video(batch(lambda v: v), normalize_normal=True, seed=5, init_noise=noise[..., :4, :4].contiguous())
    p.num_steps = STEPS


def test_tiles_off_and_one_tile_are_the_untiled_call(pkg, gpu, pipe):
    p = pipe
    rgb, noise, ci = _setup(pkg, p, 9)
    batch = {"rgb": rgb, "video": rgb, "context_index": ci[1:2]}
    p.tile_height = p.tile_width = 0
    p.tile_join = "pixel"
    off = torch.from_numpy(p.generate_video(batch, normalize_normal=True, seed=5, init_noise=noise))
    p.tile_join = "latent"
    assert torch.equal(torch.from_numpy(p.generate_video(batch, normalize_normal=True, seed=5, init_noise=noise)), off)
    for th, tw in ((48, 64), (64, 64), (576, 1024), (0, 64), (48, 0)):
        p.tile_height, p.tile_width = th, tw
        assert torch.equal(torch.from_numpy(p.generate_video(batch, normalize_normal=True, seed=5, init_noise=noise)), off), (th, tw)
    p.tile_height, p.tile_width = 32, 32
    assert not torch.equal(torch.from_numpy(p.generate_video(batch, normalize_normal=True, seed=5, init_noise=noise)), off)
    p.tile_overlap = 12
    with pytest.raises(ValueError, match="tile_overlap"):
        p.generate_video(batch, normalize_normal=True, seed=5, init_noise=noise)


# ----------------------------------------------------------------------------------------------- nodes
NAMES = ("base_color", "metallic", "roughness", "normal", "depth")          # the inverse node's order
TILE_KW = dict(tile_height=ARGS[0], tile_width=ARGS[1], tile_overlap=ARGS[2], tile_join="latent")


def _bytes(image):
    u8 = (image * 255.0).round().to(torch.uint8)
    assert torch.equal(u8.float() / 255.0, image)
    return u8.numpy()


def _drawn(p, gpu, seed, F=2):
    torch.manual_seed(seed)
    return torch.randn(size=(1, 16, F, H // 8, W // 8), device=gpu, dtype=BF) * p.model.scheduler.sigmas[0]


def test_inverse_node_latent_joined_is_the_composition_by_hand(pkg, gpu, pipe):
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    T = 9
    image = pkg.synthetic_weights.synth_tensor("lt.node.img", (1, T, H, W, 3), torch.float32).abs().clamp(max=1.0)
    got = node.run_inverse_pass(pipe, image, guidance=0.0, seed=3, **TILE_KW)
    assert len(got) == 5 and all(o.shape == (T, H, W, 3) and o.dtype == torch.float32 for o in got)
    assert pipe.tile_join == "latent"
    clip = image.permute(0, 4, 1, 2, 3) * 2.0 - 1.0
    idx = torch.tensor([[pkg.nodes.GBUFFER_INDEX_MAPPING[n]] for n in pkg.nodes.INVERSE_PASSES], dtype=torch.long)
    flags = [n == "normal" for n in pkg.nodes.INVERSE_PASSES]
    (refs,) = _hand(pkg, pipe, [{"rgb": clip, "video": clip, "context_index": idx}], [flags], _drawn(pipe, gpu, 3))
    for name, a, c in zip(NAMES, got, refs):
        assert np.array_equal(_bytes(a), c[0]), name
    # passes one after the other: the same bits; "pixel" gives others
    pipe.batch_passes = False
    seq = node.run_inverse_pass(pipe, image, guidance=0.0, seed=3, **TILE_KW)
    pipe.batch_passes = True
    assert all(torch.equal(a, b) for a, b in zip(got, seq))
    pixel = node.run_inverse_pass(pipe, image, guidance=0.0, seed=3, **dict(TILE_KW, tile_join="pixel"))
    assert pipe.tile_join == "pixel" and not torch.equal(pixel[0], got[0])
    with pytest.raises(ValueError, match="tile_overlap"):
        node.run_inverse_pass(pipe, image, guidance=0.0, seed=3, **dict(TILE_KW, tile_overlap=4))


def test_forward_node_latent_joined_is_the_composition_by_hand(pkg, gpu, pipe, monkeypatch):
    """The node builds the environment conditions for the whole picture; by hand: the batch the node handed over, composed as
    above with the forward model."""
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    sw = pkg.synthetic_weights
    names = ("depth", "normal", "roughness", "metallic", "base_color")
    g = {k: sw.synth_tensor("lt.fw." + k, (1, 9, H, W, 3), torch.float32).abs().clamp(max=1.0) for k in names}
    env = sw.synth_tensor("lt.fw.env", (1, 32, 64, 3), torch.float32).abs() * 4.0
    handed = {}
    real = pipe.generate_video

    def spy(data_batch, **kw):
        handed["batch"] = data_batch
        return real(data_batch=data_batch, **kw)
    monkeypatch.setattr(pipe, "generate_video", spy)
    (got,) = node.run_forward_pass(pipe, *(g[k] for k in names), env, guidance=0.0, seed=5, env_format="proj", env_rotation=180.0,
                                   env_spin=90.0, **TILE_KW)
    monkeypatch.undo()
    assert got.shape == (1, 9, H, W, 3) and pipe.tile_join == "latent" and pipe.model_type == "forward"
    full = dict(handed["batch"])
    full.setdefault("context_index", torch.zeros(1, 1, dtype=torch.long))
    ((ref,),) = _hand(pkg, pipe, [full], [[False]], _drawn(pipe, gpu, 5), kind="forward")
    assert np.array_equal(_bytes(got), ref), f"{(_bytes(got) != ref).sum()} bytes differ"
    (pixel,) = node.run_forward_pass(pipe, *(g[k] for k in names), env, guidance=0.0, seed=5, env_format="proj", env_rotation=180.0,
                                     env_spin=90.0, **dict(TILE_KW, tile_join="pixel"))
    assert not torch.equal(pixel, got)


def test_relight_latent_joined_is_the_two_tiled_nodes_chained(pkg, gpu, pipe):
    sw = pkg.synthetic_weights
    T = 9
    image = sw.synth_tensor("lt.rl.img", (1, T, H, W, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("lt.rl.env", (1, 32, 64, 3), torch.float32).abs() * 4.0
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
    pixel = relight.run_relight(pipe, pipe, image, env, seed=3, env_spin=45.0, **dict(TILE_KW, tile_join="pixel"))
    assert not torch.equal(pixel[0], got[0]) and not torch.equal(pixel[1], got[1])
