"""Tiles joined in latent space, on the host: tiles.latent_tile and the planner property the latent grid rests on, the refusals,
the torch specification (tiles.latent_gather / latent_step_join) against tests/latent_tile_refs.py, the proof that the inputs of
tests/test_latent_tiles_gpu.py tell a wrong kernel from a right one, the model's joint loop with a stub DiT against the
composition by hand, the nodes, and the pipeline's orchestration with a recorder model.  No GPU."""
import importlib

import numpy as np
import pytest
import torch

import latent_tile_refs as L
import tile_refs as R
import window_refs as WR
from stub_vae import StubVAE

BF = torch.bfloat16


def _tiles(pkg):
    return importlib.import_module(pkg.__name__ + ".tiles")


def to_t(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(BF)


def to_bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# ----------------------------------------------------------------------------------------------- the latent grid
def test_latent_tile_conversions_and_refusals(pkg):
    tiles = _tiles(pkg)
    plan = tiles.plan_tiles(1072, 1920, 576, 1024, 64)
    lat = [tiles.latent_tile(t, 8) for t in plan]
    assert [(t.y, t.x) for t in lat] == [(0, 0), (0, 112), (62, 0), (62, 112)]
    assert all((t.h, t.w) == (72, 128) for t in lat)
    assert lat[3] == tiles.Tile(62, 112, 72, 128, 2, 8, 8, 8) and lat[0] == tiles.Tile(0, 0, 72, 128, 0, 0, 0, 0)
    assert lat[1][4:] == (0, 8, 0, 8) and lat[2][4:] == (2, 0, 8, 0)
    assert tiles.covers(lat, 134, 240) and not tiles.covers(lat[:3], 134, 240)
    assert tiles.latent_tile(tiles.Tile(8, 16, 32, 32, 8, 0, 8, 0), 1) == tiles.Tile(8, 16, 32, 32, 8, 0, 8, 0)
    ok = tiles.Tile(16, 24, 32, 32, 8, 8, 8, 8)
    assert tiles.latent_tile(ok, 8) == tiles.Tile(2, 3, 4, 4, 1, 1, 1, 1)
    for k, name in enumerate(tiles.Tile._fields):
        with pytest.raises(ValueError, match=name):
            tiles.latent_tile(ok._replace(**{name: ok[k] + 4}), 8)
    with pytest.raises(ValueError):
        tiles.latent_tile(ok, 0)
    with pytest.raises(ValueError):
        tiles.latent_tile(ok, 8.0)


@pytest.mark.parametrize("size", [32, 64, 576, 1024])
def test_planned_tiles_lie_on_the_latent_grid_and_cover_it(pkg, size):
    """Every overlap that is a multiple of 8 up to half the tile's side, every side 16..2048 on the model's grid: start and ramp_at
    of every span are multiples of 8, and the written ranges cover the axis - so the tiles of a picture cover its latent canvas."""
    tiles = _tiles(pkg)
    plans = 0
    for Ov in range(0, size // 2 + 1, 8):
        for n in range(16, 2049, 16):
            plan = tiles.plan_axis(n, size, Ov)
            if len(plan) == 1:
                continue
            plans += 1
            written = np.zeros(n // 8, dtype=bool)
            for s in plan:
                assert s.start % 8 == 0 and s.ramp_at % 8 == 0, (n, size, Ov, s)
                written[(s.start + s.ramp_at) // 8:(s.start + size) // 8] = True
            assert written.all(), (n, size, Ov)
    assert plans > 0
    # two axes together, through latent_tile and covers
    for H, W, Ov in ((1072, 1920, 64), (48, 64, 8), (48, 64, 0), (2048, 1088, 16), (size + 16, 3 * size - 8, size // 2 // 8 * 8)):
        W, Ov = W - W % 16, min(Ov, size // 2 // 8 * 8)
        plan = tiles.plan_tiles(H, W, size, size, Ov)
        if plan is not None:
            assert tiles.covers([tiles.latent_tile(t, 8) for t in plan], H // 8, W // 8), (H, W, size, Ov)


# ----------------------------------------------------------------------------------------------- specification == reference
def _spec_step_join(pkg, mo, un, g, cur, nxt, geo, scal):
    """tiles.latent_step_join's torch backend on the reference's inputs -> (nxt bits, cur bits afterwards)."""
    tiles = _tiles(pkg)
    h, w = mo.shape[1:]
    t = tiles.Tile(geo[0], geo[1], h, w, *geo[2:])
    five = lambda b: to_t(b)[:, None, None].clone()
    c5, n5 = five(cur), five(nxt)
    tiles.latent_step_join(five(mo), None if un is None else five(un), g, c5, n5, t, *scal, backend="torch")
    return to_bits(n5[:, 0, 0]), to_bits(c5[:, 0, 0])


@pytest.mark.parametrize("canvas", L.CANVASES)
def test_specification_is_the_reference_on_the_geometry_grid(pkg, canvas):
    tiles = _tiles(pkg)
    cases = L.geometry_cases(canvas)
    assert len(cases) > 90
    for i, case in enumerate(cases):
        planes, cfg, h, w, geo, _ = case
        mo, un, cur, nxt, scal = L.case_inputs(canvas, i, case)
        got, cur_after = _spec_step_join(pkg, mo, un, L.GUIDANCE, cur, nxt, geo, scal[1:])
        ref = L.step_join_ref(mo, un, L.GUIDANCE, cur, nxt, geo, scal[1:])
        assert np.array_equal(got, ref), (canvas, i, case)
        assert np.array_equal(cur_after, cur)
        for copies in (1, 2):
            x = tiles.latent_gather(to_t(cur)[:, None, None], tiles.Tile(geo[0], geo[1], h, w, 0, 0, 0, 0), scal[0], copies,
                                    backend="torch")
            assert x.shape == (copies * planes, 1, 1, h, w) and x.is_contiguous()
            assert np.array_equal(to_bits(x[:, 0, 0]).reshape(copies, planes, h, w),
                                  L.gather_ref(cur, h, w, geo[0], geo[1], scal[0], copies))


def test_geometry_grid_reaches_what_the_kernels_branch_on():
    """Every x_at residue mod 8, odd and even pitches, both plane counts, CFG on and off, every overlap pair and ramp origin,
    written widths of one element and of a whole row."""
    seen_x, seen = set(), set()
    for canvas in L.CANVASES:
        for planes, cfg, h, w, (y_at, x_at, ry, rx, Oy, Ox), si in L.geometry_cases(canvas):
            seen_x.add(x_at % 8)
            seen.add(("planes", planes)), seen.add(("cfg", cfg)), seen.add(("O", Oy, Ox)), seen.add(("r", ry, rx)), seen.add(("s", si))
            seen.add(("odd start", (x_at + rx) % 2)), seen.add(("odd width", (w - rx) % 2)), seen.add(("pitch", canvas[1] % 2))
            if w - rx == 1:
                seen.add("one column")
            if (h, w) == canvas:
                seen.add("whole canvas")
    assert seen_x == set(range(8))
    want = {("planes", 1), ("planes", 6), ("cfg", True), ("cfg", False), ("pitch", 0), ("pitch", 1), "one column", "whole canvas"}
    want |= {("O", *o) for o in L.OVERLAPS} | {("r", a, b) for a in L.RAMP_AT for b in L.RAMP_AT} | {("s", k) for k in range(3)}
    want |= {("odd start", k) for k in range(2)} | {("odd width", k) for k in range(2)}
    assert want <= seen, want - seen


@pytest.mark.parametrize("kind", ("bf16", "random"))
@pytest.mark.parametrize("O,axis", L.GRIDS)
def test_specification_is_the_reference_on_the_value_grids_and_a_fused_blend_is_not(pkg, kind, O, axis):
    mo, cur, nxt, geo, scal = L.value_grid(kind, O, axis)
    ref = L.step_join_ref(mo, None, 0.0, cur, nxt, geo, scal)
    got, _ = _spec_step_join(pkg, mo, None, 0.0, cur, nxt, geo, scal)
    assert np.array_equal(got, ref)
    fused = L.step_join_ref(mo, None, 0.0, cur, nxt, geo, scal, variant="fma")
    n = int((fused != ref).sum())
    print(f"value grid {kind} O={O} {axis}: a fused blend differs in {n} of {mo[:, :O, :].size if axis == 'y' else mo[:, :, :O].size}")
    assert n > 0
    # with the step's scalars of the grid the step's result is the model's output: the grid's pairs ARE (a, b)
    y, x = geo[0], geo[1]
    behind = ref[:, y + O:y + mo.shape[1], x:x + mo.shape[2]] if axis == "y" else ref[:, y:y + mo.shape[1], x + O:x + mo.shape[2]]
    assert np.array_equal(L.f32(behind), L.f32(mo[:, O:] if axis == "y" else mo[:, :, O:]))      # (-0 == +0)


def test_dyadic_and_product_weights_do_not_see_a_fused_blend():
    """Why the value grids use single-axis ramps of 5 and 8: at overlaps 1 and 3 every weight is dyadic and the product a fused
    multiply-add keeps unrounded is exact."""
    for O in (1, 3):
        mo, cur, nxt, geo, scal = L.value_grid("bf16", O, "x")
        assert np.array_equal(L.step_join_ref(mo, None, 0.0, cur, nxt, geo, scal, variant="fma"),
                              L.step_join_ref(mo, None, 0.0, cur, nxt, geo, scal))


def test_grid_tells_every_wrong_kernel_from_the_reference():
    """Each stand-in differs from the reference on at least one input the GPU test uses (the geometry grid, the block case, the
    value grids), so a kernel that equals the reference on all of them is none of the stand-ins."""
    caught = {v: 0 for v in L.VARIANTS}
    caught_g = {v: 0 for v in L.GATHER_VARIANTS}
    for canvas in L.CANVASES:
        for i, case in enumerate(L.geometry_cases(canvas)):
            planes, cfg, h, w, geo, _ = case
            mo, un, cur, nxt, scal = L.case_inputs(canvas, i, case)
            ref = L.step_join_ref(mo, un, L.GUIDANCE, cur, nxt, geo, scal[1:])
            for v in L.VARIANTS:
                caught[v] += not np.array_equal(L.step_join_ref(mo, un, L.GUIDANCE, cur, nxt, geo, scal[1:], variant=v), ref)
            for copies in (1, 2):
                gref = L.gather_ref(cur, h, w, geo[0], geo[1], scal[0], copies)
                for v in L.GATHER_VARIANTS:
                    caught_g[v] += not np.array_equal(L.gather_ref(cur, h, w, geo[0], geo[1], scal[0], copies, variant=v), gref)
    mo, cur, nxt, geo, scal = L.value_grid("bf16", 5, "x")
    ref = L.step_join_ref(mo, None, 0.0, cur, nxt, geo, scal)
    caught["blend_at_one"] += not np.array_equal(L.step_join_ref(mo, None, 0.0, cur, nxt, geo, scal, variant="blend_at_one"), ref)
    print("cases that catch each stand-in:", caught, caught_g)
    assert all(caught.values()) and all(caught_g.values()), (caught, caught_g)


# ----------------------------------------------------------------------------------------------- the model's joint loop
class _StubNet:
    """Stands in for the DiT: a deterministic function of its inputs that mixes rows and columns, so that a tile's output depends
    on everything the tile was handed."""

    def __init__(self):
        self.calls = []

    def prepare_timesteps(self, ts):
        self.prepared = list(ts)

    def __call__(self, x, timesteps, latent_condition, context_index):
        self.calls.append((tuple(x.shape), float(timesteps), list(context_index)))
        xf, lf = x.float(), latent_condition[:, :16].float()
        idx = torch.tensor(context_index, dtype=torch.float32).view(-1, 1, 1, 1, 1)
        mixed = xf.roll(1, 3) * 0.25 + xf.roll(-1, 4) * 0.5 + xf.mean((3, 4), keepdim=True) + lf * (0.3 + 0.1 * idx)
        return (mixed / (1.0 + float(timesteps))).to(BF)


def _cpu_model(pkg):
    cfg = pkg.diffusion_renderer_config.get_inverse_renderer_config()
    cfg["model_type"] = "inverse"
    m = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device="cpu")
    m.net, m.vae = _StubNet(), StubVAE()
    return m


def _joint_by_hand(pkg, model, tile_batches, lat, noise, guidance, num_steps):
    """The joint loop written out with the numpy references: per step and tile gather_ref, the net, step_join_ref."""
    sched = pkg.model_diffusion_renderer.CleanEDMEulerScheduler(**{k: v for k, v in model.config.get("scheduler", {}).items()
                                                                  if k != "prediction_type"})
    sched.set_timesteps(num_steps)
    conds = [model.prepare_diffusion_renderer_latent_conditions(dict(b), model.condition_keys) for b in tile_batches]
    cis = [int(v) for v in tile_batches[0]["context_index"].flatten().tolist()]
    P = len(cis)
    shape = tuple(noise.shape[1:])
    cur = to_bits(noise.to(BF).expand(P, *shape)).reshape(-1, *shape[2:])
    for t in sched.timesteps:
        c_in, c_skip, c_out, sigma, dt = sched.step_scalars(t)
        nxt = np.full_like(cur, 0x7FC0)                                      # NaN: every latent must be written
        for cond, tl in zip(conds, lat):
            copies = 2 if guidance > 0 else 1
            xs = to_t(L.gather_ref(cur, tl.h, tl.w, tl.y, tl.x, c_in, copies)).reshape(copies * P, *shape[:2], tl.h, tl.w)
            lc = cond.expand(P, *cond.shape[1:])
            if guidance > 0:
                out = model.net(xs, t, torch.cat([lc, torch.zeros_like(lc)]), cis + [0] * P)
                mo, un = (to_bits(o).reshape(-1, tl.h, tl.w) for o in (out[:P], out[P:]))
            else:
                mo, un = to_bits(model.net(xs, t, lc, cis)).reshape(-1, tl.h, tl.w), None
            nxt = L.step_join_ref(mo, un, guidance, cur, nxt, tl[:2] + tl[4:], (c_skip, c_out, sigma, dt))
        cur = nxt
        sched.current_step += 1
    return to_t(cur).reshape(P, *shape)


@pytest.mark.parametrize("guidance", (0.0, 1.5))
def test_joint_loop_is_the_composition_by_hand(pkg, guidance):
    tiles = _tiles(pkg)
    sw = pkg.synthetic_weights
    H, W, T = 48, 64, 9
    rgb = sw.synth_tensor("lt.cpu.rgb", (1, 3, T, H, W), torch.float32, scale=0.6).to(BF)
    plan = tiles.plan_tiles(H, W, 32, 32, 8)
    lat = [tiles.latent_tile(t, 8) for t in plan]
    assert [(t.y, t.x) for t in lat] == [(0, 0), (0, 3), (0, 4), (2, 0), (2, 3), (2, 4)] and lat[5][4:] == (1, 2, 1, 1)
    ci = torch.tensor([[0], [3]], dtype=torch.long)

    def batches():
        out = []
        for t in plan:
            c = rgb[..., t.y:t.y + t.h, t.x:t.x + t.w].contiguous()
            out.append({"rgb": c, "video": c, "context_index": ci})
        return out
    model = _cpu_model(pkg)
    noise = sw.synth_tensor("lt.cpu.xT", (1, 16, 2, H // 8, W // 8), torch.float32, scale=80.0)
    keep = noise.clone()
    got = model.generate_samples_joint(batches(), lat, (16, 2, 6, 8), guidance=guidance, seed=3, num_steps=3, init_noise=noise)
    assert torch.equal(noise, keep)
    assert got.shape == (2, 16, 2, 6, 8) and got.dtype == BF and not got.float().isnan().any()
    copies = 2 if guidance > 0 else 1
    assert len(model.net.calls) == 3 * 6 and all(c[0] == (2 * copies, 16, 2, 4, 4) for c in model.net.calls)
    assert model.net.calls[0][2] == ([0, 3, 0, 0] if guidance > 0 else [0, 3])
    want = _joint_by_hand(pkg, _cpu_model(pkg), batches(), lat, noise, guidance, 3)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # without init_noise: one randn of the canvas shape under the seed, times sigma_0, shared by the passes
    a = model.generate_samples_joint(batches(), lat, (16, 2, 6, 8), guidance=guidance, seed=3, num_steps=3)
    torch.manual_seed(3)
    drawn = torch.randn(size=(1, 16, 2, 6, 8), dtype=BF) * model.scheduler.sigmas[0]
    b = model.generate_samples_joint(batches(), lat, (16, 2, 6, 8), guidance=guidance, seed=3, num_steps=3, init_noise=drawn)
    assert torch.equal(a, b) and not torch.equal(a, got)
    # a batch that already holds its condition latents is taken as it is
    ready = batches()
    for bb in ready:
        model._get_conditions(bb)
    slim = [{k: bb[k] for k in ("latent_condition", "context_index")} for bb in ready]
    assert torch.equal(model.generate_samples_joint(slim, lat, (16, 2, 6, 8), guidance=guidance, seed=3, num_steps=3,
                                                    init_noise=noise), got)


def test_joint_loop_refusals(pkg):
    tiles = _tiles(pkg)
    model = _cpu_model(pkg)
    rgb = torch.zeros(1, 3, 9, 48, 64, dtype=BF)
    plan = tiles.plan_tiles(48, 64, 32, 32, 8)
    lat = [tiles.latent_tile(t, 8) for t in plan]
    batches = [{"rgb": rgb[..., t.y:t.y + t.h, t.x:t.x + t.w].contiguous(), "context_index": torch.tensor([[3]])} for t in plan]
    run = lambda **kw: model.generate_samples_joint(**{**dict(tile_batches=[dict(b) for b in batches], tiles_lat=lat,
                                                              canvas_shape=(16, 2, 6, 8), num_steps=2), **kw})
    with pytest.raises(ValueError, match="canvas-shaped"):
        run(init_noise=torch.zeros(1, 16, 2, 4, 4))                           # one tile's noise
    with pytest.raises(ValueError, match="tile batches"):
        run(tile_batches=batches[:5])
    with pytest.raises(ValueError, match="do not write every latent"):
        run(tile_batches=batches[:5], tiles_lat=lat[:5])
    with pytest.raises(ValueError, match="context indices"):
        run(init_noise=torch.zeros(2, 16, 2, 6, 8))
    with pytest.raises(ValueError, match="context indices"):
        run(tile_batches=[dict(b, context_index=torch.tensor([[k % 2]])) for k, b in enumerate(batches)])
    model.net = None
    with pytest.raises(RuntimeError, match="weights not loaded"):
        run()


def test_scheduler_step_scalars_are_what_step_and_scale_use(pkg, monkeypatch):
    mod = pkg.model_diffusion_renderer
    seen = {}
    monkeypatch.setattr(mod.N, "edm_step", lambda mo, x, *s: seen.setdefault("step", s) and x)
    monkeypatch.setattr(mod.N, "edm_scale_input", lambda x, c_in: seen.setdefault("c_in", c_in) and x)
    s = mod.CleanEDMEulerScheduler()
    with pytest.raises(RuntimeError):
        s.step_scalars(1.0)
    s.set_timesteps(4)
    x = torch.zeros(2, dtype=BF)
    for k, t in enumerate(s.timesteps):
        seen.clear()
        sc = s.step_scalars(t)
        assert s.current_step == k                                            # the helper does not advance
        sg = torch.as_tensor(t, dtype=torch.float32)                          # the oracle's expressions (oracle/dit_oracle.py)
        assert sc == (float(1 / torch.sqrt(sg ** 2 + 0.5 ** 2)), float(0.5 ** 2 / (sg ** 2 + 0.5 ** 2)),
                      float((sg * 0.5) / torch.sqrt(sg ** 2 + 0.5 ** 2)), float(sg), float(s.sigmas[k + 1] - sg))
        s.scale_model_input(x, t)
        s.step(x, t, x)
        assert seen["c_in"] == sc[0] and seen["step"] == sc[1:] and s.current_step == k + 1
    with pytest.raises(RuntimeError, match="exhausted"):
        s.step(x, 0.02, x)


# ----------------------------------------------------------------------------------------------- the pipeline's orchestration
class _RecorderModel:
    """Stands in for the renderer model: records the crops whose conditions it is asked for and the joint calls; the "sample" of a
    joint call is a canvas that tells windows, batches and positions apart, and `decode` is the stub tokenizer's."""
    process_group = None
    net = None

    def __init__(self):
        self.config = {}
        self.vae = StubVAE()
        self.crops, self.joint, self.single, self.noises = [], [], [], []

    def to(self, device):
        return self

    def _get_conditions(self, data_batch):
        self.crops.append({k: v.clone() for k, v in data_batch.items() if isinstance(v, torch.Tensor)})
        data_batch["latent_condition"] = self.vae.encode(data_batch["rgb"])

    def generate_samples_from_batch(self, data_batch, **kw):
        self.single.append(tuple(data_batch["rgb"].shape))
        self.noises.append(kw.get("init_noise"))
        ci = data_batch["context_index"].reshape(-1)
        return torch.cat([self.vae.encode(data_batch["rgb"]) * (1.0 - 0.1 * float(c)) for c in ci]).to(BF)

    def generate_samples_joint(self, tile_batches, tiles_lat, canvas_shape, guidance, seed, num_steps, init_noise):
        tile_batches = list(tile_batches)
        self.joint.append(dict(batches=tile_batches, tiles=list(tiles_lat), canvas_shape=tuple(canvas_shape), guidance=guidance,
                               seed=seed, num_steps=num_steps, init_noise=init_noise))
        C, F, Hc, Wc = canvas_shape
        ci = tile_batches[0]["context_index"].reshape(-1).float()
        base = torch.linspace(-0.8, 0.8, C * F * Hc * Wc).view(1, C, F, Hc, Wc) + 0.01 * len(self.joint)
        return torch.cat([base * (1.0 - 0.1 * float(c)) for c in ci]).to(BF)

    def decode(self, sample):
        return self.vae.decode(sample)


@pytest.fixture()
def cpu_pipe(pkg, monkeypatch):
    mod = pkg.diffusion_renderer_pipeline
    monkeypatch.setattr(mod.N, "postprocess_window_u8",
                        lambda video, prev, ramp, ramp_at, lo, hi, normalize, out=None: WR.blend_postprocess(video, prev, ramp, ramp_at,
                                                                                                              lo, hi, normalize))
    p = mod.CleanDiffusionRendererPipeline("/nonexistent", "x.pt", model_type=None, model_instance=_RecorderModel(), guidance=0.0,
                                           num_steps=2)
    p.device = torch.device("cpu")
    p.set_model_type("inverse")
    return p


def _decode_join(pkg, p, canvases_of, plan, lat, flags, T, H, W, windows=None):
    """What the walk makes of the joint samples, by hand: per tile (outside) and window (inside) decode the tile's crop of that
    window's canvas, post-process with the window's carry, write the frames; join the tiles by the numpy reference."""
    wins = windows or [pkg.windows.Window(0, 0, 0, 0, 0)]
    O = p.window_overlap if windows else 0
    ramp = torch.from_numpy(pkg.windows.ramp_weights(O)) if O else None
    outs = [np.zeros((1, T, H, W, 3), dtype=np.uint8) for _ in flags]
    for t, tl in zip(plan, lat):
        for k, flag in enumerate(flags):
            frames = np.zeros((1, T, t.h, t.w, 3), dtype=np.uint8)
            carry = None
            for i, win in enumerate(wins):
                video = p.model.decode(canvases_of(i)[k:k + 1, ..., tl.y:tl.y + tl.h, tl.x:tl.x + tl.w].contiguous()).to(BF).contiguous()
                u8 = WR.blend_postprocess(video, carry, ramp if carry is not None else None, win.ramp_at, win.write_lo,
                                          win.write_hi or video.shape[2], flag)
                frames[:, win.out_at:win.out_at + u8.shape[1]] = u8.numpy()
                carry = video[:, :, video.shape[2] - O:].contiguous() if O and i + 1 < len(wins) else None
            outs[k] = R.blend_ref(outs[k][0], frames[0], (t.y, t.x, t.ry, t.rx, t.Oy, t.Ox))[None]
    return outs


def test_pipeline_hands_the_joint_loop_crops_windows_and_tiles_in_order(pkg, cpu_pipe):
    tiles = _tiles(pkg)
    p = cpu_pipe
    model = p.pre_loaded_model_instance
    T, H, W, args = 17, 48, 64, (32, 32, 8)
    rgb = pkg.synthetic_weights.synth_tensor("lt.pipe.rgb", (1, 3, T, H, W), torch.float32, scale=0.6)
    ci = torch.tensor([[0], [3]], dtype=torch.long)
    batch = {"rgb": rgb, "video": rgb, "context_index": ci}
    plan = tiles.plan_tiles(H, W, *args)
    lat = [tiles.latent_tile(t, 8) for t in plan]
    p.tile_height, p.tile_width, p.tile_overlap = args
    # "pixel" never calls the joint loop
    p.generate_video_passes(batch, [False, True], seed=5)
    assert not model.joint and not model.crops and len(model.single) == 6
    # "latent", whole clip: one joint call over the six tiles in raster order, each crop handed over once, then six decodes
    p.tile_join = "latent"
    del model.single[:]
    noise = torch.zeros(1, 16, 3, 6, 8)
    got = p.generate_video_passes(batch, [False, True], seed=5, init_noise=noise)
    assert not model.single and len(model.joint) == 1 and len(model.crops) == 6
    call = model.joint[0]
    assert call["tiles"] == lat and call["canvas_shape"] == (16, 3, 6, 8) and call["seed"] == 5 and call["num_steps"] == 2
    assert call["init_noise"] is noise and call["guidance"] == 0.0
    for crop, handed, t in zip(model.crops, call["batches"], plan):
        want = rgb[..., t.y:t.y + t.h, t.x:t.x + t.w].to(BF)
        assert torch.equal(crop["rgb"], want) and torch.equal(crop["video"], want) and crop["rgb"].is_contiguous()
        assert set(handed) == {"latent_condition", "context_index"}                  # the pixel crops are dropped
        assert torch.equal(handed["latent_condition"], model.vae.encode(want)) and handed["context_index"].flatten().tolist() == [0, 3]
    assert len(got) == 2 and all(g.shape == (1, T, H, W, 3) and g.dtype == np.uint8 for g in got)
    # the walk decodes crops of the canvas that call returned (a fresh recorder's call 1 returns it again)
    canvas1 = _RecorderModel().generate_samples_joint(call["batches"], lat, (16, 3, 6, 8), 0.0, 5, 2, noise)
    ref = _decode_join(pkg, p, lambda i: canvas1, plan, lat, [False, True], T, H, W)
    assert all(np.array_equal(a, b) for a, b in zip(got, ref)) and not np.array_equal(got[0], got[1])
    # windows: the joint sample of every window over all tiles comes first (windows outside, tiles inside), every window from the
    # same noise; then tiles outside, windows inside
    del model.joint[:], model.crops[:]
    p.window_frames, p.window_overlap = 9, 2
    wins = pkg.windows.plan_windows(T, 9, 2)
    noise = torch.zeros(1, 16, 2, 6, 8)
    got = p.generate_video(dict(batch, context_index=ci[1:2]), normalize_normal=True, seed=5, init_noise=noise, to_host=False)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8
    assert len(model.joint) == len(wins) == 3 and len(model.crops) == 18
    for i, (call, win) in enumerate(zip(model.joint, wins)):
        assert call["canvas_shape"] == (16, 2, 6, 8) and call["tiles"] == lat and call["init_noise"] is noise
        for crop, t in zip(model.crops[6 * i:6 * i + 6], plan):
            assert torch.equal(crop["rgb"], rgb[:, :, win.start:win.start + 9, t.y:t.y + t.h, t.x:t.x + t.w].to(BF))
    rec = _RecorderModel()
    per_window = [rec.generate_samples_joint(c["batches"], lat, (16, 2, 6, 8), 0.0, 5, 2, noise) for c in model.joint]
    (ref,) = _decode_join(pkg, p, lambda i: per_window[i], plan, lat, [True], T, H, W, windows=wins)
    assert np.array_equal(got.numpy(), ref)
    # generate_video_each: the batches of one clip share each tile's crop (one upload, and by the model's cache one encode)
    del model.joint[:], model.crops[:]
    p.window_frames = 0
    each = p.generate_video_each([dict(batch, context_index=ci[0:1]), dict(batch, context_index=ci[1:2])], [False, True], seed=5)
    assert len(each) == 2 and len(model.joint) == 2 and len(model.crops) == 12
    assert [c["rgb"].shape for c in model.crops[0::2]] == [c["rgb"].shape for c in model.crops[1::2]]
    assert [int(c["context_index"][0, 0]) for c in model.crops[:4]] == [0, 3, 0, 3]


def test_overlap_0_is_the_hard_cut_tiling_from_crops_of_the_canvas_noise(pkg, cpu_pipe):
    """Tiles that share no latent are sampled on their own: the joint loop is never called, every tile (one of them shifted back)
    is handed its crop of the one canvas noise, and the bytes are those of "pixel" with these noises handed over by hand."""
    tiles = _tiles(pkg)
    p = cpu_pipe
    model = p.pre_loaded_model_instance
    rgb = pkg.synthetic_weights.synth_tensor("lt.pipe.rgb0", (1, 3, 9, 48, 64), torch.float32, scale=0.6)
    batch = {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[3]], dtype=torch.long)}
    noise = pkg.synthetic_weights.synth_tensor("lt.pipe.xT0", (1, 16, 2, 6, 8), torch.float32, scale=80.0)
    p.tile_height, p.tile_width, p.tile_overlap, p.tile_join = 32, 32, 0, "latent"
    plan = tiles.plan_tiles(48, 64, 32, 32, 0)
    lat = [tiles.latent_tile(t, 8) for t in plan]
    assert [(t.y, t.x, t.ry) for t in lat] == [(0, 0, 0), (0, 4, 0), (2, 0, 2), (2, 4, 2)]
    got = p.generate_video(batch, normalize_normal=True, seed=5, init_noise=noise)
    assert not model.joint and not model.crops and len(model.single) == 4
    for handed, t in zip(model.noises, lat):
        assert torch.equal(handed, noise[..., t.y:t.y + t.h, t.x:t.x + t.w]) and handed.is_contiguous()
    p.tile_join, p.tile_height, p.tile_width = "pixel", 0, 0
    canvas = np.zeros((9, 48, 64, 3), dtype=np.uint8)
    for t, tl in zip(plan, lat):
        c = rgb[..., t.y:t.y + t.h, t.x:t.x + t.w].contiguous()
        o = p.generate_video(dict(batch, rgb=c, video=c), normalize_normal=True, seed=5,
                             init_noise=noise[..., tl.y:tl.y + tl.h, tl.x:tl.x + tl.w].contiguous())
        canvas = R.blend_ref(canvas, o[0], (t.y, t.x, t.ry, t.rx, t.Oy, t.Ox))
    assert np.array_equal(got[0], canvas)
    p.tile_join, p.tile_height, p.tile_width = "latent", 32, 32
    with pytest.raises(ValueError, match="canvas-shaped"):
        p.generate_video(batch, normalize_normal=True, seed=5, init_noise=noise[..., :4, :4].contiguous())


def test_pipeline_refusals(pkg, cpu_pipe):
    p = cpu_pipe
    rgb = torch.zeros(1, 3, 9, 48, 64)
    batch = {"rgb": rgb, "context_index": torch.tensor([[3]])}
    assert p.tile_join == "pixel"
    p.tile_join = "latnet"
    with pytest.raises(ValueError, match="tile_join"):
        p.generate_video(batch)
    p.tile_join = "latent"
    p.tile_height, p.tile_width, p.tile_overlap = 32, 32, 4
    with pytest.raises(ValueError, match="tile_overlap"):
        p.generate_video(batch)
    assert not p.pre_loaded_model_instance.crops and not p.pre_loaded_model_instance.joint
    # one tile, or tiles off: the untiled walk, whatever the overlap
    p.tile_height = p.tile_width = 0
    p.generate_video(batch)
    p.tile_height, p.tile_width = 48, 64
    p.generate_video(batch)
    assert len(p.pre_loaded_model_instance.single) == 2 and not p.pre_loaded_model_instance.joint
    P = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline

    class _Sharded:
        process_group = object()
    s = P("/ckpt", "m.pt", model_instance=_Sharded())
    s.tile_height, s.tile_width, s.tile_join = 32, 32, "latent"
    with pytest.raises(NotImplementedError, match="tile"):
        s.generate_video({"rgb": rgb})


# ----------------------------------------------------------------------------------------------- nodes
class _Recorder:
    """A pipeline that records what the nodes set and hand over."""

    def __init__(self):
        self.device = "cpu"
        self.calls = []

    def set_model_type(self, kind):
        self.kind = kind

    def _out(self, data_batch, to_host):
        ref = data_batch.get("rgb", data_batch.get("depth"))
        B, _, T, H, W = ref.shape
        o = torch.zeros(B, T, H, W, 3, dtype=torch.uint8)
        return o.numpy() if to_host else o

    def generate_video(self, data_batch, normalize_normal=False, seed=None, to_host=True):
        self.calls.append((self.kind, self.tile_join, self.tile_overlap))
        return self._out(data_batch, to_host)

    def generate_video_passes(self, data_batch, normalize_normal, seed=None, to_host=True):
        self.calls.append((self.kind, self.tile_join, self.tile_overlap))
        return [self._out(data_batch, to_host) for _ in normalize_normal]


def test_node_inputs_and_what_the_nodes_set(pkg):
    classes = [pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"], pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"],
               pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]]
    for cls in classes:
        opt = cls.INPUT_TYPES()["optional"]
        assert opt["tile_join"][0] == ["pixel", "latent"] and opt["tile_join"][1]["default"] == "pixel"
        tip = opt["tile_join"][1]["tooltip"]
        assert "agree" in tip and "41 MB" in tip and "multiple of 8" in tip
    sw = pkg.synthetic_weights
    image = sw.synth_tensor("lt.node", (1, 9, 48, 64, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("lt.env", (1, 16, 32, 3), torch.float32).abs()
    inv, fwd, rel = (c() for c in classes)
    r = _Recorder()
    inv.run_inverse_pass(r, image, tile_height=32, tile_width=32, tile_overlap=8, tile_join="latent")
    inv.run_inverse_pass(r, image)                                               # every call sets it
    assert r.calls == [("inverse", "latent", 8), ("inverse", "pixel", 64)]
    r = _Recorder()
    g = [image] * 5
    fwd.run_forward_pass(r, *g, env, tile_height=32, tile_width=32, tile_join="latent")
    fwd.run_forward_pass(r, *g, env)
    assert r.calls == [("forward", "latent", 64), ("forward", "pixel", 64)]
    r = _Recorder()
    rel.run_relight(r, r, image, env, tile_height=32, tile_width=32, tile_overlap=16, tile_join="latent")
    rel.run_relight(r, r, image, env)
    assert r.calls == [("inverse", "latent", 16), ("forward", "latent", 16), ("inverse", "pixel", 64), ("forward", "pixel", 64)]
