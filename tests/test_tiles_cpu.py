"""Spatial tiles on the host: the planner's properties over a grid, the proof that the inputs of tests/test_tiles_gpu.py tell
a wrong blend kernel from a right one, the torch backend against tests/tile_refs.py, and the pipeline's tile walk with a recorder
model against the composition done by hand.  No GPU."""
import importlib

import numpy as np
import pytest
import torch

import tile_refs as R
import window_refs as WR

BF = torch.bfloat16


def _tiles(pkg):
    return importlib.import_module(pkg.__name__ + ".tiles")


# ----------------------------------------------------------------------------------------------- planner
@pytest.mark.parametrize("size", [16, 32, 48, 96, 256, 576, 640])
def test_plan_axis_properties_over_the_grid(pkg, size):
    tiles = _tiles(pkg)
    for Ov in sorted({0, 1, 2, 3, 5, 8, size // 4, size // 2 - 1, size // 2}):
        for n in range(16, 2049, 16):
            plan = tiles.plan_axis(n, size, Ov)
            if n <= size:
                assert plan == [tiles.Span(0, 0)]
                continue
            stride = size - Ov
            count = -(-(n - Ov) // stride)
            assert len(plan) == count >= 2
            assert [s.start for s in plan] == [i * stride for i in range(count - 1)] + [n - size]
            assert plan[-1].start + size == n                                    # the last span ends with the axis
            written = np.zeros(n, dtype=np.int64)
            ramps = []
            for i, s in enumerate(plan):
                assert 0 <= s.start and s.start + size <= n and 0 <= s.ramp_at < size
                assert s.ramp_at == (0 if i == 0 or i < count - 1 else plan[i - 1].start + size - Ov - s.start)
                written[s.start + s.ramp_at:s.start + size] += 1
                if i:
                    lo = s.start + s.ramp_at
                    assert lo == plan[i - 1].start + size - Ov                   # the ramp is the predecessor's last Ov samples
                    assert s.ramp_at + Ov <= size
                    ramps.append((lo, lo + Ov))
            assert (written >= 1).all() and (written <= 2).all()               # every sample is written, none by three spans
            assert all(a[1] <= b[0] for a, b in zip(ramps, ramps[1:]))           # the ramps of one axis are pairwise disjoint
            twice = np.zeros(n, dtype=bool)
            for lo, hi in ramps:
                twice[lo:hi] = True
            # exactly the ramps are written twice - and whatever a shifted-back last span rewrites of its predecessor
            assert (written[twice] == 2).all()


def test_plan_tiles_example_by_hand(pkg):
    tiles = _tiles(pkg)
    T = tiles.Tile
    # 1072 rows in 576: stride 512, ceil(1008 / 512) = 2 spans at 0 and 1072 - 576 = 496; the second's ramp starts at
    # 0 + 576 - 64 - 496 = 16: rows 496 .. 511 are computed and discarded, 512 .. 575 ramp, overlap 1072 - 2 * 576 + ... = 80 rows
    # 1920 columns in 1024: stride 960, 2 spans at 0 and 896; ramp_at = 0 + 1024 - 64 - 896 = 64; the tiles share 128 columns
    assert tiles.plan_axis(1072, 576, 64) == [tiles.Span(0, 0), tiles.Span(496, 16)]
    assert tiles.plan_axis(1920, 1024, 64) == [tiles.Span(0, 0), tiles.Span(896, 64)]
    assert 576 - 496 == 80 and 1024 - 896 == 128
    assert tiles.plan_tiles(1072, 1920, 576, 1024, 64) == [
        T(0, 0, 576, 1024, 0, 0, 0, 0), T(0, 896, 576, 1024, 0, 64, 0, 64),
        T(496, 0, 576, 1024, 16, 0, 64, 0), T(496, 896, 576, 1024, 16, 64, 64, 64)]
    # the GPU pipeline test's clip: 48 x 64 in 32 x 32 at overlap 8 is 2 x 3 tiles
    assert tiles.plan_tiles(48, 64, 32, 32, 8) == [
        T(0, 0, 32, 32, 0, 0, 0, 0), T(0, 24, 32, 32, 0, 0, 0, 8), T(0, 32, 32, 32, 0, 16, 0, 8),
        T(16, 0, 32, 32, 8, 0, 8, 0), T(16, 24, 32, 32, 8, 0, 8, 8), T(16, 32, 32, 32, 8, 16, 8, 8)]
    # one axis only; an axis of 0 or of at least the side is one span of the whole side
    assert tiles.plan_tiles(48, 64, 0, 32, 0) == [T(0, 0, 48, 32, 0, 0, 0, 0), T(0, 32, 48, 32, 0, 0, 0, 0)]
    assert tiles.plan_tiles(48, 64, 64, 32, 8) == tiles.plan_tiles(48, 64, 48, 32, 8) == [
        T(0, 0, 48, 32, 0, 0, 0, 0), T(0, 24, 48, 32, 0, 0, 0, 8), T(0, 32, 48, 32, 0, 16, 0, 8)]
    # one tile in total is "not tiled"
    for th, tw in ((0, 0), (48, 64), (576, 1024), (0, 64), (48, 0)):
        assert tiles.plan_tiles(48, 64, th, tw, 8) is None


@pytest.mark.parametrize("args", [(100, 0, 0), (100, 24, 0), (100, -16, 0), (100, 32, 17), (100, 32, -1), (0, 32, 8), (-5, 32, 8),
                                  (100, 32.0, 8), (100, 32, 1.5), (100, "32", 8), (100, True, 0), (True, 32, 0), (100, 32, False)])
def test_plan_axis_rejects_illegal_arguments(pkg, args):
    with pytest.raises(ValueError):
        _tiles(pkg).plan_axis(*args)


def test_plan_tiles_errors_name_the_input(pkg):
    plan = _tiles(pkg).plan_tiles
    with pytest.raises(ValueError, match="tile_height"):
        plan(100, 100, 24, 32, 8)
    with pytest.raises(ValueError, match="tile_width"):
        plan(100, 100, 32, 40, 8)
    with pytest.raises(ValueError, match="tile_overlap"):
        plan(100, 100, 32, 32, 17)
    with pytest.raises(ValueError, match="tile_overlap"):
        plan(100, 100, 0, 0, -1)
    with pytest.raises(ValueError, match="tile_width"):
        plan(100, 100, 32, 32.0, 8)
    assert plan(100, 100, 0, 0, 64) is None                    # the default overlap beside tiles that are off is no error


# ----------------------------------------------------------------------------------------------- what the case grid can tell
def test_geometry_grid_covers_the_edges():
    for W in R.WIDTHS:
        cases = R.geometry_cases(W)
        assert 20 <= len(cases) <= 700
        for base in range(4):
            seen = set()
            for c in cases:
                seen |= R.segment_residues(W, c, base)
            assert seen == {0, 1, 2, 3}, (W, base)
        geos = [c[4] for c in cases]
        widest = max(w for (_, w) in R.TILES if w <= W)
        assert {(g[4], g[5]) for g in geos} >= {o for o in R.OVERLAPS if o[1] <= widest}      # (all six at W = 19)
        assert any(c[3] - c[4][3] == 1 for c in cases)                           # a written width of one pixel
        assert any(c[2] == c[1] and c[3] == W for c in cases)                     # a tile that covers the canvas exactly
        assert {c[0] for c in cases} == set(R.FRAMES)
        assert {g[2] for g in geos} >= {0, 1} and {g[3] for g in geos} >= {0, 1}
    assert {(3 * W) % 4 for W in R.WIDTHS} == {0, 1, 2, 3}                        # every pitch residue
    assert any(g[4][2] == 4 and g[4][3] == 4 for g in R.geometry_cases(19))


def test_geometry_grid_separates_every_wrong_kernel():
    """Every stand-in but the two rounding ones (the value grid's business) changes bytes of the geometry grid at every width
    that has room for it."""
    for W in R.WIDTHS:
        hits = {v: 0 for v in R.VARIANTS}
        for i, case in enumerate(R.geometry_cases(W)):
            canvas, tile = R.case_inputs(W, i, case)
            ref = R.blend_ref(canvas, tile, case[4])
            for v in R.VARIANTS:
                hits[v] += int((R.blend_ref(canvas, tile, case[4], variant=v) != ref).sum())
        for v in R.VARIANTS:
            assert hits[v] > 0, (W, v)


@pytest.mark.parametrize("Ov", R.GRID_OVERLAPS)
def test_value_grid_separates_the_rounding_stand_ins(Ov):
    """The 256 x 256 byte-pair grid under every weight of the pair.  Round half up, truncation, min(wy, wx) and the other weight
    stand-ins differ at every pair; a * (1 - w) + b * w differs at (5, 3).
    The fused blend (fma: the product w * (b - a) not rounded before the add) gives the same bytes at (1, 1) and (3, 3), where
    every weight is dyadic and the product is exact - there the grid can NOT tell it.  At (5, 3) it can: with wy = fp32(k / 6) the
    rounded product lands on exact .5 ties that the unrounded one misses (598 bytes of this grid)."""
    canvas, tile, geo = R.value_grid(*Ov)
    pairs = set(zip(canvas[:, 0, 0].reshape(-1).tolist(), tile[:, 0, 0].reshape(-1).tolist()))
    assert len(pairs) == 65536
    ref = R.blend_ref(canvas, tile, geo)
    assert np.array_equal(ref[:, 0], canvas[:, 0]) and np.array_equal(ref[:, :, :2], canvas[:, :, :2])      # outside: untouched
    assert np.array_equal(ref[:, 1 + Ov[0], 2 + Ov[1]], tile[:, 0, 0])                                     # behind both ramps: copied
    changed = {v: int((R.blend_ref(canvas, tile, geo, variant=v) != ref).sum()) for v in R.VARIANTS + R.NEAR_VARIANTS}
    print(f"value grid {Ov}: {changed}")
    assert changed["half_up"] > 0 and changed["trunc"] > 0 and changed["min_w"] > 0 and changed["w_j_over_O"] > 0
    assert changed["sum_w"] > 0
    if Ov == (5, 3):
        assert changed["lerp2"] > 0 and changed["fma"] > 0
    else:
        assert changed["fma"] == 0


# ----------------------------------------------------------------------------------------------- the torch backend
def _as5(a, frames):
    return torch.from_numpy(a).reshape(*frames, *a.shape[1:])


@pytest.mark.parametrize("W", R.WIDTHS)
def test_torch_backend_is_the_reference(pkg, W):
    tiles = _tiles(pkg)
    for i, case in enumerate(R.geometry_cases(W)):
        frames, H, h, w, geo = case
        canvas, tile = R.case_inputs(W, i, case)
        c5 = _as5(canvas.copy(), frames)
        t = tiles.Tile(geo[0], geo[1], h, w, *geo[2:])
        got = tiles.blend_tile(c5, _as5(tile, frames), t)
        assert got is c5
        assert np.array_equal(c5.reshape(canvas.shape).numpy(), R.blend_ref(canvas, tile, geo)), case


def test_torch_backend_on_the_value_grid(pkg):
    tiles = _tiles(pkg)
    canvas, tile, geo = R.value_grid(5, 3)
    c5 = torch.from_numpy(canvas.copy())[None]
    tiles.blend_tile(c5, torch.from_numpy(tile)[None], tiles.Tile(geo[0], geo[1], 6, 4, *geo[2:]), backend="torch")
    assert np.array_equal(c5[0].numpy(), R.blend_ref(canvas, tile, geo))


def test_blend_tile_checks_and_dispatch(pkg):
    tiles = _tiles(pkg)
    c = torch.zeros(1, 1, 8, 8, 3, dtype=torch.uint8)
    t = torch.zeros(1, 1, 4, 4, 3, dtype=torch.uint8)
    ok = tiles.Tile(2, 2, 4, 4, 1, 1, 2, 2)
    tiles.blend_tile(c, t, ok)
    with pytest.raises(ValueError, match="hip"):
        tiles.blend_tile(c, t, ok, backend="hip")
    with pytest.raises(ValueError, match="backend"):
        tiles.blend_tile(c, t, ok, backend="cuda")
    for bad in (ok._replace(y=5), ok._replace(x=-1), ok._replace(h=5), ok._replace(ry=4), ok._replace(rx=-1), ok._replace(Oy=4),
                ok._replace(Ox=-1)):
        with pytest.raises(ValueError):
            tiles.blend_tile(c, t, bad)
    with pytest.raises(ValueError):
        tiles.blend_tile(c.float(), t, ok)
    with pytest.raises(ValueError):
        tiles.blend_tile(c, t.expand(2, 1, 4, 4, 3), ok)


# ----------------------------------------------------------------------------------------------- the pipeline's walk
class _RecorderModel:
    """Stands in for the renderer model: records the batches it is handed; a "sample" is the clip scaled per pass plus a ramp
    over the sample's own rows, columns and frames - two tiles disagree where they overlap, as real tiles do."""
    process_group = None
    net = None

    def __init__(self):
        self.config = {}
        self.seen = []

    def to(self, device):
        return self

    def generate_samples_from_batch(self, data_batch, guidance, state_shape, num_steps, is_negative_prompt, seed, init_noise):
        self.seen.append({k: v.clone() for k, v in data_batch.items() if isinstance(v, torch.Tensor)})
        clip = data_batch["rgb"].float()
        T, H, W = clip.shape[2:]
        local = torch.linspace(-0.4, 0.4, H).view(H, 1) + torch.linspace(-0.3, 0.3, W).view(1, W)
        local = local + torch.linspace(-0.2, 0.2, T).view(T, 1, 1)               # (and two windows, in time)
        rows = [clip * (0.9 - 0.15 * int(ci)) + local + 0.001 * (seed or 0) for ci in data_batch["context_index"].reshape(-1)]
        return torch.cat(rows).to(BF)

    def decode(self, sample):
        return sample


@pytest.fixture()
def cpu_pipe(pkg, monkeypatch):
    """A pipeline on the CPU: the recorder model, and the uint8 post-process kernel replaced by its CPU reference."""
    mod = pkg.diffusion_renderer_pipeline

    def post(video, prev, ramp, ramp_at, lo, hi, normalize, out=None):
        return WR.blend_postprocess(video, prev, ramp, ramp_at, lo, hi, normalize)
    monkeypatch.setattr(mod.N, "postprocess_window_u8", post)
    model = _RecorderModel()
    p = mod.CleanDiffusionRendererPipeline("/nonexistent", "x.pt", model_type=None, model_instance=model, guidance=0.0, num_steps=2)
    p.device = torch.device("cpu")
    p.set_model_type("inverse")
    return p


def _clip(pkg, T, H, W, name="tiles.rgb"):
    return pkg.synthetic_weights.synth_tensor(name, (1, 3, T, H, W), torch.float32, scale=0.6)


def _by_hand(pkg, p, call, batches_of, H, W, tile_args):
    """The tiled result composed outside the pipeline: `call(batches)` (tiles off, no restore plan, results on the host) on every
    crop, joined by the numpy reference.  batches_of(crop) crops every picture-sized tensor; -> the canvases, one per result."""
    tiles = _tiles(pkg)
    keep = (p.tile_height, p.tile_width, p.restore_plan)
    p.tile_height = p.tile_width = 0
    p.restore_plan = None
    canvases = None
    for t in tiles.plan_tiles(H, W, *tile_args):
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


def test_tiled_pipeline_is_the_composition_by_hand(pkg, cpu_pipe):
    p = cpu_pipe
    T, H, W, args = 9, 48, 64, (32, 32, 8)
    rgb = _clip(pkg, T, H, W)
    ci = torch.tensor([[0], [3]], dtype=torch.long)
    p.tile_height, p.tile_width, p.tile_overlap = args

    def batch(crop, idx):
        c = crop(rgb)
        return {"rgb": c, "video": c, "context_index": idx}
    whole = lambda v: v
    # generate_video; the crops the model is handed are the planned tiles of the clip, in raster order
    got = p.generate_video(batch(whole, ci[1:2]), normalize_normal=True, seed=5)
    plan = _tiles(pkg).plan_tiles(H, W, *args)
    seen = p.pre_loaded_model_instance.seen
    assert len(seen) == len(plan) == 6
    for s, t in zip(seen, plan):
        want = rgb[..., t.y:t.y + t.h, t.x:t.x + t.w].to(BF)
        assert torch.equal(s["rgb"], want) and torch.equal(s["video"], want) and s["rgb"].is_contiguous()
    (ref,) = _by_hand(pkg, p, lambda b: [p.generate_video(b, normalize_normal=True, seed=5)], lambda crop: batch(crop, ci[1:2]),
                      H, W, args)
    assert got.shape == (1, T, H, W, 3) and got.dtype == np.uint8 and np.array_equal(got, ref)
    # tiles disagree where they meet, so the join is a real cross-fade: hard cuts give other bytes
    p.tile_overlap = 0
    assert not np.array_equal(p.generate_video(batch(whole, ci[1:2]), normalize_normal=True, seed=5), ref)
    p.tile_overlap = 8
    # generate_video_passes and generate_video_each
    flags = [False, True]
    got = p.generate_video_passes(batch(whole, ci), normalize_normal=flags, seed=5)
    ref = _by_hand(pkg, p, lambda b: p.generate_video_passes(b, normalize_normal=flags, seed=5), lambda crop: batch(crop, ci),
                   H, W, args)
    assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(got, ref)) and not np.array_equal(got[0], got[1])
    del seen[:]
    each = p.generate_video_each([batch(whole, ci[0:1]), dict(batch(whole, ci[1:2]))], flags, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip(each, ref))
    assert len(seen) == 12


def test_tiles_share_one_crop_per_tensor(pkg, cpu_pipe, monkeypatch):
    """rgb and video are one tensor, and the batches of generate_video_each share the clip: one crop per tile and tensor."""
    p = cpu_pipe
    rgb = _clip(pkg, 9, 48, 64)
    ci = torch.tensor([[0], [3]], dtype=torch.long)
    p.tile_height, p.tile_width, p.tile_overlap = 32, 32, 8
    handed = []
    real = p._walk

    def spy(batches, *a, **k):
        handed.append(batches)
        return real(batches, *a, **k)
    monkeypatch.setattr(p, "_walk", spy)
    p.generate_video_each([{"rgb": rgb, "video": rgb, "context_index": ci[k:k + 1]} for k in range(2)], [False, True], seed=1)
    assert len(handed) == 6
    for batches in handed:
        assert len({id(b[k]) for b in batches for k in ("rgb", "video")}) == 1
        assert batches[0]["context_index"] is ci[0:1] or torch.equal(batches[0]["context_index"], ci[0:1])


def test_tiles_with_windows_restore_and_device_results(pkg, cpu_pipe):
    fit = importlib.import_module(pkg.__name__ + ".fit")
    p = cpu_pipe
    T, H, W, args = 17, 48, 64, (32, 32, 8)
    rgb = _clip(pkg, T, H, W, "tiles.rgbw")
    ci = torch.tensor([[3]], dtype=torch.long)
    batch = lambda crop: {"rgb": crop(rgb), "context_index": ci}
    whole = lambda v: v
    p.tile_height, p.tile_width, p.tile_overlap = args
    call = lambda b: [p.generate_video(b, normalize_normal=True, seed=2)]
    # windows inside every tile
    p.window_frames, p.window_overlap = 9, 2
    (ref_w,) = _by_hand(pkg, p, call, batch, H, W, args)
    got = p.generate_video(batch(whole), normalize_normal=True, seed=2)
    assert got.shape == (1, T, H, W, 3) and np.array_equal(got, ref_w)
    p.window_frames = 0
    (ref,) = _by_hand(pkg, p, call, batch, H, W, args)
    assert not np.array_equal(ref, ref_w)
    # the restore plan runs once, on the joined picture, and cuts the time padding; to_host=False hands back the tensor
    plan = fit.plan_fit(12, 60, 56, "stretch", H, W)
    assert (plan.T, plan.T_out) == (12, 17)
    p.restore_plan = fit.plan_restore(plan)
    want = fit.restore_frames(torch.from_numpy(ref), p.restore_plan)
    got = p.generate_video(batch(whole), normalize_normal=True, seed=2)
    assert got.shape == (1, 12, 60, 56, 3) and np.array_equal(got, want.numpy())
    assert p.restore_plan is not None
    dev = p.generate_video(batch(whole), normalize_normal=True, seed=2, to_host=False)
    assert isinstance(dev, torch.Tensor) and dev.dtype == torch.uint8 and torch.equal(dev, want)
    p.restore_plan = None
    dev = p.generate_video(batch(whole), normalize_normal=True, seed=2, to_host=False)
    assert isinstance(dev, torch.Tensor) and np.array_equal(dev.numpy(), ref)


def test_one_tile_and_tiles_off_are_the_untiled_call(pkg, cpu_pipe, monkeypatch):
    p = cpu_pipe
    rgb = _clip(pkg, 9, 48, 64)
    batch = {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[3]], dtype=torch.long)}
    off = torch.from_numpy(p.generate_video(batch, normalize_normal=True, seed=4))
    blends = []
    mod = pkg.diffusion_renderer_pipeline
    monkeypatch.setattr(mod, "blend_tile", lambda *a, **k: blends.append(a))
    for th, tw in ((48, 64), (64, 64), (576, 1024), (0, 64), (48, 0)):
        p.tile_height, p.tile_width = th, tw
        assert torch.equal(torch.from_numpy(p.generate_video(batch, normalize_normal=True, seed=4)), off), (th, tw)
    assert not blends
    assert len(p.pre_loaded_model_instance.seen) == 6 and all(s["rgb"].shape[3:] == (48, 64) for s in p.pre_loaded_model_instance.seen)
    p.tile_height, p.tile_width, p.tile_overlap = 32, 32, 20
    with pytest.raises(ValueError, match="tile_overlap"):
        p.generate_video(batch)
    p.tile_height, p.tile_overlap = 40, 8
    with pytest.raises(ValueError, match="tile_height"):
        p.generate_video(batch)


def test_tiles_under_sequence_parallelism_are_refused(pkg):
    P = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline

    class _Sharded:
        process_group = object()
    p = P("/ckpt", "m.pt", model_instance=_Sharded())
    p.tile_height, p.tile_width = 32, 32
    with pytest.raises(NotImplementedError, match="tile"):
        p.generate_video({"rgb": torch.zeros(1, 3, 9, 48, 64)})


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

    def _note(self, data_batch):
        ref = data_batch.get("rgb", data_batch.get("depth"))
        self.calls.append((self.kind, self.tile_height, self.tile_width, self.tile_overlap, tuple(ref.shape[3:])))

    def generate_video(self, data_batch, normalize_normal=False, seed=None, to_host=True):
        self._note(data_batch)
        return self._out(data_batch, to_host)

    def generate_video_passes(self, data_batch, normalize_normal, seed=None, to_host=True):
        self._note(data_batch)
        return [self._out(data_batch, to_host) for _ in normalize_normal]


def test_node_inputs_and_pipeline_attributes(pkg):
    P = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline
    p = P("/ckpt", "m.pt")
    assert (p.tile_height, p.tile_width, p.tile_overlap) == (0, 0, 64)
    assert len(pkg.NODE_CLASS_MAPPINGS) == 4
    classes = [pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"], pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"],
               pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]]
    for cls in classes:
        opt = cls.INPUT_TYPES()["optional"]
        for name in ("tile_height", "tile_width"):
            assert opt[name][0] == "INT" and opt[name][1]["default"] == 0 and opt[name][1]["step"] == 16
        assert opt["tile_overlap"][0] == "INT" and opt["tile_overlap"][1]["default"] == 64
        tip = opt["tile_height"][1]["tooltip"]
        assert "576 x 1024" in tip and "fitted" in tip.lower() and "independent samples" in tip
    sw = pkg.synthetic_weights
    image = sw.synth_tensor("tiles.node", (1, 9, 48, 64, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("tiles.env", (1, 16, 32, 3), torch.float32).abs()
    inv, fwd, rel = (c() for c in classes)
    r = _Recorder()
    inv.run_inverse_pass(r, image, tile_height=32, tile_width=48, tile_overlap=8)
    assert r.calls == [("inverse", 32, 48, 8, (48, 64))]
    inv.run_inverse_pass(r, image)                                               # every call sets the three attributes
    assert r.calls[-1] == ("inverse", 0, 0, 64, (48, 64))
    r = _Recorder()
    g = [image] * 5
    fwd.run_forward_pass(r, *g, env, tile_height=32, tile_width=32, tile_overlap=4)
    fwd.run_forward_pass(r, *g, env)
    assert r.calls == [("forward", 32, 32, 4, (48, 64)), ("forward", 0, 0, 64, (48, 64))]
    # the relight node tiles both stages; tiles apply to the fitted picture
    r = _Recorder()
    rel.run_relight(r, r, image, env, fit="stretch", fit_height=32, fit_width=48, tile_height=16, tile_width=32, tile_overlap=2)
    assert r.calls == [("inverse", 16, 32, 2, (32, 48)), ("forward", 16, 32, 2, (32, 48))]
