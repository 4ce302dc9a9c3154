"""Long clips on the GPU: drn_postprocess_window_u8 bit for bit against tests/window_refs.py (whose inputs
tests/test_windows_cpu.py shows to separate the wrong kernels), its argument checks, and the windowed pipeline and nodes
against the composition done by hand."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import window_refs as R
from conftest import tiny_net
from oracle import dit_oracle as O
from stub_vae import StubVAE

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD, SENTINEL = 64, 0xA5          # 64 bytes keep the guarded output 8-byte aligned: the 8-pixel path stays the one under test
DRN_EINVAL = -1


def _launch(pkg, gpu, video, prev, w, geo, normalize, guard=GUARD):
    """The kernel into a guard-banded buffer, issued twice (a rerun over its own output changes nothing) -> the result on the CPU;
    the guard bands are checked here."""
    ramp_at, lo, hi = geo
    B, _, _, H, W = video.shape
    n = B * (hi - lo) * H * W * 3
    buf = torch.full((guard + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    out = buf[guard:guard + n].view(B, hi - lo, H, W, 3)
    for _ in range(2):
        pkg.native.postprocess_window_u8(video, prev, w, ramp_at, lo, hi, normalize, out=out)
    host = buf.cpu()
    assert (host[:guard] == SENTINEL).all() and (host[guard + n:] == SENTINEL).all(), "wrote outside its output"
    return host[guard:guard + n].view(B, hi - lo, H, W, 3)


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_window_kernel_bit_exact(pkg, gpu, H, W):
    launches = 0
    for B in (1, 2):
        for Ov in R.OVERLAPS:
            video, prev = R.case_inputs(B, H, W, Ov)
            w = R.ramp_table(pkg, Ov) if Ov else None
            vd, pd, wd = video.to(gpu), None if prev is None else prev.to(gpu), None if w is None else w.to(gpu)
            for geo in R.case_geometries(Ov):
                for normalize in (False, True):
                    got = _launch(pkg, gpu, vd, pd, wd, geo, normalize)
                    ref = R.blend_postprocess(video, prev, w, *geo, normalize)
                    assert torch.equal(got, ref), (f"B{B} {H}x{W} O={Ov} ramp_at/lo/hi={geo} normalize={normalize}: "
                                                   f"{int((got != ref).sum())} of {ref.numel()} bytes differ")
                    launches += 1
    print(f"window kernel {H}x{W}: {launches} cases bit-exact")


@pytest.mark.parametrize("Ov", R.GRID_OVERLAPS)
def test_window_kernel_value_grid(pkg, gpu, Ov):
    """Every finite bf16 value in [-4, 4] as a carry value under every weight of the table, plus the pairs that land on bf16
    ties: the case test_windows_cpu shows to change bytes under a fused blend."""
    video, prev = R.value_grid(Ov)
    w = R.ramp_table(pkg, Ov)
    vd, pd, wd = video.to(gpu), prev.to(gpu), w.to(gpu)
    for normalize in (False, True):
        got = _launch(pkg, gpu, vd, pd, wd, (0, 0, R.TW), normalize)
        ref = R.blend_postprocess(video, prev, w, 0, 0, R.TW, normalize)
        assert torch.equal(got, ref), f"O={Ov} normalize={normalize}: {int((got != ref).sum())} of {ref.numel()} bytes differ"


def test_window_kernel_unaligned_buffers_take_the_pixel_path(pkg, gpu):
    """An output that is not 8-byte aligned, or a window / carry that is not 16-byte aligned, at a shape of whole 8-pixel groups:
    same bytes."""
    video, prev = R.case_inputs(2, 8, 12, 2)
    w = R.ramp_table(pkg, 2)
    ref = R.blend_postprocess(video, prev, w, 3, 3, R.TW, True)
    vd, pd, wd = video.to(gpu), prev.to(gpu), w.to(gpu)
    assert torch.equal(_launch(pkg, gpu, vd, pd, wd, (3, 3, R.TW), True, guard=61), ref)

    def shifted(t):                                    # the same values 2 bytes past an aligned address
        flat = torch.empty(t.numel() + 1, dtype=BF, device=gpu)
        flat[1:] = t.reshape(-1)
        return flat[1:].view(t.shape)
    assert torch.equal(_launch(pkg, gpu, shifted(vd), pd, wd, (3, 3, R.TW), True), ref)
    assert torch.equal(_launch(pkg, gpu, vd, shifted(pd), wd, (3, 3, R.TW), True), ref)


@pytest.mark.parametrize("normalize", [False, True])
def test_window_kernel_without_a_ramp_is_postprocess_u8(pkg, gpu, normalize):
    """drn_postprocess_u8 is the window kernel with no carry over every frame: both against the CPU reference of the chain."""
    for (H, W) in ((8, 12), (5, 7), (64, 64)):
        cpu = pkg.synthetic_weights.synth_tensor(f"win.id.{H}", (2, 3, R.TW, H, W), torch.float32, scale=0.8).to(BF)
        video = cpu.to(gpu)
        ref = O.postprocess(cpu, normalize)
        assert torch.equal(pkg.native.postprocess_u8(video, normalize).cpu(), ref)
        assert torch.equal(pkg.native.postprocess_window_u8(video, None, None, 0, 0, R.TW, normalize).cpu(), ref)
        assert torch.equal(pkg.native.postprocess_window_u8(video, None, None, 3, 2, 7, normalize).cpu(), ref[:, 2:7])


def test_window_kernel_argument_checks(pkg, gpu):
    lib = pkg.native.load_library()
    Tw, H, W, Ov = R.TW, 8, 8, 2
    video = torch.zeros((1, 3, Tw, H, W), dtype=BF, device=gpu)
    prev = torch.zeros((1, 3, Ov, H, W), dtype=BF, device=gpu)
    w = R.ramp_table(pkg, Ov).to(gpu)
    n = Tw * H * W * 3
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    out = buf[GUARD:].data_ptr()
    v, p, r = video.data_ptr(), prev.data_ptr(), w.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream

    def call(video=v, prev=p, ramp=r, out=out, O_=Ov, ramp_at=0, lo=0, hi=Tw):
        return lib.drn_postprocess_window_u8(video, prev, ramp, out, 1, Tw, H, W, O_, ramp_at, lo, hi, 0, stream)
    bad = {
        "null video": dict(video=None), "null out": dict(out=None),
        "carry without weights": dict(ramp=None), "weights without carry": dict(prev=None),
        "O < 0": dict(O_=-1), "ramp_at < 0": dict(ramp_at=-1), "ramp past the window": dict(ramp_at=Tw - 1),
        "write_lo < 0": dict(lo=-1), "empty range": dict(lo=4, hi=4), "reversed range": dict(lo=5, hi=4),
        "write_hi past the window": dict(hi=Tw + 1), "write_lo inside the ramp": dict(ramp_at=3, lo=4),
    }
    for name, kw in bad.items():
        assert call(**kw) == DRN_EINVAL, name
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all(), "a rejected call wrote"
    # the neighbours of the rejected ramp positions are accepted
    assert call(ramp_at=3, lo=3) == 0 and call(ramp_at=3, lo=5) == 0 and call(ramp_at=Tw - Ov) == 0
    assert call(prev=None, ramp=None, O_=0) == 0
    torch.cuda.synchronize()
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all()


# ----------------------------------------------------------------------------------------------- pipeline
class _RaggedStubVAE(StubVAE):
    """StubVAE for clip lengths that are not 8k + 1: like the real tokenizer's (T - 1) // 8 + 1 latent frames, the frames past the
    last whole group of 8 are dropped (the stub's own reshape needs whole groups).  Identical to StubVAE at 8k + 1."""

    def encode(self, x):
        return super().encode(x[:, :, :1 + 8 * ((x.shape[2] - 1) // 8)])


def _pipeline(pkg, gpu, vae, steps=2):
    sw = pkg.synthetic_weights
    net = tiny_net(pkg, 256, 1, 2)
    cfg = pkg.diffusion_renderer_config.get_inverse_renderer_config()
    cfg["net"] = dict(net)
    model = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=gpu)
    model.load_state_dict(sw.synth_state_dict(net, BF, device=gpu), strict=True)
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=vae, model_instance=model, guidance=0.0, num_steps=steps)
    p.device = gpu
    p.set_model_type("inverse")
    return p


def _by_hand(pkg, p, rgb, cis, flags, seed, noise, Wf, Ov):
    """The windowed clip composed outside the pipeline: _sample + decode per planned window, the CPU blend reference."""
    T = rgb.shape[2]
    plan = pkg.windows.plan_windows(T, Wf, Ov)
    w = R.ramp_table(pkg, Ov) if Ov else None
    outs = [np.zeros((1, T, rgb.shape[3], rgb.shape[4], 3), dtype=np.uint8) for _ in flags]
    carry = [None] * len(flags)
    keep = (p.window_frames, p.window_overlap)
    p.window_frames = 0
    for i, win in enumerate(plan):
        clip = rgb[:, :, win.start:win.start + Wf].contiguous()
        sample = p._sample({"rgb": clip, "video": clip, "context_index": cis}, seed, noise)
        for k, flag in enumerate(flags):
            video = p.model.decode(sample[k:k + 1]).to(BF).cpu()
            prev = carry[k] if i > 0 and Ov else None
            u8 = R.blend_postprocess(video, prev, w if prev is not None else None, win.ramp_at, win.write_lo, win.write_hi, flag)
            outs[k][:, win.out_at:win.out_at + u8.shape[1]] = u8.numpy()
            carry[k] = video[:, :, Wf - Ov:].contiguous()
    p.window_frames, p.window_overlap = keep
    return outs


def test_windowed_generate_video_is_the_composition_by_hand(pkg, gpu):
    sw = pkg.synthetic_weights
    p = _pipeline(pkg, gpu, _RaggedStubVAE())
    T, Wf, Ov, seed = 21, 9, 2, 5
    rgb = sw.synth_tensor("win.rgb", (1, 3, T, 64, 64), torch.float32, scale=1.0)
    noise = sw.synth_tensor("win.xT", (1, 16, 2, 8, 8), torch.float32, scale=80.0)
    ci = torch.full((1, 1), 3, dtype=torch.long)
    batch = {"rgb": rgb, "video": rgb, "context_index": ci}

    p.window_frames, p.window_overlap = Wf, Ov
    for normalize in (False, True):
        got = p.generate_video(batch, normalize_normal=normalize, seed=seed, init_noise=noise)
        (ref,) = _by_hand(pkg, p, rgb, ci, [normalize], seed, noise, Wf, Ov)
        assert got.shape == (1, T, 64, 64, 3) and got.dtype == np.uint8
        assert np.array_equal(got, ref), f"normalize={normalize}: {(got != ref).sum()} bytes differ"
    # without init_noise every window draws the same start noise from the seed
    a = p.generate_video(batch, normalize_normal=True, seed=seed)
    (b,) = _by_hand(pkg, p, rgb, ci, [True], seed, None, Wf, Ov)
    assert np.array_equal(a, b)
    # overlap 0: hard cuts, the shifted last window writes only its last 3 frames
    p.window_overlap = 0
    (cut,) = _by_hand(pkg, p, rgb, ci, [True], seed, noise, Wf, 0)
    assert np.array_equal(p.generate_video(batch, normalize_normal=True, seed=seed, init_noise=noise), cut)
    assert not np.array_equal(cut, ref)                 # (ref: the cross-faded normal pass of the loop above)

    # a clip that fits one window takes today's path
    p.window_frames, p.window_overlap = Wf, Ov
    short = {"rgb": rgb[:, :, :9].contiguous(), "context_index": ci}
    short["video"] = short["rgb"]
    on = p.generate_video(short, normalize_normal=True, seed=seed, init_noise=noise)
    p.window_frames = 0
    off = p.generate_video(short, normalize_normal=True, seed=seed, init_noise=noise)
    assert np.array_equal(on, off) and on.shape == (1, 9, 64, 64, 3)

    # windows off at T = 21: today's output (one sequence of 3 latent frames), bit for bit
    noise3 = sw.synth_tensor("win.xT3", (1, 16, 3, 8, 8), torch.float32, scale=80.0)
    today = p.generate_video(batch, normalize_normal=True, seed=seed, init_noise=noise3)
    sample = p._sample(batch, seed, noise3)
    ref = O.postprocess(p.model.decode(sample).to(BF).cpu(), True).numpy()
    assert np.array_equal(today, ref) and today.shape[1] == 17


def test_windowed_passes_match_the_passes_run_singly(pkg, gpu):
    sw = pkg.synthetic_weights
    p = _pipeline(pkg, gpu, _RaggedStubVAE())
    T, Wf, Ov, seed = 21, 9, 2, 9
    rgb = sw.synth_tensor("winp.rgb", (1, 3, T, 64, 64), torch.float32, scale=1.0)
    p.window_frames, p.window_overlap = Wf, Ov
    idx = torch.tensor([[0], [3]], dtype=torch.long)
    both = p.generate_video_passes({"rgb": rgb, "video": rgb, "context_index": idx}, normalize_normal=[False, True], seed=seed)
    assert len(both) == 2
    singles, each_batches = [], []
    for k, flag in ((0, False), (1, True)):
        b = {"rgb": rgb, "video": rgb, "context_index": idx[k:k + 1]}
        each_batches.append(b)
        singles.append(p.generate_video(b, normalize_normal=flag, seed=seed))
    for a, b in zip(both, singles):
        assert a.shape == (1, T, 64, 64, 3) and np.array_equal(a, b)
    assert not np.array_equal(both[0], both[1])
    each = p.generate_video_each(each_batches, [False, True], seed=seed)          # windows outside, passes inside
    assert all(np.array_equal(a, b) for a, b in zip(each, singles))
    with pytest.raises(ValueError, match="normalize_normal flags"):
        p.generate_video_passes({"rgb": rgb, "video": rgb, "context_index": idx}, normalize_normal=[False])


def test_generate_video_of_a_batch_of_clips(pkg, gpu, monkeypatch):
    """Windows off, a sample of two different clips: one decode, one flag, one host buffer of B = 2, byte for byte the chain by hand.
    The renderer model itself samples one clip per call (its noise is drawn with batch 1, as in the reference), so the two-clip
    sample is the two clips' samples stacked and stands in for _sample; everything after it is the pipeline's own walk."""
    sw = pkg.synthetic_weights
    p = _pipeline(pkg, gpu, StubVAE())
    rgb = sw.synth_tensor("winb.rgb", (2, 3, 9, 64, 64), torch.float32, scale=1.0)
    batch = {"rgb": rgb, "video": rgb, "context_index": torch.full((2, 1), 3, dtype=torch.long)}
    with pytest.raises(ValueError, match="one clip per call"):
        p.generate_video(batch, seed=7)
    rows = []
    for k in range(2):
        clip = rgb[k:k + 1].contiguous()
        rows.append(p._sample({"rgb": clip, "video": clip, "context_index": batch["context_index"][k:k + 1]}, 7, None))
    sample = torch.cat(rows)
    monkeypatch.setattr(p, "_sample", lambda *a, **k: sample)
    video = p.model.decode(p._sample(batch, 7, None)).to(BF).cpu()
    for normalize in (False, True):
        got = p.generate_video(batch, normalize_normal=normalize, seed=7)
        ref = O.postprocess(video, normalize).numpy()
        assert got.shape == (2, 9, 64, 64, 3) and got.dtype == np.uint8
        assert np.array_equal(got, ref), f"normalize={normalize}: {(got != ref).sum()} bytes differ"
    assert not np.array_equal(got[0], got[1])


def test_restore_through_one_window(pkg, gpu):
    """A clip padded in time by the fit (12 -> 17 frames) with a restore plan: the whole-clip window restores what it wrote and
    keeps the plan's 12 frames, with windows off and with one window of 17."""
    fit = importlib.import_module(pkg.__name__ + ".fit")
    p = _pipeline(pkg, gpu, _RaggedStubVAE())
    image = pkg.synthetic_weights.synth_tensor("winr.img", (1, 12, 40, 36, 3), torch.float32).abs().clamp(max=1.0)
    plan = fit.plan_fit(12, 40, 36, "stretch", 32, 32)
    clip = fit.fit_frames(image, plan, device=gpu)
    assert clip.shape == (1, 3, 17, 32, 32)
    batch = {"rgb": clip, "video": clip, "context_index": torch.full((1, 1), 3, dtype=torch.long)}
    p.restore_plan = fit.plan_restore(plan)
    sample = p._sample(batch, 5, None)
    u8 = pkg.native.postprocess_u8(p.model.decode(sample).to(BF).contiguous(), True)
    ref = fit.restore_frames(u8, p.restore_plan).cpu().numpy()
    assert u8.shape == (1, 17, 32, 32, 3) and ref.shape == (1, 12, 40, 36, 3)
    off = p.generate_video(batch, normalize_normal=True, seed=5)
    assert np.array_equal(off, ref), f"{(off != ref).sum()} bytes differ"
    p.window_frames = 17
    assert len(pkg.windows.plan_windows(17, p.window_frames, p.window_overlap)) == 1
    assert np.array_equal(p.generate_video(batch, normalize_normal=True, seed=5), ref)


# ----------------------------------------------------------------------------------------------- nodes
def test_inverse_node_windowed_with_hip_tokenizer(pkg, gpu):
    sw = pkg.synthetic_weights
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=gpu), device=gpu)
    encodes = []
    real_encode = vae.encode

    def counting(x, *a, **k):
        encodes.append(tuple(x.shape))
        return real_encode(x, *a, **k)
    vae.encode = counting
    p = _pipeline(pkg, gpu, vae)
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    image = sw.synth_tensor("winnode.img", (1, 21, 64, 64, 3), torch.float32).abs()
    outs = node.run_inverse_pass(p, image, guidance=0.0, seed=3, window_frames=9, window_overlap=2)
    assert len(outs) == 5 and encodes == [(1, 3, 9, 64, 64)] * 3                    # one encode per window
    for o in outs:
        assert o.shape == (21, 64, 64, 3) and o.dtype == torch.float32
        assert 0.0 <= o.min() and o.max() <= 1.0 and torch.equal(o, torch.round(o * 255) / 255)
    # window 0 alone: the node on the first 9 frames gives frames [0, 7) (it writes up to its carry)
    head = node.run_inverse_pass(p, image[:, :9].contiguous(), guidance=0.0, seed=3, window_frames=9, window_overlap=2)
    for a, b in zip(outs, head):
        assert b.shape == (9, 64, 64, 3) and torch.equal(a[:7], b[:7])
    # reproducible from its seed
    again = node.run_inverse_pass(p, image, guidance=0.0, seed=3, window_frames=9, window_overlap=2)
    assert all(torch.equal(a, b) for a, b in zip(outs, again))
    # passes one after the other: windows outside, passes inside - same bits, still one encode per window
    del encodes[:]
    p.batch_passes = False
    seq = node.run_inverse_pass(p, image, guidance=0.0, seed=3, window_frames=9, window_overlap=2)
    p.batch_passes = True
    assert encodes == [(1, 3, 9, 64, 64)] * 3
    for name, a, b in zip(("basecolor", "metallic", "roughness", "normal", "depth"), outs, seq):
        assert torch.equal(a, b), name
    assert not torch.equal(outs[0], outs[3])
    with pytest.raises(ValueError, match="window_frames"):
        node.run_inverse_pass(p, image, guidance=0.0, seed=3, window_frames=12, window_overlap=2)


def test_forward_node_windowed(pkg, gpu):
    sw = pkg.synthetic_weights
    cfgm = pkg.diffusion_renderer_config
    net = tiny_net(pkg, 256, 1, 2, forward=True)
    cfg = cfgm.get_forward_renderer_config()
    cfg["net"] = dict(net)
    cfg["model_type"] = "forward"
    model = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=gpu)
    model.load_state_dict(sw.synth_state_dict(net, BF, device=gpu), strict=True)
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=gpu), device=gpu)
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=vae, model_instance={"forward": model}, guidance=0.0, num_steps=2)
    p.device = gpu
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    names = ("depth", "normal", "roughness", "metallic", "base_color")
    g = {k: sw.synth_tensor("winfw." + k, (1, 17, 32, 32, 3), torch.float32).abs() for k in names}
    env = sw.synth_tensor("winfw.env", (1, 32, 64, 3), torch.float32).abs() * 4.0

    def run(maps, **kw):
        return node.run_forward_pass(p, *(maps[k] for k in names), env, guidance=0.0, seed=5, env_format="proj",
                                     env_rotation=180.0, **kw)[0]
    out = run(g, env_spin=0.0, window_frames=9, window_overlap=1)
    assert out.shape == (1, 17, 32, 32, 3) and out.dtype == torch.float32 and 0.0 <= out.min() and out.max() <= 1.0
    assert torch.equal(out, torch.round(out * 255) / 255)
    head = run({k: v[:, :9].contiguous() for k, v in g.items()}, env_spin=0.0, window_frames=9, window_overlap=1)
    assert head.shape == (1, 9, 32, 32, 3) and torch.equal(out[:, :8], head[:, :8])
    # a turning light is built over the WHOLE clip and cut per window
    spun = run(g, env_spin=90.0, window_frames=9, window_overlap=1)
    assert spun.shape == (1, 17, 32, 32, 3) and not torch.equal(spun, out)
    with pytest.raises(ValueError, match="window_overlap"):
        run(g, window_frames=9, window_overlap=5)
