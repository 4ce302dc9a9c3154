"""`window_align` on the GPU: drn_window_align_affine within the allowance of tests/window_align_refs.py (which
tests/test_window_align_cpu.py shows to separate the wrong kernels), drn_postprocess_window_align_u8 bit for bit against the torch
specification, every refusal of both, and the windowed pipeline and nodes against the composition by hand from the entries.
Every kernel case is launched twice inside sentinel guard bands."""
import dataclasses
import importlib

import numpy as np
import pytest
import torch

import dit_refs as D
import window_align_refs as A
import window_refs as WR
from test_windows_gpu import _RaggedStubVAE, _by_hand, _pipeline

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 64                      # bytes; keeps every guarded output 16-byte aligned: the 8-value paths stay the ones under test
DRN_EINVAL = -1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _at_offset(t, gpu, off):
    """The same values `off` elements past a 16-byte aligned address."""
    flat = torch.empty(t.numel() + off, dtype=t.dtype, device=gpu)
    flat[off:] = t.reshape(-1).to(gpu)
    return flat[off:].view(t.shape)


class _Guarded:
    """Output regions of any dtype inside ONE byte buffer full of dit_refs.SENTINEL_U8, GUARD bytes apart."""

    def __init__(self, gpu, **regions):
        self.spans, at = {}, GUARD
        for name, (shape, dtype) in regions.items():
            n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            self.spans[name] = (at, n, shape, dtype)
            at += (n + GUARD + 15) // 16 * 16
        self.buf = torch.full((at,), D.SENTINEL_U8, dtype=torch.uint8, device=gpu)

    def __getitem__(self, name):
        at, n, shape, dtype = self.spans[name]
        return self.buf[at:at + n].view(dtype).view(shape)

    def intact(self):
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for at, n, _, _ in self.spans.values():
            inside[at:at + n] = True
        return bool(((self.buf == D.SENTINEL_U8) | inside).all())

    def untouched(self):
        return bool((self.buf == D.SENTINEL_U8).all())


def _affine(pkg, gpu, video, prev, ramp_at):
    """drn_window_align_affine into guard-banded outputs and workspace, twice -> (affine fp32 [B,2], moments fp64 [B,6]) on the CPU;
    the two launches must agree in every bit and write nothing else."""
    lib = pkg.native.load_library()
    B, _, Tw, H, W = video.shape
    Ov = prev.shape[2]
    nbytes = lib.drn_window_align_workspace_bytes(B, H, W, Ov)
    assert nbytes == B * 3 * -(-Ov * H * W // A.CHUNK) * 5 * 8
    runs = []
    for _ in range(2):
        g = _Guarded(gpu, affine=((B, 2), torch.float32), moments=((B, 6), torch.float64), ws=((nbytes // 8,), torch.float64))
        rc = lib.drn_window_align_affine(video.data_ptr(), prev.data_ptr(), g["affine"].data_ptr(), g["moments"].data_ptr(),
                                         g["ws"].data_ptr(), nbytes, B, Tw, H, W, Ov, ramp_at, _stream())
        assert rc == 0
        assert g.intact(), "wrote outside its outputs"
        runs.append((g["affine"].cpu().clone(), g["moments"].cpu().clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), "two launches differ"
    assert torch.equal(runs[0][1].view(torch.int64), runs[1][1].view(torch.int64)), "two launches differ"
    return runs[0]


@pytest.mark.parametrize("H,W", A.SHAPES)
def test_affine_kernel_on_the_grid(pkg, gpu, H, W):
    cases = [c for c in A.grid() if c[:2] == (H, W)]
    for (_, _, Ov, B, at, off) in cases:
        prev, over = A.overlap_pair(H, W, Ov, B)
        ref = A.overlap_reference(H, W, Ov, B)
        video = A.window_around(over, at)
        aff, mom = _affine(pkg, gpu, _at_offset(video, gpu, off), _at_offset(prev, gpu, off), at)
        print(f"window-align affine {H}x{W} O={Ov} B={B} ramp_at={at} offset={off}: worst {ref.worst(aff.numpy()):.3f} allowances, "
              f"g {aff[:, 0].tolist()} o {aff[:, 1].tolist()}")
        assert ref.affine_ok(aff.numpy()), (Ov, B, at, off, aff, ref.affine)
        assert ref.moments_ok(mom.numpy()), (Ov, B, at, off, mom, ref.moments)
        if not off:                                                    # the wrapper makes the same call
            assert torch.equal(pkg.native.window_align_affine(video.to(gpu), prev.to(gpu), at).cpu(), aff)


def test_affine_kernel_on_the_rule_cases(pkg, gpu):
    for name in A.RULE_CASES:
        prev, over, _ = A.rule_pair(name)
        ref = A.rule_reference(name)
        aff, mom = _affine(pkg, gpu, A.window_around(over, A.RULE_AT).to(gpu), prev.to(gpu), A.RULE_AT)
        print(f"window-align affine rule {name}: g {float(aff[0, 0])!r} o {float(aff[0, 1])!r} (exact {ref.affine[0].tolist()})")
        assert ref.affine_ok(aff.numpy()), (name, aff, ref.affine)
        assert ref.moments_ok(mom.numpy()), (name, mom, ref.moments)


def test_affine_kernel_refusals(pkg, gpu):
    lib = pkg.native.load_library()
    B, Tw, H, W, Ov = 1, A.TW, 8, 8, 2
    video = torch.zeros((B, 3, Tw, H, W), dtype=BF, device=gpu)
    prev = torch.zeros((B, 3, Ov, H, W), dtype=BF, device=gpu)
    nbytes = lib.drn_window_align_workspace_bytes(B, H, W, Ov)
    assert nbytes == 3 * 5 * 8 and lib.drn_window_align_workspace_bytes(B, H, W, 0) == 0
    assert lib.drn_window_align_workspace_bytes(0, H, W, Ov) == 0 and lib.drn_window_align_workspace_bytes(B, -1, W, Ov) == 0
    g = _Guarded(gpu, affine=((B, 2), torch.float32), moments=((B, 6), torch.float64), ws=((nbytes // 8,), torch.float64))
    v, p, a, m, ws = video.data_ptr(), prev.data_ptr(), g["affine"].data_ptr(), g["moments"].data_ptr(), g["ws"].data_ptr()

    def call(video=v, prev=p, affine=a, moments=m, ws=ws, ws_bytes=nbytes, B_=B, Tw_=Tw, H_=H, W_=W, O_=Ov, ramp_at=0):
        return lib.drn_window_align_affine(video, prev, affine, moments, ws, ws_bytes, B_, Tw_, H_, W_, O_, ramp_at, _stream())
    bad = {
        "null video": dict(video=None), "null carry": dict(prev=None), "null affine": dict(affine=None), "null workspace": dict(ws=None),
        "O = 0": dict(O_=0), "O < 0": dict(O_=-1), "ramp_at < 0": dict(ramp_at=-1), "overlap past the window": dict(ramp_at=Tw - 1),
        "short workspace": dict(ws_bytes=nbytes - 8), "odd video": dict(video=v + 1), "odd carry": dict(prev=p + 1),
        "affine off 4": dict(affine=a + 2), "moments off 8": dict(moments=m + 4), "workspace off 8": dict(ws=ws + 4),
        "B = 0": dict(B_=0), "Tw = 0": dict(Tw_=0), "H = 0": dict(H_=0), "W < 0": dict(W_=-8),
    }
    for name, kw in bad.items():
        assert call(**kw) == DRN_EINVAL, name
    torch.cuda.synchronize()
    assert g.untouched(), "a rejected call wrote"
    assert call(ramp_at=Tw - Ov) == 0 and call(moments=None) == 0
    torch.cuda.synchronize()
    assert g.intact()


# ----------------------------------------------------------------------------------------------- the align post-process
def _launch(pkg, gpu, video, prev, w, affine, geo, normalize, carry_frames):
    """drn_postprocess_window_align_u8 into guard-banded outputs, twice -> (bytes, carry or None) on the CPU."""
    ramp_at, lo, hi = geo
    B, _, _, H, W = video.shape
    regions = dict(out=((B, hi - lo, H, W, 3), torch.uint8))
    if carry_frames:
        regions["carry"] = ((B, 3, carry_frames, H, W), BF)
    g = _Guarded(gpu, **regions)
    for _ in range(2):
        pkg.native.postprocess_window_align_u8(video, prev, w, affine, ramp_at, lo, hi, normalize, out=g["out"],
                                               carry_out=g["carry"] if carry_frames else None)
    assert g.intact(), "wrote outside its outputs"
    return g["out"].cpu().clone(), g["carry"].cpu().clone() if carry_frames else None


def _affines(B):
    fixed = [(1.0, 0.0), (0.5, 0.25), (2.0, -1.0)]
    gen = torch.Generator().manual_seed(515 + B)
    drawn = torch.stack([0.5 + 1.5 * torch.rand(B, generator=gen), torch.rand(B, generator=gen) - 0.5], 1)
    return [torch.tensor([f] * B) for f in fixed] + [drawn]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("H,W", WR.SHAPES)
def test_align_kernel_bit_exact(pkg, gpu, H, W):
    launches = 0
    for B in (1, 2):
        for Ov in WR.OVERLAPS:
            video, prev = WR.case_inputs(B, H, W, Ov)
            w = WR.ramp_table(pkg, Ov) if Ov else None
            vd, pd, wd = video.to(gpu), None if prev is None else prev.to(gpu), None if w is None else w.to(gpu)
            for k, geo in enumerate(WR.case_geometries(Ov)):
                for normalize in (False, True):
                    for aff in (_affines(B) if B == 2 else _affines(B)[(k + normalize) % 4:][:1]):
                        got, carry = _launch(pkg, gpu, vd, pd, wd, aff.to(gpu), geo, normalize, Ov)
                        ref, rcarry = A.align_postprocess(video, prev, w, aff, *geo, normalize, Ov)
                        tag = f"B{B} {H}x{W} O={Ov} ramp_at/lo/hi={geo} normalize={normalize} affine={aff.tolist()}"
                        assert torch.equal(got, ref), f"{tag}: {int((got != ref).sum())} of {ref.numel()} bytes differ"
                        assert (carry is None and rcarry is None) or _same_bits(carry, rcarry), f"{tag}: the carry differs"
                        launches += 1
    print(f"window-align kernel {H}x{W}: {launches} cases bit-exact")


@pytest.mark.parametrize("H,W", [(8, 12), (5, 7)])
def test_align_kernel_without_an_affine_is_todays_kernel_and_the_raw_tail(pkg, gpu, H, W):
    for Ov in (1, 2, 4):
        video, prev = WR.case_inputs(2, H, W, Ov)
        vd, pd, wd = video.to(gpu), prev.to(gpu), WR.ramp_table(pkg, Ov).to(gpu)
        for geo in WR.case_geometries(Ov):
            for normalize in (False, True):
                got, carry = _launch(pkg, gpu, vd, pd, wd, None, geo, normalize, Ov)
                today = pkg.native.postprocess_window_u8(vd, pd, wd, *geo, normalize).cpu()
                assert torch.equal(got, today) and _same_bits(carry, video[:, :, WR.TW - Ov:])
        # window 0's shape of call: no carry read, a carry written
        got, carry = _launch(pkg, gpu, vd, None, None, None, (0, 0, WR.TW - Ov), False, Ov)
        assert torch.equal(got, pkg.native.postprocess_window_u8(vd, None, None, 0, 0, WR.TW - Ov, False).cpu())
        assert _same_bits(carry, video[:, :, WR.TW - Ov:])


def test_align_kernel_value_grid_shows_a_fused_apply(pkg, gpu):
    """window_refs.value_grid under the affine of window_align_refs.fma_affine: test_window_align_cpu shows that a fused
    multiply-add changes bytes there."""
    Ov = 2
    video, prev = WR.value_grid(Ov)
    w = WR.ramp_table(pkg, Ov)
    aff = torch.tensor([A.fma_affine()])
    for normalize in (False, True):
        got, carry = _launch(pkg, gpu, video.to(gpu), prev.to(gpu), w.to(gpu), aff.to(gpu), (0, 0, WR.TW), normalize, Ov)
        ref, rcarry = A.align_postprocess(video, prev, w, aff, 0, 0, WR.TW, normalize, Ov)
        print(f"window-align value grid normalize={normalize}: {int((got != ref).sum())} bytes differ")
        assert torch.equal(got, ref) and _same_bits(carry, rcarry)


def test_align_kernel_unaligned_buffers_take_the_pixel_path(pkg, gpu):
    video, prev = WR.case_inputs(2, 8, 12, 2)
    w = WR.ramp_table(pkg, 2)
    aff = _affines(2)[3]
    ref, rcarry = A.align_postprocess(video, prev, w, aff, 3, 3, WR.TW, False, 2)
    vd, pd, wd, ad = video.to(gpu), prev.to(gpu), w.to(gpu), aff.to(gpu)
    for v_, p_ in ((_at_offset(video, gpu, 1), pd), (vd, _at_offset(prev, gpu, 1))):
        got, carry = _launch(pkg, gpu, v_, p_, wd, ad, (3, 3, WR.TW), False, 2)
        assert torch.equal(got, ref) and _same_bits(carry, rcarry)
    # a carry_out 2 bytes past an aligned address
    flat = torch.full((rcarry.numel() + 16,), D.SENTINEL, dtype=torch.int16, device=gpu).view(BF)
    out, carry = pkg.native.postprocess_window_align_u8(vd, pd, wd, ad, 3, 3, WR.TW, False, carry_out=flat[1:1 + rcarry.numel()].view(rcarry.shape))
    assert torch.equal(out.cpu(), ref) and _same_bits(carry.cpu(), rcarry)
    assert D.is_sentinel(flat[:1]).all() and D.is_sentinel(flat[1 + rcarry.numel():]).all()


def test_align_kernel_refusals(pkg, gpu):
    lib = pkg.native.load_library()
    Tw, H, W, Ov = WR.TW, 8, 8, 2
    video = torch.zeros((1, 3, Tw, H, W), dtype=BF, device=gpu)
    prev = torch.zeros((1, 3, Ov, H, W), dtype=BF, device=gpu)
    w = WR.ramp_table(pkg, Ov).to(gpu)
    aff = torch.ones((1, 2), dtype=torch.float32, device=gpu)
    g = _Guarded(gpu, out=((1, Tw, H, W, 3), torch.uint8), carry=((1, 3, Ov, H, W), BF))
    v, p, r, a, o, c = video.data_ptr(), prev.data_ptr(), w.data_ptr(), aff.data_ptr(), g["out"].data_ptr(), g["carry"].data_ptr()

    def call(video=v, prev=p, ramp=r, affine=a, out=o, carry=c, O_=Ov, ramp_at=0, lo=0, hi=Tw, B_=1, H_=H):
        return lib.drn_postprocess_window_align_u8(video, prev, ramp, affine, out, carry, B_, Tw, H_, W, O_, ramp_at, lo, hi, 0, _stream())
    bad = {
        # the refusals of drn_postprocess_window_u8
        "null video": dict(video=None), "null out": dict(out=None),
        "carry without weights": dict(ramp=None), "weights without carry": dict(prev=None),
        "O < 0": dict(O_=-1), "ramp_at < 0": dict(ramp_at=-1), "ramp past the window": dict(ramp_at=Tw - 1),
        "write_lo < 0": dict(lo=-1), "empty range": dict(lo=4, hi=4), "reversed range": dict(lo=5, hi=4),
        "write_hi past the window": dict(hi=Tw + 1), "write_lo inside the ramp": dict(ramp_at=3, lo=4),
        "B = 0": dict(B_=0), "H < 0": dict(H_=-8), "odd video": dict(video=v + 1), "odd carry": dict(prev=p + 1),
        "weights off 4": dict(ramp=r + 2),
        # and those of the two new pointers
        "affine off 4": dict(affine=a + 2), "odd carry_out": dict(carry=c + 1),
        "carry_out without frames": dict(prev=None, ramp=None, O_=0), "carry_out is the carry read": dict(carry=p),
        "carry_out is the window": dict(carry=v),
    }
    for name, kw in bad.items():
        assert call(**kw) == DRN_EINVAL, name
    torch.cuda.synchronize()
    assert g.untouched(), "a rejected call wrote"
    assert call(ramp_at=3, lo=3) == 0 and call(ramp_at=Tw - Ov) == 0 and call(affine=None) == 0 and call(carry=None) == 0
    assert call(prev=None, ramp=None, carry=None, O_=0) == 0 and call(prev=None, ramp=None) == 0
    torch.cuda.synchronize()
    assert g.intact()


# ----------------------------------------------------------------------------------------------- pipeline
def _by_hand_aligned(pkg, p, rgb, cis, flags, seed, noise, Wf, Ov, restore=None):
    """The aligned windowed clip composed outside the pipeline, from the entries: _sample + decode per planned window, then per
    pass today's call (window 0, a normal pass) or the affine launch and the align launch."""
    N = pkg.native
    fit = importlib.import_module(pkg.__name__ + ".fit")
    T = rgb.shape[2]
    plan = pkg.windows.plan_windows(T, Wf, Ov)
    w = WR.ramp_table(pkg, Ov).to(p.device)
    outs, carry = [None] * len(flags), [None] * len(flags)
    keep = (p.window_frames, p.window_align)
    p.window_frames, p.window_align = 0, False
    for i, win in enumerate(plan):
        clip = rgb[:, :, win.start:win.start + Wf].contiguous()
        sample = p._sample({"rgb": clip, "video": clip, "context_index": cis}, seed, noise)
        last = i + 1 == len(plan)
        for k, flag in enumerate(flags):
            video = p.model.decode(sample[k:k + 1]).to(BF).contiguous()
            prev = carry[k]
            if prev is not None and not flag:
                aff = N.window_align_affine(video, prev, win.ramp_at)
                u8, carry[k] = N.postprocess_window_align_u8(video, prev, w, aff, win.ramp_at, win.write_lo, win.write_hi, flag,
                                                             carry_frames=0 if last else Ov)
            else:
                u8 = N.postprocess_window_u8(video, prev, w if prev is not None else None, win.ramp_at, win.write_lo, win.write_hi, flag)
                carry[k] = video[:, :, Wf - Ov:].contiguous()
            if restore is not None:
                u8 = fit.restore_frames(u8, dataclasses.replace(restore, T=u8.shape[1]))
            if outs[k] is None:
                outs[k] = torch.zeros((1, T) + tuple(u8.shape[2:]), dtype=torch.uint8, device=u8.device)
            outs[k][:, win.out_at:win.out_at + u8.shape[1]] = u8
    p.window_frames, p.window_align = keep
    return [o.cpu().numpy() for o in outs]


def test_aligned_pipeline_is_the_composition_by_hand(pkg, gpu):
    sw = pkg.synthetic_weights
    fit = importlib.import_module(pkg.__name__ + ".fit")
    p = _pipeline(pkg, gpu, _RaggedStubVAE())
    T, Wf, Ov, seed = 21, 9, 2, 5
    rgb = sw.synth_tensor("align.rgb", (1, 3, T, 64, 64), torch.float32, scale=1.0)
    noise = sw.synth_tensor("align.xT", (1, 16, 2, 8, 8), torch.float32, scale=80.0)
    ci = torch.full((1, 1), 3, dtype=torch.long)
    batch = {"rgb": rgb, "video": rgb, "context_index": ci}
    p.window_frames, p.window_overlap = Wf, Ov

    # window_align off: bit for bit the parent's output (the CPU blend reference of test_windows_gpu)
    for normalize in (False, True):
        (today,) = _by_hand(pkg, p, rgb, ci, [normalize], seed, noise, Wf, Ov)
        assert np.array_equal(p.generate_video(batch, normalize_normal=normalize, seed=seed, init_noise=noise), today)
        # on: generate_video against the entries by hand; a normal pass is never aligned
        p.window_align = True
        got = p.generate_video(batch, normalize_normal=normalize, seed=seed, init_noise=noise)
        (ref,) = _by_hand_aligned(pkg, p, rgb, ci, [normalize], seed, noise, Wf, Ov)
        p.window_align = False
        assert got.shape == (1, T, 64, 64, 3) and np.array_equal(got, ref), f"normalize={normalize}: {(got != ref).sum()} bytes differ"
        first = pkg.windows.plan_windows(T, Wf, Ov)[1].out_at
        assert np.array_equal(got[:, :first], today[:, :first])
        assert np.array_equal(got, today) == normalize
        print(f"window-align pipeline normalize={normalize}: {(got != today).sum()} of {got.size} bytes moved by the alignment")

    # passes in one batch, passes one after the other, results left on the device
    p.window_align = True
    idx = torch.tensor([[0], [3]], dtype=torch.long)
    refs = _by_hand_aligned(pkg, p, rgb, idx, [False, True], seed, None, Wf, Ov)
    both = p.generate_video_passes({"rgb": rgb, "video": rgb, "context_index": idx}, normalize_normal=[False, True], seed=seed,
                                   to_host=False)
    assert all(isinstance(b, torch.Tensor) and b.is_cuda for b in both)
    assert all(np.array_equal(b.cpu().numpy(), r) for b, r in zip(both, refs))
    each = p.generate_video_each([{"rgb": rgb, "video": rgb, "context_index": idx[k:k + 1]} for k in range(2)], [False, True], seed=seed)
    assert all(np.array_equal(e, r) for e, r in zip(each, refs))

    # a restore plan: every window's written frames come back at the source's size
    plan = fit.plan_fit(T, 80, 72, "stretch", 64, 64, windowed=True)
    p.restore_plan = fit.plan_restore(plan)
    got = p.generate_video(batch, normalize_normal=False, seed=seed, init_noise=noise)
    (ref,) = _by_hand_aligned(pkg, p, rgb, ci, [False], seed, noise, Wf, Ov, restore=p.restore_plan)
    assert got.shape == (1, T, 80, 72, 3) and np.array_equal(got, ref)
    p.restore_plan = None

    # refusals, and a clip of one window
    p.window_overlap = 0
    with pytest.raises(ValueError, match="window_overlap"):
        p.generate_video(batch, seed=seed)
    p.window_overlap, p.tile_height, p.tile_width = Ov, 32, 32
    with pytest.raises(ValueError, match="tiles"):
        p.generate_video(batch, seed=seed)
    p.tile_height = p.tile_width = 0
    short = {"rgb": rgb[:, :, :9].contiguous(), "context_index": ci}
    short["video"] = short["rgb"]
    on = p.generate_video(short, normalize_normal=False, seed=seed, init_noise=noise)
    p.window_align = False
    assert np.array_equal(on, p.generate_video(short, normalize_normal=False, seed=seed, init_noise=noise))


# ----------------------------------------------------------------------------------------------- nodes
def test_nodes_with_window_align(pkg, gpu):
    sw = pkg.synthetic_weights
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=gpu), device=gpu)
    p = _pipeline(pkg, gpu, vae)
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    image = sw.synth_tensor("alignnode.img", (1, 21, 64, 64, 3), torch.float32).abs()
    off = node.run_inverse_pass(p, image, guidance=0.0, seed=3, window_frames=9, window_overlap=2)
    on = node.run_inverse_pass(p, image, guidance=0.0, seed=3, window_frames=9, window_overlap=2, window_align=True)
    assert p.window_align is True and len(on) == 5
    for name, a, b in zip(("basecolor", "metallic", "roughness", "normal", "depth"), on, off):
        assert a.shape == (21, 64, 64, 3) and torch.equal(a[:7], b[:7]), name          # window 0 is nobody's follower
        assert torch.equal(a, b) == (name == "normal"), name                           # the normal pass is never aligned
        assert torch.equal(a, torch.round(a * 255) / 255)
    again = node.run_inverse_pass(p, image, guidance=0.0, seed=3, window_frames=9, window_overlap=2, window_align=True)
    assert all(torch.equal(a, b) for a, b in zip(on, again))                           # no atomics: the same bits every run
    with pytest.raises(ValueError, match="window_overlap"):
        node.run_inverse_pass(p, image, guidance=0.0, seed=3, window_frames=9, window_overlap=0, window_align=True)


def test_forward_and_relight_nodes_with_window_align(pkg, gpu):
    sw = pkg.synthetic_weights
    cfgm = pkg.diffusion_renderer_config
    from conftest import tiny_net
    models = {}
    for kind, forward in (("inverse", False), ("forward", True)):
        net = tiny_net(pkg, 256, 1, 2, forward=forward)
        cfg = cfgm.get_forward_renderer_config() if forward else cfgm.get_inverse_renderer_config()
        cfg["net"] = dict(net)
        cfg["model_type"] = kind
        models[kind] = pkg.model_diffusion_renderer.CleanDiffusionRendererModel(cfg, device=gpu)
        models[kind].load_state_dict(sw.synth_state_dict(net, BF, device=gpu), strict=True)
    vae = pkg.CleanVAE.CleanVAE(state_dict=sw.synth_vae_state_dict(device=gpu), device=gpu)
    p = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline(
        "/nonexistent", "x.pt", model_type=None, vae_instance=vae, model_instance=models, guidance=0.0, num_steps=2)
    p.device = gpu
    fwd = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    rel = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    names = ("depth", "normal", "roughness", "metallic", "base_color")
    g = {k: sw.synth_tensor("alignfw." + k, (1, 17, 32, 32, 3), torch.float32).abs() for k in names}
    env = sw.synth_tensor("alignfw.env", (1, 32, 64, 3), torch.float32).abs() * 4.0

    def run(**kw):
        return fwd.run_forward_pass(p, *(g[k] for k in names), env, guidance=0.0, seed=5, env_format="proj", env_rotation=180.0,
                                    window_frames=9, window_overlap=1, **kw)[0]
    off, on = run(), run(window_align=True)
    assert on.shape == (1, 17, 32, 32, 3) and torch.equal(on[:, :8], off[:, :8]) and not torch.equal(on, off)
    assert torch.equal(on, run(window_align=True))
    image = sw.synth_tensor("alignrel.img", (1, 17, 32, 32, 3), torch.float32).abs().clamp(max=1.0)
    outs_off = rel.run_relight(p, p, image, env, seed=5, window_frames=9, window_overlap=1)
    outs_on = rel.run_relight(p, p, image, env, seed=5, window_frames=9, window_overlap=1, window_align=True)
    assert len(outs_on) == 6 and not torch.equal(outs_on[0], outs_off[0])
    assert torch.equal(outs_on[4], outs_off[4])                                       # RETURN_NAMES[4] = normal: never aligned
    assert not torch.equal(outs_on[1], outs_off[1])
