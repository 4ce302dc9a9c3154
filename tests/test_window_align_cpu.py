"""`window_align` without a GPU: the specification in windows.py against the float64 references of tests/window_align_refs.py,
the proof that the cases of the GPU test tell a right kernel from the wrong ones, and the host semantics (plan, refusals, nodes,
"off = today's calls")."""
import numpy as np
import pytest
import torch

import window_align_refs as A
import window_refs as WR

BF = torch.bfloat16


# ----------------------------------------------------------------------------------------------- references and allowance
def test_grid_covers_what_the_issue_names():
    g = A.grid()
    assert len(g) == len(set(g)) == 7 * 3 * 2 * 3 * 2
    assert {c[:2] for c in g} >= {(8, 8), (5, 7), (3, 11), (8, 12), (37, 53), (64, 96)}
    assert {c[2] for c in g} == {1, 2, 4} and {c[3] for c in g} == {1, 3} and {c[5] for c in g} == {0, 1}
    for O in A.OVERLAPS:
        assert A.ramp_ats(O) == sorted({0, 3, A.TW - O})
    assert (37 * 53) % 8 and (45 * 61) % 8 and not (64 * 96) % 8
    assert 4 * 64 * 96 > 2 * A.CHUNK and 2 * A.CHUNK > 4 * 45 * 61 > A.CHUNK > 4 * 8 * 12          # several blocks per channel


@pytest.mark.parametrize("H,W", A.SHAPES)
def test_allowance_stays_near_one_ulp(H, W):
    """var_v >= 1e-3 keeps E[x^2] - mean^2 well conditioned: the two float64 evaluations agree far below an fp32 ulp, so the
    allowance is one ulp and a little."""
    for O in A.OVERLAPS:
        for B in A.BATCHES:
            ref = A.overlap_reference(H, W, O, B)
            assert (ref.moments[:, 4] >= 1e-3).all() and (ref.moments[:, 3] >= 1e-3).all() and (ref.moments[:, 5] > 0).all()
            ratio = ref.allow / A.ulp32(ref.affine)
            print(f"window-align allowance {H}x{W} O={O} B={B}: {ratio.max():.6f} ulp")
            assert (ratio >= 1.0).all() and (ratio <= 1.01).all()
            assert ((ref.affine[:, 0] > 0.5) & (ref.affine[:, 0] < 2.0)).all()                # the grid is not the clamp's business
            if B == 3:
                assert len({round(float(g), 2) for g in ref.affine[:, 0]}) == 3               # different statistics per row


def test_rule_cases_are_what_they_claim():
    for name in A.RULE_CASES:
        prev, over, want = A.rule_pair(name)
        ref = A.rule_reference(name)
        g, o = ref.affine[0]
        n, ma, mv, va, vv, cov = ref.moments[0]
        if name.startswith(("nan", "inf")):
            assert not np.isfinite(ref.moments).all() and (g, o) == (1.0, 0.0)
        elif name.startswith("flat"):
            assert min(va, vv) < A.FLAT_VAR and g == 1.0 and o == ma - mv
        elif name == "cov_negative":
            assert cov < 0 and va > 1e-3 and vv > 1e-3 and g == 1.0 and o == ma - mv
        elif name == "gain_4":
            assert np.sqrt(va / vv) > 3.5 and g == 2.0 and o == ma - 2.0 * mv and abs(o - (ma - np.sqrt(va / vv) * mv)) > 0.05
        elif name == "gain_quarter":
            assert np.sqrt(va / vv) < 0.3 and g == 0.5 and o == ma - 0.5 * mv
        else:
            assert float(over.float().abs().max()) > 65504 / 2 and np.isfinite(ref.moments).all() and 1.0 < g < 1.5
        assert ref.affine_ok(ref.affine_pw)


# ----------------------------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("H,W", A.SHAPES)
def test_specification_meets_the_reference(pkg, H, W):
    for O in A.OVERLAPS:
        for B in A.BATCHES:
            prev, over = A.overlap_pair(H, W, O, B)
            ref = A.overlap_reference(H, W, O, B)
            for at in A.ramp_ats(O):
                got = pkg.windows.align_affine(A.window_around(over, at), prev, at)
                assert got.dtype == torch.float32 and got.shape == (B, 2)
                assert ref.affine_ok(got.numpy()), (H, W, O, B, at, ref.worst(got.numpy()))


def test_specification_on_the_rule_cases(pkg):
    for name in A.RULE_CASES:
        prev, over, _ = A.rule_pair(name)
        got = pkg.windows.align_affine(A.window_around(over, A.RULE_AT), prev, A.RULE_AT).numpy()
        assert A.rule_reference(name).affine_ok(got), (name, got)
    with pytest.raises(ValueError):
        pkg.windows.align_affine(torch.zeros(1, 3, 9, 2, 2).to(BF), torch.zeros(1, 3, 2, 2, 2).to(BF), 8)


def test_apply_specification_spells_the_contract(pkg):
    """One value by hand - two fp32 roundings, then bf16 - and the torch reference on a window."""
    x, g, o = np.float32(0.77734375), np.float32(1.2345678), np.float32(-0.3456789)
    want = torch.tensor(float(np.float32(np.float32(g * x) + o))).to(BF)
    got = pkg.windows.apply_affine(torch.full((1, 3, 1, 1, 1), float(x)).to(BF), torch.tensor([[g, o]]))
    assert got.dtype == BF and (got == want).all()
    video, _ = WR.case_inputs(3, 5, 7, 2)
    aff = torch.tensor([[1.0, 0.0], [0.5, 0.25], [1.7, -0.3]])
    assert torch.equal(pkg.windows.apply_affine(video, aff), A.apply_affine(video, aff))
    assert torch.equal(pkg.windows.apply_affine(video, aff)[0], video[0])                     # (1, 0) is the identity


# ----------------------------------------------------------------------------------------------- the proof
@pytest.mark.parametrize("H,W", A.SHAPES)
def test_block_partition_standin_passes_every_case(H, W):
    for O in A.OVERLAPS:
        for B in A.BATCHES:
            prev, over = A.overlap_pair(H, W, O, B)
            ref = A.overlap_reference(H, W, O, B)
            for at in A.ramp_ats(O):
                got = A.standin(prev, A.window_around(over, at), at)
                assert ref.affine_ok(got), (H, W, O, B, at, ref.worst(got))


def test_block_partition_standin_passes_the_rule_cases():
    for name in A.RULE_CASES:
        prev, over, _ = A.rule_pair(name)
        assert A.rule_reference(name).affine_ok(A.standin(prev, A.window_around(over, A.RULE_AT), A.RULE_AT)), name


# variant -> the case that catches it: a grid case (H, W, O, B, ramp_at) or a rule case
CAUGHT_BY = {"slope": (8, 12, 2, 1, 3), "per_channel": (5, 7, 1, 1, 0), "row0": (3, 11, 4, 3, 5), "o_unclamped": "gain_4",
             "no_sqrt": (45, 61, 4, 1, 0), "swapped": (64, 96, 2, 3, 3), "head": (8, 8, 2, 1, 3)}


@pytest.mark.parametrize("variant", A.STANDINS)
def test_every_wrong_standin_fails_a_named_case(variant):
    case = CAUGHT_BY[variant]
    if isinstance(case, str):
        prev, over, _ = A.rule_pair(case)
        ref, at = A.rule_reference(case), A.RULE_AT
    else:
        H, W, O, B, at = case
        assert (H, W, O, B, at, 0) in A.grid()
        prev, over = A.overlap_pair(H, W, O, B)
        ref = A.overlap_reference(H, W, O, B)
    video = A.window_around(over, at)
    assert ref.affine_ok(A.standin(prev, video, at))
    wrong = A.standin(prev, video, at, variant=variant)
    print(f"window-align stand-in {variant} at {case}: {ref.worst(wrong):.3g} allowances off")
    assert not ref.affine_ok(wrong)


def _walk_inputs(pkg):
    """Three windows of 9 over 21 frames (O = 2), two passes - pass 1 a normal pass - whose windows disagree in gain and offset."""
    plan = pkg.windows.plan_windows(21, 9, 2)
    g = torch.Generator().manual_seed(77)
    truth = torch.randn((2, 3, 21, 8, 12), generator=g) * 0.4
    windows = [((0.8 + 0.3 * i) * truth[:, :, w.start:w.start + 9] + 0.1 * i - 0.05
                + 0.02 * torch.randn((2, 3, 9, 8, 12), generator=g)).to(BF) for i, w in enumerate(plan)]
    return plan, windows, WR.ramp_table(pkg, 2)


def test_apply_standins_change_bytes(pkg):
    """The wrong applies against the byte reference.  The fused apply needs the value grid and an affine under which a bf16 tie
    is hit (window_align_refs.fma_affine); the others change bytes on any windowed clip."""
    plan, windows, ramp = _walk_inputs(pkg)
    ref = A.walk(windows, plan, 2, ramp, [False, True], True, pkg.windows.align_affine)
    off = A.walk(windows, plan, 2, ramp, [False, True], False, pkg.windows.align_affine)
    assert not torch.equal(ref[0], off[0]) and torch.equal(ref[1], off[1])                   # the normal pass is never aligned
    assert torch.equal(ref[:, :plan[1].out_at], off[:, :plan[1].out_at])                     # window 0 is nobody's follower
    for variant in A.APPLY_VARIANTS:
        if variant == "fma":
            continue
        got = A.walk(windows, plan, 2, ramp, [False, True], True, pkg.windows.align_affine, variant=variant)
        n = int((got != ref).sum())
        print(f"window-align apply stand-in {variant}: {n} bytes differ")
        assert n > 0, variant
    video, prev = WR.value_grid(2)
    aff = torch.tensor([A.fma_affine()])
    a, ca = A.align_postprocess(video, prev, ramp, aff, 0, 0, A.TW, False, 2)
    b, cb = A.align_postprocess(video, prev, ramp, aff, 0, 0, A.TW, False, 2, variant="fma")
    print(f"window-align apply stand-in fma: {int((a != b).sum())} bytes, {int((ca.view(torch.int16) != cb.view(torch.int16)).sum())} carry values differ")
    assert int((a != b).sum()) >= 8


def test_affine_none_is_todays_kernel_and_the_raw_tail():
    video, prev = WR.case_inputs(2, 5, 7, 2)
    w = torch.tensor([1 / 3, 2 / 3])
    u8, carry = A.align_postprocess(video, prev, w, None, 3, 3, 7, True, 2)
    assert torch.equal(u8, WR.blend_postprocess(video, prev, w, 3, 3, 7, True)) and torch.equal(carry, video[:, :, 7:])


def test_quality_on_is_smaller_than_off(pkg):
    """Recorded in profiles/window_align_parity.txt, not judged beyond the order."""
    off, on = A.quality_figures(pkg)
    print(f"window-align quality: mean |byte error| against window 0's space, off {off:.3f}, on {on:.3f}")
    assert on < off


# ----------------------------------------------------------------------------------------------- host semantics
def test_check_window_align_rules(pkg):
    chk = pkg.windows.check_window_align
    chk(False, 9, 0, 32, 32)
    chk(True, 0, 0, 32, 32)                       # windows off: nothing to align, nothing to refuse
    chk(True, 9, 2)
    with pytest.raises(ValueError, match="window_overlap"):
        chk(True, 9, 0)
    for th, tw in ((32, 0), (0, 32), (32, 32)):
        with pytest.raises(ValueError, match="tiles"):
            chk(True, 9, 2, th, tw)


class _Model:
    """Stands in for the renderer model: window k of the clip comes back with a gain and offset of its own."""
    process_group = None
    net = None

    def __init__(self):
        self.config = {}
        self.calls = 0

    def to(self, device):
        return self

    def generate_samples_from_batch(self, data_batch, guidance, state_shape, num_steps, is_negative_prompt, seed, init_noise):
        k = self.calls
        self.calls += 1
        clip = data_batch["rgb"].float()
        rows = [clip * (0.8 + 0.25 * k - 0.05 * int(ci)) + 0.08 * k - 0.1 for ci in data_batch["context_index"].reshape(-1)]
        return torch.cat(rows).to(BF)

    def decode(self, sample):
        return sample


@pytest.fixture()
def cpu_pipe(pkg, monkeypatch):
    """A pipeline on the CPU whose native calls are recorded and answered by the CPU references."""
    mod = pkg.diffusion_renderer_pipeline
    calls = []

    def post(video, prev, ramp, ramp_at, lo, hi, normalize, out=None):
        calls.append(("postprocess_window_u8", prev is not None, ramp_at, lo, hi, bool(normalize)))
        return WR.blend_postprocess(video, prev, ramp, ramp_at, lo, hi, normalize)

    def affine(video, prev, ramp_at, moments=False):
        calls.append(("window_align_affine", ramp_at))
        return pkg.windows.align_affine(video, prev, ramp_at)

    def post_align(video, prev, ramp, aff, ramp_at, lo, hi, normalize, carry_frames=0, out=None, carry_out=None):
        calls.append(("postprocess_window_align_u8", ramp_at, lo, hi, bool(normalize), carry_frames))
        return A.align_postprocess(video, prev, ramp, aff, ramp_at, lo, hi, normalize, carry_frames)
    monkeypatch.setattr(mod.N, "postprocess_window_u8", post)
    monkeypatch.setattr(mod.N, "window_align_affine", affine)
    monkeypatch.setattr(mod.N, "postprocess_window_align_u8", post_align)
    model = _Model()
    p = mod.CleanDiffusionRendererPipeline("/nonexistent", "x.pt", model_type=None, model_instance=model, guidance=0.0, num_steps=2)
    p.device = torch.device("cpu")
    p.set_model_type("inverse")
    p.calls = calls
    return p


def _passes_batch(pkg, T=21):
    rgb = pkg.synthetic_weights.synth_tensor("align.rgb", (1, 3, T, 8, 12), torch.float32, scale=0.5)
    return {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[0], [3]], dtype=torch.long)}


def test_off_is_todays_calls(pkg, cpu_pipe):
    p = cpu_pipe
    assert p.window_align is False
    p.window_frames, p.window_overlap = 9, 2
    off = p.generate_video_passes(_passes_batch(pkg), normalize_normal=[False, True])
    names = [c[0] for c in p.calls]
    assert names == ["postprocess_window_u8"] * 6
    today = list(p.calls)
    # window_align on a clip of one window, or with windows off: the same calls as without it
    for frames, T in ((9, 9), (0, 21)):
        p.model.calls = 0
        del p.calls[:]
        p.window_frames = frames
        p.window_align = False
        a = p.generate_video_passes(_passes_batch(pkg, T), normalize_normal=[False, True])
        plain = list(p.calls)
        p.model.calls = 0
        del p.calls[:]
        p.window_align = True
        b = p.generate_video_passes(_passes_batch(pkg, T), normalize_normal=[False, True])
        assert p.calls == plain and all(c[0] == "postprocess_window_u8" for c in plain)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len(today) == 6 and len(off) == 2


def test_on_walks_affine_then_align_and_never_the_normal_pass(pkg, cpu_pipe):
    p = cpu_pipe
    p.window_frames, p.window_overlap, p.window_align = 9, 2, True
    plan = pkg.windows.plan_windows(21, 9, 2)
    on = p.generate_video_passes(_passes_batch(pkg), normalize_normal=[False, True])
    w1, w2 = plan[1], plan[2]
    assert p.calls == [
        ("postprocess_window_u8", False, 0, 0, 7, False), ("postprocess_window_u8", False, 0, 0, 7, True),
        ("window_align_affine", w1.ramp_at), ("postprocess_window_align_u8", w1.ramp_at, w1.write_lo, w1.write_hi, False, 2),
        ("postprocess_window_u8", True, w1.ramp_at, w1.write_lo, w1.write_hi, True),
        ("window_align_affine", w2.ramp_at), ("postprocess_window_align_u8", w2.ramp_at, w2.write_lo, w2.write_hi, False, 0),
        ("postprocess_window_u8", True, w2.ramp_at, w2.write_lo, w2.write_hi, True)]
    # the bytes are the reference walk's on the same decoded windows
    m = _Model()
    batch = _passes_batch(pkg)
    windows = [m.generate_samples_from_batch({"rgb": batch["rgb"][:, :, w.start:w.start + 9].to(BF), "context_index": batch["context_index"]},
                                             0, None, 2, False, 0, None) for w in plan]
    ref = A.walk(windows, plan, 2, WR.ramp_table(pkg, 2), [False, True], True, pkg.windows.align_affine)
    assert np.array_equal(on[0][0], ref[0].numpy()) and np.array_equal(on[1][0], ref[1].numpy())
    p.model.calls = 0
    p.window_align = False
    off = p.generate_video_passes(batch, normalize_normal=[False, True])
    assert np.array_equal(on[1], off[1]) and not np.array_equal(on[0], off[0])
    assert np.array_equal(on[0][:, :plan[1].out_at], off[0][:, :plan[1].out_at])


def test_refusals_come_before_any_work(pkg, cpu_pipe):
    p = cpu_pipe
    p.window_frames, p.window_overlap, p.window_align = 9, 0, True
    with pytest.raises(ValueError, match="window_overlap"):
        p.generate_video_passes(_passes_batch(pkg), normalize_normal=[False, True])
    p.window_overlap, p.tile_height, p.tile_width = 2, 16, 16
    with pytest.raises(ValueError, match="tiles"):
        p.generate_video_passes(_passes_batch(pkg), normalize_normal=[False, True])
    assert p.calls == [] and p.model is None and p.pre_loaded_model_instance.calls == 0

    class _Sharded:
        process_group = object()
    P = pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline
    q = P("/ckpt", "m.pt", model_instance=_Sharded())
    q.window_frames, q.window_align = 9, True
    with pytest.raises(NotImplementedError):
        q.generate_video({"rgb": torch.zeros(1, 3, 21, 8, 8)})


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
        self.calls.append((self.kind, self.window_frames, self.window_overlap, self.window_align))
        return self._out(data_batch, to_host)

    def generate_video_passes(self, data_batch, normalize_normal, seed=None, to_host=True):
        self.calls.append((self.kind, self.window_frames, self.window_overlap, self.window_align))
        return [self._out(data_batch, to_host) for _ in normalize_normal]


def test_nodes_hand_window_align_to_the_pipeline(pkg):
    classes = [pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"], pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"],
               pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]]
    for cls in classes:
        opt = cls.INPUT_TYPES()["optional"]["window_align"]
        assert opt[0] == "BOOLEAN" and opt[1]["default"] is False and "gain and offset" in opt[1]["tooltip"]
    assert pkg.diffusion_renderer_pipeline.CleanDiffusionRendererPipeline("/ckpt", "m.pt").window_align is False
    sw = pkg.synthetic_weights
    image = sw.synth_tensor("align.node", (1, 17, 32, 32, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("align.env", (1, 16, 32, 3), torch.float32).abs()
    inv, fwd, rel = (c() for c in classes)
    r = _Recorder()
    inv.run_inverse_pass(r, image, window_frames=9, window_overlap=1, window_align=True)
    inv.run_inverse_pass(r, image, window_frames=9, window_overlap=1)                        # every call sets the attribute
    assert r.calls == [("inverse", 9, 1, True), ("inverse", 9, 1, False)]
    r = _Recorder()
    fwd.run_forward_pass(r, *([image] * 5), env, window_frames=9, window_overlap=1, window_align=True)
    assert r.calls == [("forward", 9, 1, True)]
    r = _Recorder()
    rel.run_relight(r, r, image, env, window_frames=9, window_overlap=1, window_align=True)
    assert r.calls == [("inverse", 9, 1, True), ("forward", 9, 1, True)]
    # refused by the nodes before anything is handed over
    r = _Recorder()
    with pytest.raises(ValueError, match="window_overlap"):
        inv.run_inverse_pass(r, image, window_frames=9, window_overlap=0, window_align=True)
    with pytest.raises(ValueError, match="tiles"):
        fwd.run_forward_pass(r, *([image] * 5), env, window_frames=9, window_overlap=1, window_align=True, tile_height=16,
                             tile_width=16)
    with pytest.raises(ValueError, match="tiles"):
        rel.run_relight(r, r, image, env, window_frames=9, window_overlap=1, window_align=True, tile_width=16)
    assert r.calls == []
