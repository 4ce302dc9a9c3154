"""Ensembles that agree on the CPU: the numpy reference of tests/ensemble_align_refs.py (integer sums, then the rule) against a
brute-force float64 evaluation, the torch / numpy specification (ensemble.align_members, apply_affine_u8, reduce_members with an
affine) against the reference on the whole case grids, every branch of the rule on a named case, the proof that the grids tell
every wrong stand-in from the reference, the robustness inequality on a scene with structure, and the orchestration - the walk of
reduce_results, the pipeline's member loop with a recorder model whose members differ by known gains, the refusals, and what the
nodes set."""
import numpy as np
import pytest
import torch

import ensemble_align_refs as A
import ensemble_refs as R
from stub_vae import StubVAE

BF = torch.bfloat16


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tensors(mem):
    """[N, B, n] uint8 (n a multiple of 3) -> N tensors [B, n / 3, 3]."""
    N, B, n = mem.shape
    return [torch.from_numpy(np.ascontiguousarray(mem[k])).view(B, n // 3, 3) for k in range(N)]


@pytest.fixture(scope="module")
def solve_grid():
    return {name: mem for name, mem in A.solve_cases()}


@pytest.fixture(scope="module")
def solve_refs(solve_grid):
    return {name: A.align_ref(mem) for name, mem in solve_grid.items()}


@pytest.fixture(scope="module")
def reduce_grid():
    return {name: (mode, mem, aff) for name, mode, mem, aff in A.reduce_cases()}


# ----------------------------------------------------------------------------------------------- the solve
def test_reference_is_the_brute_force_evaluation(solve_grid, solve_refs):
    """Integer sums and E[xy] - E[x] E[y] against centred float64 moments.  Both carry float64 rounding only (the moments of
    bytes are below 2^16, so their error is below 2^16 * 2^-52 * a few, and the affine's below 1e-9); the reference is then
    rounded to fp32 once: half an ulp of a gain up to 2 (2^-24 * 2) and of an offset up to 512 (2^-24 * 512 = 3.1e-5)."""
    for name, mem in solve_grid.items():
        aff, _ = solve_refs[name]
        brute = A.align_brute(mem)
        assert np.abs(brute[..., 0] - aff[..., 0].astype(np.float64)).max() <= 2.0 ** -23 + 1e-9, name
        assert np.abs(brute[..., 1] - aff[..., 1].astype(np.float64)).max() <= 2.0 ** -15 + 1e-9, name


def test_specification_is_the_reference_on_the_whole_grid(pkg, solve_grid, solve_refs):
    E = pkg.ensemble
    ran = 0
    for name, mem in solve_grid.items():
        N, B, n = mem.shape
        want, stats = solve_refs[name]
        if n % 3 == 0:
            got = E.align_members(_tensors(mem))
            assert got.dtype == torch.float32 and tuple(got.shape) == (N, B, 2) and not got.is_cuda
            assert np.array_equal(_bits(got.numpy()), _bits(want)), name
            assert np.array_equal(_bits(E.align_members(_tensors(mem), backend="torch").numpy()), _bits(want)), name
        for b in range(B):                                           # the rule alone, at every size
            S, G = A.sums_ref(mem[:, b])
            aff, (mean, C) = E.align_solve_members(n, S, G)
            assert aff.dtype == np.float32 and np.array_equal(_bits(aff), _bits(want[:, b])), (name, b)
            assert np.array_equal(np.concatenate([mean, C.reshape(-1)]), stats[b]), (name, b)
        ran += 1
    assert ran == 2 * 16 + 3 * len(A.SOLVE_SIZES) + 7 + 1 + 1


def test_every_branch_of_the_rule_is_hit_by_a_named_case(pkg, solve_grid, solve_refs):
    E = pkg.ensemble

    def parts(name, b=0):
        mem = solve_grid[name]
        N = mem.shape[0]
        aff, stats = solve_refs[name]
        return aff[:, b], stats[b][:N], stats[b][N:].reshape(N, N)
    # N = 2: no third member, moment matching
    aff, mean, C = parts("branch.n2")
    assert aff[1, 0] == np.float32(np.sqrt(C[0, 0] / C[1, 1])) and 0.5 < aff[1, 0] < 1.0 and C[0, 1] > 0
    # a flat member: its own g is 1 (den and C_11 are 0); the member beside it loses its instrument (num = C_01 = 0) and falls
    # back to moment matching
    aff, mean, C = parts("branch.flat")
    assert C[1, 1] == 0 and aff[1, 0] == 1.0 and aff[1, 1] == np.float32(mean[0] - mean[1])
    assert C[0, 1] < A.FLAT and aff[2, 0] == np.float32(np.sqrt(C[0, 0] / C[2, 2]))
    # contents that disagree
    aff, mean, C = parts("branch.anti")
    assert C[0, 1] <= 0 and C[0, 0] >= A.FLAT and C[1, 1] >= A.FLAT and aff[1, 0] == 1.0
    # num below FLAT (member 2 shares nothing with anybody): member 1 falls back to moment matching, member 2 to g = 1 or the same
    aff, mean, C = parts("branch.num_flat")
    assert C[0, 2] < A.FLAT and C[0, 1] > 0 and aff[1, 0] == np.float32(np.sqrt(C[0, 0] / C[1, 1]))
    # den below FLAT with num fine
    aff, mean, C = parts("branch.den_flat")
    assert C[0, 2] >= A.FLAT and C[1, 2] < A.FLAT
    assert aff[1, 0] == (np.float32(np.sqrt(C[0, 0] / C[1, 1])) if C[0, 1] > 0 else 1.0)
    assert aff[2, 0] == np.float32(min(max(C[0, 1] / C[2, 1], 0.5), 2.0)) if C[2, 1] >= A.FLAT and C[0, 1] >= A.FLAT else True
    # both clamps; o from the clamped g
    aff, mean, C = parts("branch.clamp_hi")
    assert (aff[1:, 0] == 2.0).all() and aff[1, 1] == np.float32(mean[0] - np.float64(2.0) * mean[1])
    aff, mean, C = parts("branch.clamp_lo")
    assert (aff[1:, 0] == 0.5).all() and aff[2, 1] == np.float32(mean[0] - np.float64(0.5) * mean[2])
    # the cross rule itself, by hand at N = 3: g_1 = C_02 / C_12, g_2 = C_01 / C_21
    aff, mean, C = parts("members.n3")
    assert aff[1, 0] == np.float32(C[0, 2] / C[1, 2]) and aff[2, 0] == np.float32(C[0, 1] / C[2, 1])
    assert tuple(aff[0]) == (1.0, 0.0)
    # non-finite sums: (1, 0) for every member, from the specification and from the reference
    S, G = A.sums_ref(solve_grid["members.n3"][:, 0])
    for bad in (float("inf"), float("nan")):
        S2 = [S[0], bad, S[2]]
        aff, _ = E.align_solve_members(771, S2, G)
        assert tuple(aff[1]) == (1.0, 0.0) and np.isfinite(aff).all()
        assert np.array_equal(_bits(aff), _bits(A.solve_ref(771, S2, G)[0]))
        G2 = [row[:] for row in G]
        G2[0][0] = bad
        aff, _ = E.align_solve_members(771, S, G2)
        assert (aff[1:] == np.array([1.0, 0.0], dtype=np.float32)).all()
        assert np.array_equal(_bits(aff), _bits(A.solve_ref(771, S, G2)[0]))


def test_solve_grid_tells_every_wrong_stand_in_from_the_reference(solve_grid, solve_refs):
    assert len(A.SOLVE_WRONG) == 10
    for kind, case in A.SOLVE_WRONG.items():
        mem = solve_grid[case]
        want_a, want_s = solve_refs[case]
        got_a, got_s = A.align_ref(mem, kind)
        n_a, n_s = int((_bits(got_a) != _bits(want_a)).sum()), int((got_s != want_s).sum())
        print(f"ensemble_align solve stand-in {kind:22s} at {case:16s}: {n_a} affine values, {n_s} moments differ")
        assert n_a + n_s > 0, (kind, case)
    # the case that carries a 32-bit accumulator past its range: more than 2^32 / 255^2 bytes on one thread of the second launch
    N, B, n = solve_grid["sweep.255"].shape
    rows = A.SOLVE_THREADS // (N + N * (N + 1) // 2)
    assert n > rows * (2 ** 32 // 255 ** 2) + rows * A.CHUNK and n > A.SOLVE_WAVES * A.CHUNK


# ----------------------------------------------------------------------------------------------- the reduce behind an affine
def test_affine_reduce_is_the_reference_on_the_whole_grid(pkg, reduce_grid):
    E = pkg.ensemble
    for name, (mode, mem, aff) in reduce_grid.items():
        a = torch.from_numpy(aff)
        if mem.shape[2] % 3:                 # no whole pixels: no tensor [..., 3]; the apply alone (the reduce behind it is 4m's)
            for k in range(mem.shape[0]):
                assert np.array_equal(E.apply_affine_u8(torch.from_numpy(mem[k].copy()), a[k]).numpy(), A.aligned_ref(mem, aff)[k]), name
            continue
        members = _tensors(mem)
        for spread in (False, True):
            r, sp = E.reduce_members(members, mode, spread=spread, affine=a)
            want_r, want_sp = A.reduce_affine_ref(mem, aff, mode, spread)
            assert r.dtype == torch.uint8 and r.shape == members[0].shape and np.array_equal(r.numpy().reshape(-1), want_r), name
            assert (sp is None) == (not spread)
            if spread:
                assert np.array_equal(sp.numpy().reshape(-1), want_sp), (name, "spread")
        for k in range(mem.shape[0]):
            assert np.array_equal(E.apply_affine_u8(members[k], a[k]).numpy().reshape(mem.shape[1], -1), A.aligned_ref(mem, aff)[k]), name


def test_identity_affine_reproduces_the_reduce_without_one(pkg, reduce_grid):
    E = pkg.ensemble
    for name in ("members.n5.median", "members.n8.mean", "size.51.b3.median", "clamps.mean"):
        mode, mem, aff = reduce_grid[name]
        members = _tensors(mem)
        one = torch.zeros(aff.shape, dtype=torch.float32)
        one[..., 0] = 1.0
        for k in range(mem.shape[0]):
            assert torch.equal(E.apply_affine_u8(members[k], one[k]), members[k])
        a = E.reduce_members(members, mode, spread=True, affine=one)
        b = E.reduce_members(members, mode, spread=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name
    ramp = torch.arange(256, dtype=torch.uint8).repeat(3).view(1, 256, 3)
    assert torch.equal(E.apply_affine_u8(ramp, torch.tensor([[1.0, 0.0]])), ramp)


def test_reduce_grid_tells_every_wrong_stand_in_from_the_reference(reduce_grid):
    assert len(A.REDUCE_WRONG) == 8
    for kind, case in A.REDUCE_WRONG.items():
        mode, mem, aff = reduce_grid[case]
        want_r, want_sp = A.reduce_affine_ref(mem, aff, mode, True)
        got_r, got_sp = A.reduce_affine_ref(mem, aff, mode, True, wrong=kind)
        n_r, n_sp = int((got_r != want_r).sum()), int((got_sp != want_sp).sum())
        print(f"ensemble_align reduce stand-in {kind:30s} at {case:20s}: {n_r} result bytes, {n_sp} spread bytes differ")
        assert n_r + n_sp > 0, (kind, case)
    mode, mem, aff = reduce_grid[A.REDUCE_WRONG["spread_around_the_unaligned"]]
    assert np.array_equal(A.reduce_affine_ref(mem, aff, mode, True, wrong="spread_around_the_unaligned")[0],
                          A.reduce_affine_ref(mem, aff, mode)[0])
    # every FMA-telling triple does tell, at its byte
    for t, (gh, oh, x) in enumerate(A.FMA_TRIPLES):
        g, o = np.float32(float.fromhex(gh)), np.float32(float.fromhex(oh))
        one = np.array([x], dtype=np.uint8)
        assert A.apply_ref(one, g, o)[0] != A.apply_ref(one, g, o, fused=True)[0], t
    # the clamp cases reach both ends
    mode, mem, aff = reduce_grid["clamps.median"]
    al = A.aligned_ref(mem, aff)
    assert (al == 0).any() and (al == 255).any()


def test_aligned_members_are_closer_to_member_0_than_todays_median():
    """Recorded in profiles/ensemble_align_parity.txt.  The condition is the inequality cross rule < moment matching < unaligned
    on the scene with gains; the figures, and the same scene with all gains 1, are printed and not judged."""
    f = A.robustness_figures()
    fmt = lambda v: ", ".join(f"{x:.3f}" for x in v)
    print(f"ensemble_align robustness, N = 5, 20 % salt: mean byte error against member 0's space: today's median "
          f"{f['unaligned']:.3f}, moment matching {f['moment']:.3f}, cross rule {f['cross']:.3f}")
    print(f"ensemble_align robustness, gains: true {fmt(f['true_gains'])}; moment matching {fmt(f['moment_gains'])}; cross rule "
          f"{fmt(f['cross_gains'])}")
    one = A.robustness_figures(gains=(1.0,) * 5, offsets=(0.0,) * 5)
    print(f"ensemble_align robustness, all gains 1: today's median {one['unaligned']:.3f}, moment matching {one['moment']:.3f}, "
          f"cross rule {one['cross']:.3f}; cross-rule gains {fmt(one['cross_gains'])}")
    assert f["cross"] < f["moment"] < f["unaligned"]


# ----------------------------------------------------------------------------------------------- refusals and the walk
def test_refusals_on_the_cpu(pkg):
    E = pkg.ensemble
    chk = E.check_ensemble
    chk(3, "median", ensemble_align=True)
    chk(1, "mean", ensemble_align=False)
    for bad in (1, 0, "yes", None, 1.0, np.bool_(True)):
        with pytest.raises(ValueError, match="ensemble_align"):
            chk(3, "median", ensemble_align=bad)
    m = torch.zeros(2, 4, 3, dtype=torch.uint8)
    one = torch.tensor([[[1.0, 0.0]] * 2] * 2)
    E.reduce_members([m, m], "median", affine=one)
    for kw, match in ((dict(members=[m, m], mode="normal", affine=one), "normal"),
                      (dict(members=[m, m], mode="median", affine=one[:1]), "affine"),
                      (dict(members=[m, m], mode="median", affine=one.double()), "affine"),
                      (dict(members=[m, m], mode="median", affine=one[:, :1]), "affine"),
                      (dict(members=[m[0, 0], m[0, 0]], mode="mean", affine=one), "clips"),
                      (dict(members=[m, m], mode="median", affine=one, backend="hip"), "GPU")):
        with pytest.raises(ValueError, match=match):
            E.reduce_members(**kw)
    for kw, match in ((dict(members=[m, m], backend="cuda"), "backend"), (dict(members=[]), "members"),
                      (dict(members=[m] * 17), "members"), (dict(members=[m, m.float()]), "uint8"),
                      (dict(members=[m, m[:1]]), "one result"), (dict(members=[m[:0], m[:0]]), "clips"),
                      (dict(members=[m, m], backend="hip"), "GPU")):
        with pytest.raises(ValueError, match=match):
            E.align_members(**kw)
    assert torch.equal(E.align_members([m]), torch.tensor([[[1.0, 0.0]] * 2]))       # one member: (1, 0)


def test_reduce_results_aligns_every_pass_but_the_normal_ones(pkg, monkeypatch):
    E = pkg.ensemble
    mem = A.scene("walk", 3, 2, 771, gains=[1.0, 0.7, 1.3], offsets=[0.0, 30.0, -20.0])
    nrm = R._normal_sets(3, A._rng("walk.normals"))[:, :2 * 771].reshape(3, 2, 771)
    outs = lambda: [[[_tensors(mem)[k], _tensors(nrm)[k]], [_tensors(mem[:, ::-1])[k]]] for k in range(3)]
    flags = [[False, True], [False]]
    res, spr, aff = E.reduce_results(outs(), flags, "median", spread=True, align=True)
    want_a, _ = A.align_ref(mem)
    assert np.array_equal(_bits(aff[0][0].numpy()), _bits(want_a)) and aff[0][1] is None
    assert np.array_equal(_bits(aff[1][0].numpy()), _bits(A.align_ref(np.ascontiguousarray(mem[:, ::-1]))[0]))
    r, sp = A.reduce_affine_ref(mem, want_a, "median", True)
    assert np.array_equal(res[0][0].numpy().reshape(-1), r) and np.array_equal(spr[0][0].numpy().reshape(-1), sp)
    assert not np.array_equal(r, R.reduce_ref([m.reshape(-1) for m in mem], "median")[0])    # the affines do move the result
    # the normal pass is today's: a stand-in that aligned it (its members through the affines of their own Gram matrix, or the
    # channel-wise median behind them) gives another picture
    n_r, n_sp = R.reduce_ref([m.reshape(-1) for m in nrm], "normal", True)
    assert np.array_equal(res[0][1].numpy().reshape(-1), n_r) and np.array_equal(spr[0][1].numpy().reshape(-1), n_sp)
    n_aff, _ = A.align_ref(nrm)
    assert not np.array_equal(R.reduce_ref([m.reshape(-1) for m in A.aligned_ref(nrm, n_aff)], "normal")[0], n_r)
    # the members are dropped as their pass is reduced
    held = outs()
    E.reduce_results(held, flags, "mean", align=True)
    assert all(t is None for outs_k in held for batch in outs_k for t in batch)
    # off: two entries and exactly today's calls
    calls = []
    real = E.reduce_members
    monkeypatch.setattr(E, "reduce_members", lambda *a, **k: (calls.append((a[1], k)), real(*a, **k))[1])
    monkeypatch.setattr(E, "align_members", lambda *a, **k: pytest.fail("nothing is solved with the switch off"))
    for kw in ({}, {"align": False}):
        out = E.reduce_results(outs(), flags, "median", spread=True, **kw)
        assert len(out) == 2 and torch.equal(out[0][0][1], res[0][1])
        assert np.array_equal(out[0][0][0].numpy().reshape(-1), R.reduce_ref([m.reshape(-1) for m in mem], "median")[0])
    assert calls == [("median", {"spread": True}), ("normal", {"spread": True}), ("median", {"spread": True})] * 2


# ----------------------------------------------------------------------------------------------- the pipeline
GAINS = {50: (1.0, 0.0), 51: (0.75, 0.12), 52: (1.3, -0.1)}      # seed -> what the recorder's member does to the clean sample


class _GainModel:
    """Stands in for the renderer model: every seed gives the same structured sample at a gain and offset of its own plus a
    little seeded noise - members that differ by known gains; one row per pass, moved by the pass."""
    process_group = None
    net = None

    def __init__(self):
        self.config = {}
        self.vae = StubVAE()
        self.calls, self.seen, self.pipeline = [], [], None

    def to(self, device):
        return self

    def generate_samples_from_batch(self, data_batch, **kw):
        self.calls.append(kw)
        self.seen.append((self.pipeline.restore_plan, self.pipeline.restore_guide))
        P = data_batch["context_index"].shape[0]
        z = self.vae.encode(data_batch["rgb"]).float()
        z = z + data_batch["context_index"][:, 0].float().view(P, 1, 1, 1, 1) * 0.05
        z = z + torch.sin(torch.arange(z[0].numel(), dtype=torch.float32).view(z[0].shape) * 0.37) * 0.3   # structure all seeds share
        g, o = GAINS[kw["seed"]]
        noise = torch.stack([torch.randn(z[0].shape, generator=torch.Generator().manual_seed(kw["seed"] * 7 + int(c))) * 0.02
                             for c in data_batch["context_index"][:, 0]])          # a pass is the same sample alone and in a batch
        return (g * z + o + noise).to(BF)

    def decode(self, sample):
        return self.vae.decode(sample)


@pytest.fixture
def rig(pkg, monkeypatch):
    import window_refs as WR
    mod = pkg.diffusion_renderer_pipeline
    monkeypatch.setattr(mod.N, "postprocess_window_u8",
                        lambda video, prev, ramp, ramp_at, lo, hi, normalize, out=None: WR.blend_postprocess(video, prev, ramp, ramp_at,
                                                                                                              lo, hi, normalize))
    model = _GainModel()
    p = mod.CleanDiffusionRendererPipeline("/nonexistent", "x.pt", model_type=None, model_instance=model, guidance=0.0, num_steps=2)
    p.device = torch.device("cpu")
    p.set_model_type("inverse")
    model.pipeline = p
    rgb = pkg.synthetic_weights.synth_tensor("ensemble_align.pipe.rgb", (1, 3, 17, 48, 64), torch.float32, scale=0.6)
    batch = {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[0], [3]], dtype=torch.long)}
    return mod, p, model, batch


_compose = A.compose_ref


@pytest.mark.parametrize("path", ("whole_clip", "windowed", "pixel_tiled"))
def test_member_loop_aligns_known_gains_and_reduces_through_them(rig, path):
    mod, p, model, batch = rig
    if path == "windowed":
        p.window_frames, p.window_overlap = 9, 2
    if path == "pixel_tiled":
        p.tile_height, p.tile_width, p.tile_overlap = 32, 32, 8
    flags = [False, True]
    assert p.ensemble_align is False and p.last_ensemble_align == []
    members = [p.generate_video_passes(batch, flags, seed=50 + k) for k in range(3)]
    per_member = len(model.calls) // 3
    p.ensemble = 3
    plain = p.generate_video_passes(batch, flags, seed=50)
    assert p.last_ensemble_align == []
    del model.calls[:]
    for reduce in ("median", "mean"):
        p.ensemble_reduce, p.ensemble_align = reduce, True
        got = p.generate_video_passes(batch, flags, seed=50)
        want = _compose(members, flags, reduce)
        for g, (w, _, _) in zip(got, want):
            assert isinstance(g, np.ndarray) and g.dtype == np.uint8 and np.array_equal(g, w), (path, reduce)
        (a0, a1), = p.last_ensemble_align
        assert a1 is None and a0.dtype == torch.float32 and tuple(a0.shape) == (3, 1, 2)
        assert np.array_equal(_bits(a0.numpy()), _bits(want[0][2]))
    assert [c["seed"] for c in model.calls] == ([50] * per_member + [51] * per_member + [52] * per_member) * 2
    # the members differ by known gains, and the solve finds them: g_k ~ g_0 / g_k, far from (1, 0); the result is not today's
    gains = a0[:, 0, 0].numpy()
    assert gains[0] == 1.0 and a0[0, 0, 1] == 0.0
    for k in (1, 2):
        assert abs(gains[k] - 1.0 / GAINS[50 + k][0]) < 0.08, (k, gains)
    assert not np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])     # the normal pass is never aligned
    # aligned, the members agree with member 0 more closely than they did raw
    raw = np.mean([np.abs(m[0].astype(np.int64) - members[0][0]).mean() for m in members[1:]])
    mem = np.stack([np.ascontiguousarray(m[0]).reshape(1, -1) for m in members])
    al = A.aligned_ref(mem, want[0][2])
    assert np.mean([np.abs(al[k].astype(np.int64) - al[0]).mean() for k in (1, 2)]) < 0.25 * raw
    # the other public calls; the device results; the spread around the aligned members
    each = [dict(batch, context_index=batch["context_index"][i:i + 1]) for i in range(2)]
    b = p.generate_video_each(each, flags, seed=50, to_host=False)
    assert isinstance(b[0], torch.Tensor) and np.array_equal(b[0].numpy(), got[0]) and np.array_equal(b[1].numpy(), got[1])
    assert len(p.last_ensemble_align) == 2 and p.last_ensemble_align[1] == [None]
    res, spr = p.generate_video_ensemble(each, flags, seed=50)
    want = _compose(members, flags, "mean", spread=True)
    for i in range(2):
        assert np.array_equal(res[i], want[i][0]) and np.array_equal(spr[i], want[i][1])
    # ignored at ensemble = 1; False set explicitly is the default call
    p.ensemble = 1
    assert np.array_equal(p.generate_video_passes(batch, flags, seed=50)[0], members[0][0]) and p.last_ensemble_align == []
    res1, spr1 = p.generate_video_ensemble(each, flags, seed=50)
    assert np.array_equal(res1[0], members[0][0]) and not spr1[0].any() and p.last_ensemble_align == []
    p.ensemble, p.ensemble_align, p.ensemble_reduce = 3, False, "median"
    again = p.generate_video_passes(batch, flags, seed=50)
    assert all(np.array_equal(a, b) for a, b in zip(again, plain)) and p.last_ensemble_align == []


def test_off_the_walk_makes_exactly_todays_calls(rig, monkeypatch):
    mod, p, model, batch = rig
    seen = []
    real = mod.reduce_results
    monkeypatch.setattr(mod, "reduce_results", lambda *a, **k: (seen.append((len(a), dict(k))), real(*a, **k))[1])
    p.ensemble = 3
    p.generate_video_passes(batch, [False, True], seed=50)
    p.ensemble_align = False
    p.generate_video_passes(batch, [False, True], seed=50)
    assert seen == [(3, {"spread": False})] * 2
    p.ensemble_align = True
    p.generate_video_passes(batch, [False, True], seed=50)
    assert seen[-1] == (3, {"spread": False, "align": True})


def test_restore_runs_once_after_the_aligned_reduce(rig, monkeypatch):
    import dataclasses

    @dataclasses.dataclass
    class Plan:
        T: int
    mod, p, model, batch = rig
    flags = [False, True]
    members = [p.generate_video_passes(batch, flags, seed=50 + k) for k in range(3)]
    want = _compose(members, flags, "median")
    plain = []

    def restore(u8, plan):
        plain.append(u8.clone())
        return u8[:, :plan.T, ::2]
    monkeypatch.setattr(mod, "restore_frames", restore)
    plan = Plan(T=11)
    p.restore_plan, p.ensemble, p.ensemble_align = plan, 3, True
    del model.seen[:]
    got = p.generate_video_passes(batch, flags, seed=50)
    assert all(s == (None, None) for s in model.seen) and p.restore_plan is plan
    assert len(plain) == 2
    for u8, (w, _, _), g in zip(plain, want, got):
        assert np.array_equal(u8.numpy(), w) and np.array_equal(g, w[:, :11, ::2])


def test_a_bad_switch_is_refused_before_any_model_call(rig):
    mod, p, model, batch = rig
    each = [dict(batch, context_index=batch["context_index"][i:i + 1]) for i in range(2)]
    for bad in (1, "on", None):
        p.ensemble_align = bad
        for call in (lambda: p.generate_video(each[0]), lambda: p.generate_video_passes(batch, [False, True]),
                     lambda: p.generate_video_each(each, [False, True]), lambda: p.generate_video_ensemble(each, [False, True])):
            with pytest.raises(ValueError, match="ensemble_align"):
                call()
    assert not model.calls


# ----------------------------------------------------------------------------------------------- nodes
class _Recorder:
    """A plain object where the pipeline stands: records what the nodes set and hand over, and every look at its device."""

    def __init__(self):
        self.num_steps = 15
        self.calls, self.touched = [], []

    @property
    def device(self):
        self.touched.append("device")
        return "cpu"

    def set_model_type(self, kind):
        self.touched.append("set_model_type")
        self.kind = kind

    def _out(self, data_batch, to_host):
        ref = data_batch.get("rgb", data_batch.get("depth"))
        B, _, T, H, W = ref.shape
        o = torch.zeros(B, T, H, W, 3, dtype=torch.uint8)
        return o.numpy() if to_host else o

    def generate_video(self, data_batch, normalize_normal=False, seed=None, to_host=True):
        self.calls.append((self.kind, self.ensemble, self.ensemble_align))
        return self._out(data_batch, to_host)

    def generate_video_passes(self, data_batch, normalize_normal, seed=None, to_host=True):
        self.calls.append((self.kind, self.ensemble, self.ensemble_align))
        return [self._out(data_batch, to_host) for _ in normalize_normal]


def test_node_inputs_and_what_the_nodes_set(pkg):
    inv_c, fwd_c = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"], pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]
    rel_c = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]
    for cls in (inv_c, rel_c):
        kind, o = cls.INPUT_TYPES()["optional"]["ensemble_align"]
        assert kind == "BOOLEAN" and o["default"] is False and "gain and offset" in o["tooltip"]
    assert "ensemble_align" not in fwd_c.INPUT_TYPES()["optional"]
    sw = pkg.synthetic_weights
    image = sw.synth_tensor("ensemble_align.node", (1, 9, 48, 64, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("ensemble_align.env", (1, 16, 32, 3), torch.float32).abs()
    inv, fwd, rel = inv_c(), fwd_c(), rel_c()
    r = _Recorder()
    inv.run_inverse_pass(r, image)
    inv.run_inverse_pass(r, image, ensemble=3, ensemble_align=True)
    inv.run_inverse_pass(r, image, ensemble_align=True)                          # set as given; the pipeline ignores it at 1
    inv.run_inverse_pass(r, image, ensemble=3)
    assert r.calls == [("inverse", 1, False), ("inverse", 3, True), ("inverse", 1, True), ("inverse", 3, False)]
    r = _Recorder()
    r.ensemble, r.ensemble_align = 4, True                                       # left behind by an inverse run on the same object
    fwd.run_forward_pass(r, *[image] * 5, env)
    assert r.calls == [("forward", 1, False)]
    with pytest.raises(TypeError):
        fwd.run_forward_pass(_Recorder(), *[image] * 5, env, ensemble_align=True)
    r = _Recorder()
    rel.run_relight(r, r, image, env, ensemble=3, ensemble_align=True)
    assert r.calls == [("inverse", 3, True), ("forward", 1, False)]
    # refused before anything is set or uploaded
    u8 = torch.zeros(1, 9, 48, 64, 3, dtype=torch.uint8)
    for bad in (1, "yes", None):
        r = _Recorder()
        for run in (lambda: inv.run_inverse_pass(r, u8, ensemble=2, ensemble_align=bad),
                    lambda: rel.run_relight(r, r, u8, env, ensemble=2, ensemble_align=bad)):
            with pytest.raises(ValueError, match="ensemble_align"):
                run()
        assert not r.calls and not r.touched and not hasattr(r, "ensemble_align"), bad
