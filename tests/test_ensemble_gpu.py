"""Seed ensembles on the GPU: drn_ensemble_reduce_u8 bit for bit against tests/ensemble_refs.py on the case grid that
tests/test_ensemble_cpu.py shows to separate every wrong stand-in - with and without the spread, every buffer at byte offsets
0..3 inside sentinel guard bands compared whole, members as views into one allocation and as allocations of their own, every
launch twice -, the entry's refusals, the dispatch of ensemble.reduce_members, and the pipeline and the nodes at ensemble = 3
against the reduce by hand of three ensemble = 1 calls."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import ensemble_refs as R
from conftest import tiny_net
from stub_vae import StubVAE

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GUARD = 32                       # bytes of sentinel on both sides of every buffer
SENT = 0xA5
MODE = {"median": 0, "mean": 1, "normal": 2}
EINVAL = -1


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Arena:
    """Buffers of n bytes at byte offsets inside guard bands.  together: all of them views into ONE device allocation (every
    buffer's region starts on the 16-byte grid); otherwise every buffer is an allocation of its own."""

    def __init__(self, gpu, payloads, n, offs, together):
        self.n = n
        region = (GUARD + 3 + n + GUARD + 15) // 16 * 16
        self.los = [(i * region if together else 0) + GUARD + off for i, off in enumerate(offs)]
        self.which = [0 if together else i for i in range(len(offs))]
        hosts = [np.full(region * (len(offs) if together else 1), SENT, dtype=np.uint8) for _ in range(1 if together else len(offs))]
        for lo, w, payload in zip(self.los, self.which, payloads):
            if payload is not None:
                hosts[w][lo:lo + n] = payload
        self.hosts = hosts
        self.devs = [torch.from_numpy(h).to(gpu) for h in hosts]
        assert all(d.data_ptr() % 16 == 0 for d in self.devs)

    def ptr(self, i):
        return self.devs[self.which[i]].data_ptr() + self.los[i]

    def check(self, expect, tag):
        """expect: buffer index -> the bytes it must hold now (the others: what they held); everything compared whole."""
        want = [h.copy() for h in self.hosts]
        for i, payload in expect.items():
            want[self.which[i]][self.los[i]:self.los[i] + self.n] = payload
        for d, w in zip(self.devs, want):
            assert np.array_equal(d.cpu().numpy(), w), tag


def _run_case(pkg, gpu, name, mode, mem, want_r, want_sp, offs, together):
    """members 0..N-1, dst = N, spread = N + 1; without the spread, then with it; every launch twice."""
    lib = pkg.native.load_library()
    N, n = mem.shape
    for spread in (False, True):
        arena = _Arena(gpu, list(mem) + [None, None], n, offs, together)
        table = (ctypes.c_void_p * N)(*[arena.ptr(k) for k in range(N)])
        for run in range(2):
            rc = lib.drn_ensemble_reduce_u8(table, N, arena.ptr(N), arena.ptr(N + 1) if spread else None, n, MODE[mode], _stream())
            assert rc == 0, (name, rc)
            torch.cuda.synchronize()
            arena.check({N: want_r, N + 1: want_sp} if spread else {N: want_r}, (name, "spread" if spread else "plain", "run", run))


def _variants(idx, N):
    """(byte offsets of the N members, dst and spread; together) - all on the 16-byte grid (the wide path), then ragged."""
    yield [0] * (N + 2), bool(idx % 2)
    yield [(idx + k) % 4 for k in range(N)] + [(idx + 1) % 4, (idx + 2) % 4 or 3], not idx % 2


GROUPS = ("size", "members", "pairs", "sets", "normals")


@pytest.mark.parametrize("group", GROUPS)
def test_kernel_is_the_reference_on_the_grid(pkg, gpu, group):
    ran = 0
    for idx, (name, mode, mem) in enumerate(R.cases(big=False)):
        if name.split(".")[0] != group:
            continue
        want_r, want_sp = R.reduce_ref(list(mem), mode, True)
        for offs, together in _variants(idx, mem.shape[0]):
            _run_case(pkg, gpu, name, mode, mem, want_r, want_sp, offs, together)
        ran += 1
    assert ran == {"size": 3 * len(R.SIZES), "members": 48, "pairs": 2, "sets": 2 * len(R.SET_N), "normals": len(R.SET_N) + 3}[group]


BIG = ("sweep.median", "sweep.normal", "sweep.mean", "sweep.median.ragged", "sweep.mean.ragged", "sweep.normal.ragged")


@pytest.mark.parametrize("which", BIG)
def test_kernel_is_the_reference_past_one_sweep_of_the_capped_grid(pkg, gpu, which):
    """More lanes' worth of work than the capped grid has: every lane takes a second piece (64-bit offsets, the strided loop)."""
    (name, mode, mem), = [c for c in R.big_cases() if c[0] == which]
    want_r, want_sp = R.reduce_ref(list(mem), mode, True)
    N = mem.shape[0]
    ragged = which.endswith(".ragged")
    lanes_work = mem.shape[1] // (1 if ragged else 16) // (3 if mode == "normal" else 1)
    assert lanes_work > R.SWEEP_LANES
    offs = [1 + k % 3 for k in range(N)] + [2, 3] if ragged else [0] * (N + 2)
    _run_case(pkg, gpu, name, mode, mem, want_r, want_sp, offs, together=not ragged)


def test_refusals_of_the_entry(pkg, gpu):
    lib = pkg.native.load_library()
    n = 96
    mem = np.arange(3 * n, dtype=np.uint8).reshape(3, n)
    arena = _Arena(gpu, list(mem) + [None, None], n, [0] * 5, True)
    ptrs = [arena.ptr(k) for k in range(5)]

    def call(members=ptrs[:3], N=3, dst=ptrs[3], spread=ptrs[4], n_bytes=n, mode=0, null_table=False):
        table = None if null_table else (ctypes.c_void_p * max(len(members), 1))(*members)
        return lib.drn_ensemble_reduce_u8(table, N, dst, spread, n_bytes, mode, _stream())
    bad = {"null members": dict(null_table=True), "null member": dict(members=[ptrs[0], None, ptrs[2]]), "null dst": dict(dst=None),
           "N = 0": dict(N=0), "N = 17": dict(members=ptrs[:1] * 17, N=17), "N < 0": dict(N=-1), "mode -1": dict(mode=-1),
           "mode 3": dict(mode=3), "n_bytes < 0": dict(n_bytes=-3), "cut pixel": dict(mode=2, n_bytes=n - 1),
           "dst == spread": dict(spread=ptrs[3]), "dst is a member": dict(dst=ptrs[1]), "spread is a member": dict(spread=ptrs[2])}
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
    assert call(n_bytes=0) == 0 and call(n_bytes=0, mode=2, spread=None) == 0
    torch.cuda.synchronize()
    arena.check({}, "nothing was launched")
    assert call(n_bytes=n - 1, mode=1) == 0                       # a cut pixel is nobody's business outside mode 2
    torch.cuda.synchronize()
    want_r, want_sp = R.reduce_ref(list(mem[:, :n - 1]), "mean", True)
    arena.check({3: np.concatenate([want_r, [SENT]]), 4: np.concatenate([want_sp, [SENT]])}, "mean")


def test_dispatch_of_reduce_members(pkg, gpu):
    E = pkg.ensemble
    rng = np.random.default_rng(11)
    mem = rng.integers(0, 256, size=(5, 2, 7, 33, 3), dtype=np.uint8)
    flat = [m.reshape(-1) for m in mem]
    cpu = [torch.from_numpy(m) for m in mem]
    dev = [t.to(gpu) for t in cpu]
    dev[1] = torch.from_numpy(np.ascontiguousarray(mem[1].transpose(1, 0, 2, 3))).to(gpu).permute(1, 0, 2, 3)   # not contiguous
    assert not dev[1].is_contiguous()
    for mode in R.MODES:
        want_r, want_sp = R.reduce_ref(flat, mode, True)
        for backend in ("auto", "hip"):
            r, sp = E.reduce_members(dev, mode, spread=True, backend=backend)
            assert r.is_cuda and r.dtype == torch.uint8 and r.shape == sp.shape == (2, 7, 33, 3)
            assert np.array_equal(r.cpu().numpy().reshape(-1), want_r) and np.array_equal(sp.cpu().numpy().reshape(-1), want_sp)
            assert E.reduce_members(dev, mode, backend=backend)[1] is None
        r, sp = E.reduce_members(cpu, mode, spread=True)                          # auto on the CPU: torch
        assert not r.is_cuda and np.array_equal(r.numpy().reshape(-1), want_r) and np.array_equal(sp.numpy().reshape(-1), want_sp)
        with pytest.raises(ValueError, match="GPU"):
            E.reduce_members(cpu, mode, backend="hip")
        if mode != "normal":                                                      # integers: the torch path on the device too
            r, sp = E.reduce_members(dev, mode, spread=True, backend="torch")
            assert r.is_cuda and np.array_equal(r.cpu().numpy().reshape(-1), want_r)
            assert np.array_equal(sp.cpu().numpy().reshape(-1), want_sp)
    with pytest.raises(ValueError, match="one result"):
        E.reduce_members([dev[0], cpu[2]], "median")
    # the kernel path builds no stack: beyond the members it holds the result and the spread
    big = [torch.randint(0, 256, (1 << 20, 3), dtype=torch.uint8, device=gpu) for _ in range(8)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    r, sp = E.reduce_members(big, "median", spread=True)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before <= 2 * big[0].numel() + (1 << 20)
    assert np.array_equal(r[:99].cpu().numpy().reshape(-1), R.reduce_ref([b[:99].cpu().numpy().reshape(-1) for b in big], "median")[0])
    empty = E.reduce_members([big[0][:0], big[1][:0]], "normal", spread=True)          # nothing to reduce: nothing launched
    assert empty[0].shape == empty[1].shape == (0, 3)


# ----------------------------------------------------------------------------------------------- pipeline and nodes
H, W = 48, 64


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
        "/nonexistent", "x.pt", model_type=None, vae_instance=StubVAE(), model_instance=models, guidance=0.0, num_steps=2)
    p.device = gpu
    p.set_model_type("inverse")
    return p


@pytest.fixture(scope="module")
def pipe(pkg, gpu):
    return _pipeline(pkg, gpu)


def _reset(p):
    p.set_model_type("inverse")
    p.guidance, p.restore_plan, p.restore_guide, p.num_steps, p.sampler = 0.0, None, None, 2, "euler"
    p.window_frames, p.window_overlap, p.tile_height, p.tile_width, p.tile_overlap, p.tile_join = 0, 8, 0, 0, 64, "pixel"
    p.window_align, p.ensemble, p.ensemble_reduce = False, 1, "median"


def _reduce_by_hand(members, flags, reduce):
    """members[k][i]: member k's uint8 result i (array or tensor) -> per result the reference's reduce, as arrays."""
    out = []
    for i, flag in enumerate(flags):
        arrs = [np.ascontiguousarray(torch.as_tensor(m[i]).cpu().numpy()) for m in members]
        r, _ = R.reduce_ref([a.reshape(-1) for a in arrs], "normal" if flag else reduce)
        out.append(r.reshape(arrs[0].shape))
    return out


PATHS = {
    "whole_clip": dict(),
    "windowed": dict(window_frames=9, window_overlap=2),
    "windows_aligned": dict(window_frames=9, window_overlap=2, window_align=True),
    "pixel_tiled": dict(tile_height=32, tile_width=32, tile_overlap=8),
    "latent_tiled": dict(tile_height=32, tile_width=32, tile_overlap=8, tile_join="latent"),
    "dpmpp_2m": dict(sampler="dpmpp_2m", num_steps=3),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_pipeline_at_ensemble_3_is_three_calls_reduced_by_hand(pkg, gpu, pipe, path):
    p = pipe
    _reset(p)
    for k, v in PATHS[path].items():
        setattr(p, k, v)
    T = 17 if "window" in path else 9
    rgb = pkg.synthetic_weights.synth_tensor(f"ensemble.gpu.clip{T}", (1, 3, T, H, W), torch.float32, scale=1.0)
    batch = {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[0], [3]], dtype=torch.long)}
    flags = [False, True]
    p.guidance, seed = 1.5, 2 ** 64 - 2 if path == "whole_clip" else 5                  # (the whole clip also wraps the seed)
    members = [p.generate_video_passes(batch, flags, seed=(seed + k) & (2 ** 64 - 1), to_host=False) for k in range(3)]
    assert not torch.equal(members[0][0], members[1][0]) and not torch.equal(members[0][1], members[2][1])
    default = p.generate_video_passes(batch, flags, seed=seed)
    for reduce in ("median", "mean"):
        p.ensemble, p.ensemble_reduce = 3, reduce
        want = _reduce_by_hand(members, flags, reduce)
        got = p.generate_video_passes(batch, flags, seed=seed)
        dev = p.generate_video_passes(batch, flags, seed=seed, to_host=False)
        for g, d, w in zip(got, dev, want):
            assert isinstance(g, np.ndarray) and g.shape == (1, T, H, W, 3) and np.array_equal(g, w), (path, reduce)
            assert d.is_cuda and d.dtype == torch.uint8 and torch.equal(d.cpu(), torch.from_numpy(w)), (path, reduce)
    assert np.array_equal(got[1], _reduce_by_hand(members, flags, "median")[1])          # the normal pass ignores ensemble_reduce
    # ensemble = 1 set explicitly is the default call
    p.ensemble = 1
    again = p.generate_video_passes(batch, flags, seed=seed)
    assert all(np.array_equal(a, b) for a, b in zip(default, again))
    assert all(np.array_equal(a, m.cpu().numpy()) for a, m in zip(default, members[0]))
    _reset(p)


def test_pipeline_ensemble_with_a_restore_plan_restores_once_after_the_reduce(pkg, gpu, pipe):
    fit = importlib.import_module(pkg.__name__ + ".fit")
    p = pipe
    _reset(p)
    image = pkg.synthetic_weights.synth_tensor("ensemble.gpu.img", (1, 7, 60, 56, 3), torch.float32).abs().clamp(max=1.0)
    plan = fit.plan_fit(7, 60, 56, "stretch", H, W)
    clip = fit.fit_frames(image, plan, device=gpu)
    ci = torch.tensor([[0], [3]], dtype=torch.long)
    each = [{"rgb": clip, "video": clip, "context_index": ci[i:i + 1]} for i in range(2)]
    flags = [False, True]
    members = [p.generate_video_each(each, flags, seed=9 + k, to_host=False) for k in range(3)]
    rplan = fit.plan_restore(plan)
    p.restore_plan, p.ensemble = rplan, 3
    got = p.generate_video_each(each, flags, seed=9)
    res, spr = p.generate_video_ensemble(each, flags, seed=9)
    assert p.restore_plan is rplan
    for i, flag in enumerate(flags):
        flat = [m[i].cpu().numpy().reshape(-1) for m in members]
        r, sp = R.reduce_ref(flat, "normal" if flag else "median", True)
        shape = tuple(members[0][i].shape)
        want = fit.restore_frames(torch.from_numpy(r.reshape(shape)).to(gpu), rplan).cpu().numpy()
        want_sp = fit.restore_frames(torch.from_numpy(sp.reshape(shape)).to(gpu), rplan).cpu().numpy()
        assert got[i].shape == want.shape == (1, 7, 60, 56, 3) and np.array_equal(got[i], want)
        assert np.array_equal(res[i], want) and spr[i].shape == want.shape and np.array_equal(spr[i], want_sp)
        # restoring every member first is another picture
        early = [fit.restore_frames(m[i], rplan).cpu().numpy().reshape(-1) for m in members]
        assert not np.array_equal(R.reduce_ref(early, "normal" if flag else "median")[0].reshape(want.shape), want)
    # refusals from settings alone
    p.ensemble = 2
    with pytest.raises(ValueError, match="init_noise"):
        p.generate_video(each[0], seed=9, init_noise=torch.zeros(1, 16, 2, 6, 8, device=gpu, dtype=BF))
    p.ensemble = 17
    with pytest.raises(ValueError, match="ensemble"):
        p.generate_video(each[0], seed=9)
    _reset(p)


def test_nodes_at_ensemble_3_are_the_composition_by_hand(pkg, gpu, pipe):
    p = pipe
    _reset(p)
    sw = pkg.synthetic_weights
    T = 9
    image = sw.synth_tensor("ensemble.node.img", (1, T, H, W, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("ensemble.node.env", (1, 32, 64, 3), torch.float32).abs() * 4.0
    inv = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    fwd = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    rel = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    normal_at = 3                                                                 # RETURN_NAMES: base_color, metallic, roughness, normal, depth
    members = [inv.run_inverse_pass(p, image, guidance=1.0, seed=(3 + k)) for k in range(3)]
    assert p.ensemble == 1
    for reduce in ("median", "mean"):
        got = inv.run_inverse_pass(p, image, guidance=1.0, seed=3, ensemble=3, ensemble_reduce=reduce)
        assert (p.ensemble, p.ensemble_reduce) == (3, reduce) and len(got) == 5
        for i in range(5):
            u8 = [(m[i] * 255.0).round().to(torch.uint8).numpy().reshape(-1) for m in members]
            want, _ = R.reduce_ref(u8, "normal" if i == normal_at else reduce)
            assert torch.equal(got[i], torch.from_numpy(want.reshape(tuple(got[i].shape))).float() / 255.0), (reduce, i)
    # relight: the ensemble belongs to the inverse stage; the forward stage renders one sample from the reduced G-buffers
    out = rel.run_relight(p, p, image, env, guidance=1.0, seed=3, env_spin=45.0, ensemble=3, ensemble_reduce="mean")
    assert p.ensemble == 1 and p.model_type == "forward"
    for a, b in zip(out[1:], got):
        assert torch.equal(a, b)
    g5 = [o.reshape(1, T, H, W, 3) for o in got]
    (lit,) = fwd.run_forward_pass(p, g5[4], g5[3], g5[2], g5[1], g5[0], env, guidance=0.0, seed=3, env_spin=45.0)
    assert torch.equal(out[0], lit)
    _reset(p)
