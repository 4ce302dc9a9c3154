"""Ensembles that agree on the GPU: drn_ensemble_align_affine and drn_ensemble_reduce_affine_u8 bit for bit against
tests/ensemble_align_refs.py on the case grids that tests/test_ensemble_align_cpu.py shows to separate every wrong stand-in - every
buffer inside sentinel guard bands compared whole, the byte buffers at byte offsets 0..3 (the fp32 and fp64 ones at offsets on
their own grids), every launch twice with the workspace and the outputs poisoned in between -, the refusals of both entries, the
dispatch of ensemble.align_members / reduce_members, and the pipeline and the nodes at ensemble = 3 with ensemble_align against
three ensemble = 1 calls composed by hand from the specification."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import ensemble_align_refs as A
import ensemble_refs as R
from conftest import tiny_net
from stub_vae import StubVAE

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GUARD = 32                       # bytes of sentinel on both sides of every buffer
SENT = 0xA5
POISON = 0xFF
MODE = {"median": 0, "mean": 1}
EINVAL = -1


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Buf:
    """n bytes at a byte offset inside guard bands, an allocation of its own (its region starts on the 16-byte grid)."""

    def __init__(self, gpu, n, off=0, payload=None):
        self.n, self.lo = n, GUARD + off
        self.host = np.full((GUARD + off + n + GUARD + 15) // 16 * 16, SENT, dtype=np.uint8)
        if payload is not None:
            self.host[self.lo:self.lo + n] = np.frombuffer(np.ascontiguousarray(payload).tobytes(), dtype=np.uint8)
        self.dev = torch.from_numpy(self.host).to(gpu)
        assert self.dev.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.lo

    def poison(self):
        self.dev[self.lo:self.lo + self.n] = POISON

    def check(self, payload, tag, inside=True):
        """Guard bands intact and (inside) the payload what it must be; payload None: what the buffer held."""
        got = self.dev.cpu().numpy()
        want = self.host.copy()
        if payload is not None:
            want[self.lo:self.lo + self.n] = np.frombuffer(np.ascontiguousarray(payload).tobytes(), dtype=np.uint8)
        if not inside:
            want[self.lo:self.lo + self.n] = got[self.lo:self.lo + self.n]
        assert np.array_equal(got, want), tag


def _table(bufs):
    return (ctypes.c_void_p * len(bufs))(*[b.ptr for b in bufs])


# ----------------------------------------------------------------------------------------------- the solve
def _run_solve(pkg, gpu, name, mem, want, moffs, aoff, soff, woff):
    lib = pkg.native.load_library()
    N, B, n = mem.shape
    want_a, want_s = want
    members = [_Buf(gpu, B * n, moffs[k], mem[k]) for k in range(N)]
    nbytes = lib.drn_ensemble_align_workspace_bytes(N, B, n)
    assert nbytes == B * -(-n // A.CHUNK) * (N + N * (N + 1) // 2) * 4
    aff, st, ws = _Buf(gpu, N * B * 8, aoff), _Buf(gpu, B * (N + N * N) * 8, soff), _Buf(gpu, nbytes, woff)
    ws.poison()
    for run, with_stats in enumerate((True, False, True)):
        rc = lib.drn_ensemble_align_affine(_table(members), N, B, n, aff.ptr, st.ptr if with_stats else None, ws.ptr, nbytes, _stream())
        assert rc == 0, (name, rc)
        torch.cuda.synchronize()
        aff.check(want_a, (name, "affine", run))
        st.check(want_s if with_stats else None, (name, "stats", run))
        ws.check(None, (name, "workspace guards", run), inside=False)
        for k, m in enumerate(members):
            m.check(None, (name, "member", k))
        aff.poison(), ws.poison()
        if with_stats:
            st.dev[st.lo:st.lo + st.n] = SENT


def _solve_variants(idx, N):
    """(member byte offsets, affine / stats / workspace offsets): everything on the 16-byte grid, then ragged."""
    yield [0] * N, 0, 0, 0
    yield [(idx + k) % 4 for k in range(N)], 4 * (1 + idx % 3), 8, 8


SOLVE_GROUPS = ("members", "wide", "size", "branch", "clips")


@pytest.fixture(scope="module")
def solve_grid():
    return [(name, mem, A.align_ref(mem)) for name, mem in A.solve_cases(big=False)]


@pytest.mark.parametrize("group", SOLVE_GROUPS)
def test_solve_is_the_reference_on_the_grid(pkg, gpu, solve_grid, group):
    ran = 0
    for idx, (name, mem, want) in enumerate(solve_grid):
        if name.split(".")[0] != group:
            continue
        for moffs, aoff, soff, woff in _solve_variants(idx, mem.shape[0]):
            _run_solve(pkg, gpu, name, mem, want, moffs, aoff, soff, woff)
        ran += 1
    assert ran == {"members": 16, "wide": 16, "size": 3 * len(A.SOLVE_SIZES), "branch": 7, "clips": 1}[group]


def test_solve_is_the_reference_past_one_sweep_of_the_capped_grid(pkg, gpu):
    """Every byte 255 at N = 3, more chunks than the capped grid has workgroups: the second chunk of a workgroup, 64-bit sums."""
    (name, mem), = [c for c in A.solve_cases() if c[0] == "sweep.255"]
    N, B, n = mem.shape
    assert n > A.SOLVE_WAVES * A.CHUNK and n % 16 == 0
    S = [255 * n] * 3
    G = [[255 * 255 * n] * 3 for _ in range(3)]
    aff, stats = A.solve_ref(n, S, G)                                # the sums of a constant clip, without walking it
    want = (aff[:, None, :], stats[None])
    assert np.array_equal(want[0], A.align_ref(mem[:, :, :3 * A.CHUNK])[0])               # flat: (1, 0) for every member
    _run_solve(pkg, gpu, name, mem, want, [0, 0, 0], 0, 0, 0)
    _run_solve(pkg, gpu, name + ".ragged", mem, want, [1, 2, 3], 4, 8, 8)


def test_refusals_of_the_solve(pkg, gpu):
    lib = pkg.native.load_library()
    N, B, n = 3, 2, 96
    mem = A.scene("refusals", N, B, n)
    members = [_Buf(gpu, B * n, 0, mem[k]) for k in range(N)]
    nbytes = lib.drn_ensemble_align_workspace_bytes(N, B, n)
    aff, st, ws = _Buf(gpu, N * B * 8 + 8), _Buf(gpu, B * (N + N * N) * 8 + 8), _Buf(gpu, nbytes + 8)
    ptrs = [m.ptr for m in members]

    def call(members=ptrs, N=N, B=B, clip_bytes=n, affine=aff.ptr, stats=st.ptr, workspace=ws.ptr, workspace_bytes=nbytes,
             null_table=False):
        table = None if null_table else (ctypes.c_void_p * max(len(members), 1))(*members)
        return lib.drn_ensemble_align_affine(table, N, B, clip_bytes, affine, stats, workspace, workspace_bytes, _stream())
    bad = {"null members": dict(null_table=True), "null member": dict(members=[ptrs[0], None, ptrs[2]]), "null affine": dict(affine=None),
           "null workspace": dict(workspace=None), "N = 0": dict(N=0), "N = 17": dict(members=ptrs[:1] * 17, N=17), "N < 0": dict(N=-1),
           "B = 0": dict(B=0), "B = 65536": dict(B=65536, workspace_bytes=1 << 40), "clip_bytes = 0": dict(clip_bytes=0),
           "clip_bytes < 0": dict(clip_bytes=-3), "clip_bytes > 2^36": dict(clip_bytes=2 ** 36 + 1, workspace_bytes=1 << 50),
           "short workspace": dict(workspace_bytes=nbytes - 1), "affine off 4": dict(affine=aff.ptr + 2),
           "stats off 8": dict(stats=st.ptr + 4), "workspace off 8": dict(workspace=ws.ptr + 4, workspace_bytes=nbytes)}
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
    torch.cuda.synchronize()
    for b in members + [aff, st, ws]:
        b.check(None, "nothing was launched")
    # the workspace is host arithmetic, and 0 for what the entry refuses
    wsb = lib.drn_ensemble_align_workspace_bytes
    assert wsb(16, 1, 57 * 576 * 1024 * 3) == -(-57 * 576 * 1024 * 3 // 8192) * 152 * 4
    assert wsb(3, 2, 2 ** 36) == 2 * (2 ** 36 // 8192) * 9 * 4
    assert [wsb(0, 1, 8), wsb(17, 1, 8), wsb(3, 0, 8), wsb(3, 65536, 8), wsb(3, 1, 0), wsb(3, 1, 2 ** 36 + 1)] == [0] * 6
    # the grid's edges are accepted: stats NULL, affine on the 4-byte grid, N = 1 writes (1, 0)
    assert call(stats=None, affine=aff.ptr + 4) == 0
    assert call(members=ptrs[:1], N=1, stats=None) == 0
    torch.cuda.synchronize()
    got = np.frombuffer(aff.dev.cpu().numpy()[aff.lo:aff.lo + B * 8].tobytes(), dtype=np.float32)
    assert got.tolist() == [1.0, 0.0] * B


# ----------------------------------------------------------------------------------------------- the reduce behind an affine
def _run_reduce(pkg, gpu, name, mode, mem, aff, want, offs, aoff, affine=True):
    """members at offs[:N], dst at offs[N], spread at offs[N + 1]; without the spread, then with it; every launch twice."""
    lib = pkg.native.load_library()
    N, B, n = mem.shape
    want_r, want_sp = want
    for spread in (False, True):
        members = [_Buf(gpu, B * n, offs[k], mem[k]) for k in range(N)]
        dst, sp, ab = _Buf(gpu, B * n, offs[N]), _Buf(gpu, B * n, offs[N + 1]), _Buf(gpu, N * B * 8, aoff, aff)
        for run in range(2):
            rc = lib.drn_ensemble_reduce_affine_u8(_table(members), N, ab.ptr if affine else None, B, n, dst.ptr,
                                                   sp.ptr if spread else None, MODE[mode], _stream())
            assert rc == 0, (name, rc)
            torch.cuda.synchronize()
            tag = (name, "spread" if spread else "plain", "run", run)
            dst.check(want_r, tag)
            sp.check(want_sp if spread else None, tag)
            ab.check(None, tag)
            for m in members:
                m.check(None, tag)
            dst.poison()


def _reduce_variants(idx, N):
    yield [0] * (N + 2), 0
    yield [(idx + k) % 4 for k in range(N)] + [(idx + 1) % 4, (idx + 2) % 4 or 3], 4 * (1 + idx % 3)


REDUCE_GROUPS = ("members", "size", "clamps", "fma")


@pytest.fixture(scope="module")
def reduce_grid():
    return [(name, mode, mem, aff, A.reduce_affine_ref(mem, aff, mode, True)) for name, mode, mem, aff in A.reduce_cases(big=False)]


@pytest.mark.parametrize("group", REDUCE_GROUPS)
def test_affine_reduce_is_the_reference_on_the_grid(pkg, gpu, reduce_grid, group):
    ran = 0
    for idx, (name, mode, mem, aff, want) in enumerate(reduce_grid):
        if name.split(".")[0] != group:
            continue
        for offs, aoff in _reduce_variants(idx, mem.shape[0]):
            _run_reduce(pkg, gpu, name, mode, mem, aff, want, offs, aoff)
        ran += 1
    assert ran == {"members": 32, "size": 6 * len(A.REDUCE_SIZES), "clamps": 2, "fma": len(A.FMA_TRIPLES)}[group]


@pytest.mark.parametrize("which", ("sweep.median", "sweep.mean.ragged"))
def test_affine_reduce_is_the_reference_past_one_sweep_of_the_capped_grid(pkg, gpu, which):
    (name, mode, mem, aff), = [c for c in A.reduce_big_cases() if c[0] == which]
    want = A.reduce_affine_ref(mem, aff, mode, True)
    N, B, n = mem.shape
    ragged = which.endswith(".ragged")
    assert n // (1 if ragged else 16) > A.SWEEP_LANES
    offs = [1 + k % 3 for k in range(N)] + [2, 3] if ragged else [0] * (N + 2)
    _run_reduce(pkg, gpu, name, mode, mem, aff, want, offs, 4 if ragged else 0)


def test_null_and_identity_affines_are_the_reduce_without_one(pkg, gpu, reduce_grid):
    lib = pkg.native.load_library()
    picked = [c for c in reduce_grid if c[0] in ("members.n1.median", "members.n5.median", "members.n8.mean", "members.n16.median",
                                                 "size.51.b3.median", "size.48.b2.mean", "size.17.b3.mean", "clamps.mean")]
    assert len(picked) == 8
    for idx, (name, mode, mem, aff, _) in enumerate(picked):
        N, B, n = mem.shape
        flat = [mem[k].reshape(-1) for k in range(N)]
        want = R.reduce_ref(flat, mode, True)
        one = np.zeros_like(aff)
        one[..., 0] = 1.0
        for offs, aoff in _reduce_variants(idx, N):
            _run_reduce(pkg, gpu, name + ".identity", mode, mem, one, want, offs, aoff)
            _run_reduce(pkg, gpu, name + ".null", mode, mem, one, want, offs, aoff, affine=False)
        # and the entry itself, on the same bytes
        members = [_Buf(gpu, B * n, 0, flat[k]) for k in range(N)]
        dst, sp = _Buf(gpu, B * n), _Buf(gpu, B * n)
        assert lib.drn_ensemble_reduce_u8(_table(members), N, dst.ptr, sp.ptr, B * n, MODE[mode], _stream()) == 0
        torch.cuda.synchronize()
        dst.check(want[0], name), sp.check(want[1], name)


def test_refusals_of_the_affine_reduce(pkg, gpu):
    lib = pkg.native.load_library()
    N, B, n = 3, 2, 48
    mem = np.arange(N * B * n, dtype=np.uint8).reshape(N, B, n)
    aff = A._affines("refusals", N, B)
    members = [_Buf(gpu, B * n, 0, mem[k]) for k in range(N)]
    dst, sp, ab = _Buf(gpu, B * n), _Buf(gpu, B * n), _Buf(gpu, N * B * 8 + 8, 0, np.concatenate([aff.reshape(-1), [0, 0]]).astype(np.float32))
    ptrs = [m.ptr for m in members]

    def call(members=ptrs, N=N, affine=ab.ptr, B=B, clip_bytes=n, dst=dst.ptr, spread=sp.ptr, mode=0, null_table=False):
        table = None if null_table else (ctypes.c_void_p * max(len(members), 1))(*members)
        return lib.drn_ensemble_reduce_affine_u8(table, N, affine, B, clip_bytes, dst, spread, mode, _stream())
    bad = {"null members": dict(null_table=True), "null member": dict(members=[ptrs[0], None, ptrs[2]]), "null dst": dict(dst=None),
           "N = 0": dict(N=0), "N = 17": dict(members=ptrs[:1] * 17, N=17), "N < 0": dict(N=-1), "mode -1": dict(mode=-1),
           "mode 2": dict(mode=2), "mode 2, no affine": dict(mode=2, affine=None), "mode 3": dict(mode=3), "B = 0": dict(B=0),
           "B < 0": dict(B=-1), "clip_bytes < 0": dict(clip_bytes=-3), "affine off 4": dict(affine=ab.ptr + 2),
           "dst == spread": dict(spread=dst.ptr), "dst is a member": dict(dst=ptrs[1]), "spread is a member": dict(spread=ptrs[2]),
           "null members, no affine": dict(null_table=True, affine=None), "N = 17, no affine": dict(members=ptrs[:1] * 17, N=17, affine=None),
           "dst is a member, no affine": dict(dst=ptrs[1], affine=None)}
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
    assert call(clip_bytes=0) == 0 and call(clip_bytes=0, affine=None, spread=None) == 0
    torch.cuda.synchronize()
    for b in members + [dst, sp, ab]:
        b.check(None, "nothing was launched")
    assert call(affine=ab.ptr + 4, mode=1) == 0                      # the 4-byte grid is enough
    torch.cuda.synchronize()
    shifted = np.concatenate([aff.reshape(-1)[1:], [0]]).astype(np.float32).reshape(N, B, 2)
    r, s = A.reduce_affine_ref(mem, shifted, "mean", True)
    dst.check(r, "mean"), sp.check(s, "mean spread")


# ----------------------------------------------------------------------------------------------- the dispatch
def test_dispatch_of_align_members_and_reduce_members(pkg, gpu):
    E = pkg.ensemble
    mem = A.scene("dispatch", 5, 2, 7 * 33 * 3).reshape(5, 2, 7, 33, 3)
    flat = mem.reshape(5, 2, -1)
    want_a, _ = A.align_ref(flat)
    cpu = [torch.from_numpy(m.copy()) for m in mem]
    dev = [t.to(gpu) for t in cpu]
    dev[1] = torch.from_numpy(np.ascontiguousarray(mem[1].transpose(0, 2, 1, 3))).to(gpu).permute(0, 2, 1, 3)       # not contiguous
    assert not dev[1].is_contiguous()
    for backend in ("auto", "hip", "torch"):
        a = E.align_members(dev, backend=backend)
        assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (5, 2, 2)
        assert np.array_equal(a.cpu().numpy().view(np.uint32), want_a.view(np.uint32)), backend
    a_cpu = E.align_members(cpu)
    assert not a_cpu.is_cuda and np.array_equal(a_cpu.numpy().view(np.uint32), want_a.view(np.uint32))
    with pytest.raises(ValueError, match="GPU"):
        E.align_members(cpu, backend="hip")
    for mode in ("median", "mean"):
        want_r, want_sp = A.reduce_affine_ref(flat, want_a, mode, True)
        for backend in ("auto", "hip", "torch"):
            r, sp = E.reduce_members(dev, mode, spread=True, backend=backend, affine=a)
            assert r.is_cuda and r.shape == sp.shape == (2, 7, 33, 3)
            assert np.array_equal(r.cpu().numpy().reshape(-1), want_r) and np.array_equal(sp.cpu().numpy().reshape(-1), want_sp)
            assert E.reduce_members(dev, mode, backend=backend, affine=a)[1] is None
    with pytest.raises(ValueError, match="affine"):
        E.reduce_members(dev, "median", affine=a_cpu)                 # the affines live where the members live
    with pytest.raises(ValueError, match="normal"):
        E.reduce_members(dev, "normal", affine=a)
    # the native wrappers hand back the moments too
    a2, st = pkg.native.ensemble_align_affine([d.contiguous() for d in dev], stats=True)
    assert torch.equal(a2, a) and np.array_equal(st.cpu().numpy(), A.align_ref(flat)[1])
    # neither kernel path builds a stack: beyond the members, the workspace (Q words per 8192 bytes), the result and the spread
    big = [torch.randint(0, 256, (1, 1 << 20, 3), dtype=torch.uint8, device=gpu) for _ in range(8)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ab = E.align_members(big)
    r, sp = E.reduce_members(big, "median", spread=True, affine=ab)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before <= 2 * big[0].numel() + (1 << 20)
    small = np.stack([b[:, :99].cpu().numpy().reshape(1, -1) for b in big])
    assert np.array_equal(r[:, :99].cpu().numpy().reshape(-1), A.reduce_affine_ref(small, ab.cpu().numpy(), "median")[0])


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
    p.window_align, p.ensemble, p.ensemble_reduce, p.ensemble_align = False, 1, "median", False


def _host(members):
    return [[np.ascontiguousarray(torch.as_tensor(t).cpu().numpy()) for t in m] for m in members]


PATHS = {
    "whole_clip": dict(),
    "windowed": dict(window_frames=9, window_overlap=2),
    "pixel_tiled": dict(tile_height=32, tile_width=32, tile_overlap=8),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_pipeline_with_ensemble_align_is_three_calls_composed_by_hand(pkg, gpu, pipe, path):
    p = pipe
    _reset(p)
    for k, v in PATHS[path].items():
        setattr(p, k, v)
    T = 17 if path == "windowed" else 9
    rgb = pkg.synthetic_weights.synth_tensor(f"ensemble_align.gpu.clip{T}", (1, 3, T, H, W), torch.float32, scale=1.0)
    batch = {"rgb": rgb, "video": rgb, "context_index": torch.tensor([[0], [3]], dtype=torch.long)}
    flags = [False, True]
    p.guidance, seed = 1.5, 5
    members = _host([p.generate_video_passes(batch, flags, seed=seed + k, to_host=False) for k in range(3)])
    p.ensemble = 3
    default = p.generate_video_passes(batch, flags, seed=seed)
    assert p.last_ensemble_align == []
    p.ensemble_align = False
    explicit = p.generate_video_passes(batch, flags, seed=seed)
    assert all(np.array_equal(a, b) for a, b in zip(default, explicit)) and p.last_ensemble_align == []
    for reduce in ("median", "mean"):
        p.ensemble_reduce, p.ensemble_align = reduce, True
        want = A.compose_ref(members, flags, reduce)
        got = p.generate_video_passes(batch, flags, seed=seed)
        (a0, a1), = p.last_ensemble_align
        assert a1 is None and a0.is_cuda and a0.dtype == torch.float32 and tuple(a0.shape) == (3, 1, 2)
        print(f"ensemble_align pipeline {path} {reduce}: affines {a0.cpu().numpy().reshape(3, 2).tolist()}")
        assert np.array_equal(a0.cpu().numpy().view(np.uint32), want[0][2].view(np.uint32)), (path, reduce)
        dev = p.generate_video_passes(batch, flags, seed=seed, to_host=False)
        for g, d, (w, _, _) in zip(got, dev, want):
            assert isinstance(g, np.ndarray) and g.shape == (1, T, H, W, 3) and np.array_equal(g, w), (path, reduce)
            assert d.is_cuda and d.dtype == torch.uint8 and torch.equal(d.cpu(), torch.from_numpy(w)), (path, reduce)
    assert np.array_equal(got[1], default[1])                        # the normal pass is never aligned
    each = [dict(batch, context_index=batch["context_index"][i:i + 1]) for i in range(2)]
    res, spr = p.generate_video_ensemble(each, flags, seed=seed)
    want = A.compose_ref(members, flags, "mean", spread=True)
    for i in range(2):
        assert np.array_equal(res[i], want[i][0]) and np.array_equal(spr[i], want[i][1])
    _reset(p)


def test_pipeline_with_a_restore_plan_restores_once_after_the_aligned_reduce(pkg, gpu, pipe):
    fit = importlib.import_module(pkg.__name__ + ".fit")
    p = pipe
    _reset(p)
    image = pkg.synthetic_weights.synth_tensor("ensemble_align.gpu.img", (1, 7, 60, 56, 3), torch.float32).abs().clamp(max=1.0)
    plan = fit.plan_fit(7, 60, 56, "stretch", H, W)
    clip = fit.fit_frames(image, plan, device=gpu)
    ci = torch.tensor([[0], [3]], dtype=torch.long)
    each = [{"rgb": clip, "video": clip, "context_index": ci[i:i + 1]} for i in range(2)]
    flags = [False, True]
    members = _host([p.generate_video_each(each, flags, seed=9 + k, to_host=False) for k in range(3)])
    rplan = fit.plan_restore(plan)
    p.restore_plan, p.ensemble, p.ensemble_align = rplan, 3, True
    got = p.generate_video_each(each, flags, seed=9)
    dev = p.generate_video_each(each, flags, seed=9, to_host=False)
    assert p.restore_plan is rplan
    want = A.compose_ref(members, flags, "median")
    for i in range(2):
        back = fit.restore_frames(torch.from_numpy(want[i][0]).to(gpu), rplan).cpu().numpy()
        assert got[i].shape == back.shape == (1, 7, 60, 56, 3) and np.array_equal(got[i], back)
        assert dev[i].is_cuda and np.array_equal(dev[i].cpu().numpy(), back)
    assert len(p.last_ensemble_align) == 2 and p.last_ensemble_align[1] == [None]
    assert np.array_equal(p.last_ensemble_align[0][0].cpu().numpy().view(np.uint32), want[0][2].view(np.uint32))
    _reset(p)


def test_nodes_with_ensemble_align_are_the_composition_by_hand(pkg, gpu, pipe):
    p = pipe
    _reset(p)
    sw = pkg.synthetic_weights
    T = 9
    image = sw.synth_tensor("ensemble_align.node.img", (1, T, H, W, 3), torch.float32).abs().clamp(max=1.0)
    env = sw.synth_tensor("ensemble_align.node.env", (1, 32, 64, 3), torch.float32).abs() * 4.0
    inv = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    fwd = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    rel = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    normal_at = 3                                                                 # RETURN_NAMES: base_color, metallic, roughness, normal, depth
    members = [inv.run_inverse_pass(p, image, guidance=1.0, seed=(3 + k)) for k in range(3)]
    u8 = [[(m[i] * 255.0).round().to(torch.uint8).numpy().reshape(1, T, H, W, 3) for i in range(5)] for m in members]
    flags = [i == normal_at for i in range(5)]
    plain = inv.run_inverse_pass(p, image, guidance=1.0, seed=3, ensemble=3)
    assert p.ensemble_align is False
    off = inv.run_inverse_pass(p, image, guidance=1.0, seed=3, ensemble=3, ensemble_align=False)
    assert all(torch.equal(a, b) for a, b in zip(plain, off))
    got = inv.run_inverse_pass(p, image, guidance=1.0, seed=3, ensemble=3, ensemble_reduce="mean", ensemble_align=True)
    assert (p.ensemble, p.ensemble_reduce, p.ensemble_align) == (3, "mean", True) and len(got) == 5
    want = A.compose_ref(u8, flags, "mean")
    for i in range(5):
        assert torch.equal(got[i], torch.from_numpy(want[i][0].reshape(tuple(got[i].shape))).float() / 255.0), i
    # relight: the switch belongs to the inverse stage; the forward stage renders one sample from the aligned, reduced G-buffers
    out = rel.run_relight(p, p, image, env, guidance=1.0, seed=3, env_spin=45.0, ensemble=3, ensemble_reduce="mean", ensemble_align=True)
    assert p.ensemble == 1 and p.ensemble_align is False and p.model_type == "forward"
    for a, b in zip(out[1:], got):
        assert torch.equal(a, b)
    g5 = [o.reshape(1, T, H, W, 3) for o in got]
    (lit,) = fwd.run_forward_pass(p, g5[4], g5[3], g5[2], g5[1], g5[0], env, guidance=0.0, seed=3, env_spin=45.0)
    assert torch.equal(out[0], lit)
    _reset(p)
