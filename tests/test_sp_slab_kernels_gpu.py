"""The kernels of the sequence-parallel exchange at plane, tile and clip edges: drn_gemm_bf16_blocked (the bf16 slab GEMM of the
"slabs" route) through the C entry at every case of dit_refs.GRID_GEMM_BLOCKED - for which tests/test_sp_slab_refs_cpu.py has shown
a correct stand-in to pass and seven wrong plane addressings to fail - and drn_permute_021 (the "regroup" route, and the byte-pair
regroup of the e4m3 return).

Every GEMM case: operands and outputs live in sentinel-filled guard windows (padded planes: row padding and the gaps between
planes too) that must be intact afterwards; the result must be finite; the launch is made twice into fresh windows and both results
must be bit-equal; the result regrouped with from_planes must pass dit_refs.GEMM_BOUND against the fp64 gemm_ref; under a forced
tile it must also equal drn_gemm_bf16 on the same logical data bit for bit.  Every force hook is restored in a `finally`.
`-s` prints one `sp-slab-edge` line of figures per case."""
import pytest
import torch

import dit_refs as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EINVAL = -1


def _finite(t):
    return bool(torch.isfinite(t.float()).all())


def _blocked_call(pkg, c, aw, wd, cw, gate, rw, prefetch=1):
    """drn_gemm_bf16_blocked on the windows of case c under its forced tile; the hooks are back at their defaults afterwards."""
    N_ = pkg.native
    lib = N_.load_library()
    g = R.blocked_geometry(c)
    lib.drn_gemm_force_tile(c.tile if c.tile > 0 else -1)
    lib.drn_gemm_force_res_prefetch(prefetch)
    try:
        rc = lib.drn_gemm_bf16_blocked(aw.data_ptr(), wd.data_ptr(), cw.data_ptr(), c.M, c.N, c.K, g["lda"], wd.stride(0), g["ldc"],
                                       c.epi, N_._ptr(gate), N_._ptr(rw), g["ldr"] if rw is not None else 0, c.rpb,
                                       c.abc, g["a_stride"], c.cbc, g["c_stride"], N_._stream())
        torch.cuda.synchronize()
    finally:
        lib.drn_gemm_force_tile(-1)
        lib.drn_gemm_force_res_prefetch(1)
    return rc


def _launch(pkg, gpu, c, a, wd, gate_d, res, prefetch=1):
    """One launch of case c into fresh windows, checked for what a launch may touch.  Returns the logical [M, N] result (GPU)."""
    wins = R.blocked_windows(c, a, res, gpu)
    aw, cw = wins["a"][1], wins["c"][1]
    rw = None
    if c.epi == R.EPI_GATE_RES:
        rw = cw[0] if c.alias else wins["r"][1][0]
    a_before = aw.clone()
    assert _blocked_call(pkg, c, aw, wd, cw, gate_d if c.epi == R.EPI_GATE_RES else None, rw, prefetch) == 0
    for key in ("a", "c", "r"):
        if wins[key] is not None:
            R.assert_guard_intact(*wins[key])
    assert torch.equal(aw, a_before), "A is an input: not written"
    if rw is not None and not c.alias:
        assert torch.equal(rw, res.to(gpu)), "the residual is an input: not written"
    return R.from_planes(cw)


def _plain(pkg, gpu, c, a, wd, gate_d, res):
    """drn_gemm_bf16 on the same logical data (contiguous) under the same forced tile."""
    N_ = pkg.native
    lib = N_.load_library()
    ad, out = a.to(gpu), torch.empty((c.M, c.N), dtype=BF, device=gpu)
    gate = rd = None
    if c.epi == R.EPI_GATE_RES:
        gate = gate_d
        if c.alias:
            out.copy_(res)
            rd = out
        else:
            rd = res.to(gpu)
    lib.drn_gemm_force_tile(c.tile)
    try:
        rc = lib.drn_gemm_bf16(ad.data_ptr(), wd.data_ptr(), out.data_ptr(), c.M, c.N, c.K, c.K, wd.stride(0), c.N, c.epi,
                               N_._ptr(gate), N_._ptr(rd), c.N if rd is not None else 0, c.rpb, N_._stream())
        torch.cuda.synchronize()
    finally:
        lib.drn_gemm_force_tile(-1)
    assert rc == 0
    return out


@pytest.mark.parametrize("c", R.GRID_GEMM_BLOCKED, ids=R.blocked_id)
def test_gemm_blocked_edges(pkg, gpu, c):
    a, w, gate, res, ref, mag = R.blocked_inputs_ref(c)
    wd, gate_d = w.to(gpu), gate.to(gpu)
    if c.tile < 0:
        assert pkg.native.gemm_blocked_ok(c.M, c.N), "the route takes the slab GEMM only where this holds"
    out = _launch(pkg, gpu, c, a, wd, gate_d, res)
    again = _launch(pkg, gpu, c, a, wd, gate_d, res)
    assert _finite(out), "a sentinel of the row padding / a plane gap reached the result, or an element was never written"
    assert torch.equal(out, again), "two launches of the same case differ"
    o = out.cpu()
    print(f"sp-slab-edge gemm {R.blocked_id(c)}: {R.figures(o, ref, mag)}")
    ok, msg = R.ulp_diff_ok(o, ref, mag=mag, **R.GEMM_BOUND[c.epi])
    assert ok, msg
    if c.tile > 0:
        assert torch.equal(out, _plain(pkg, gpu, c, a, wd, gate_d, res)), "differs from drn_gemm_bf16 on the same logical data"
    if c.pre:
        off = _launch(pkg, gpu, c, a, wd, gate_d, res, prefetch=0)
        assert torch.equal(out, off), "the residual-prefetch variant and the plain epilogue differ"


@pytest.mark.parametrize("tile", [1, 2])
def test_gemm_blocked_lane_map_exact_integers(pkg, gpu, tile):
    """Small integers and an identity operand: the product IS the other operand, so one misplaced lane, column or plane shows as a
    wrong integer.  A planes of 64 / 128 / 256 columns against an identity W; C planes of 256 / 512 columns from an identity A."""
    M, X = R.GEMM_TILE_ROWS[tile] + 1, 1024
    m, x = torch.arange(M).view(M, 1), torch.arange(X).view(1, X)
    ints = ((m * 131 + x * 7) % 251 - 125).to(BF)                     # [M, 1024], |v| <= 125: exact in bf16
    eye = torch.eye(X, dtype=BF)
    for abc in (64, 128, 256):
        c = R.BlockedCase(tile, M, X, X, R.EPI_NONE, "a", abc, 0, True, False, M, False, 0)
        for _ in (0, 1):
            got = _launch(pkg, gpu, c, ints, eye.to(gpu), None, None).cpu()
            bad = (got != ints).nonzero()
            assert bad.numel() == 0, f"A planes of {abc}: {bad.shape[0]} of {M * X} differ; first (m, n): {bad[:8].tolist()}"
    n = torch.arange(X).view(X, 1)
    w = ((n * 131 + x * 7) % 251 - 125).to(BF)                        # [N, K], not symmetric
    assert not torch.equal(w, w.t())
    want = w.t()[:M].contiguous()                                     # C[m][n] = sum_k eye[m][k] W[n][k] = W[n][m]
    for cbc in (256, 512):
        c = R.BlockedCase(tile, M, X, X, R.EPI_NONE, "c", 0, cbc, True, False, M, False, 0)
        wins = R.blocked_windows(c, eye[:M], None, gpu)
        assert _blocked_call(pkg, c, wins["a"][1], w.to(gpu), wins["c"][1], None, None) == 0
        R.assert_guard_intact(*wins["c"])
        assert torch.equal(wins["c"][1].cpu(), R.planes_of(want, cbc)), f"C planes of {cbc} columns"
    print(f"sp-slab-edge lane-map tile{tile} M{M}: A planes 64 / 128 / 256 and C planes 256 / 512 bit-exact")


def test_gemm_blocked_refusals_write_nothing(pkg, gpu):
    """Every DRN_CHECK_ARG of the entry, every shape that would take the 128 x 128 kernel (it has no plane layouts) and the gated
    call with several clips at such a shape: DRN_EINVAL, and C with its guards still holds the sentinel.  native.gemm_blocked_ok
    says exactly where an automatic blocked launch is accepted."""
    N_ = pkg.native
    lib = N_.load_library()
    a = R.rnd((1 << 22,), seed=1).to(gpu)
    w = R.rnd((8192, 192), 0.1, seed=2).to(gpu)
    gate, res = R.rnd((2, 8192), seed=3).to(gpu), R.rnd((2304, 4096), seed=4).to(gpu)
    cbuf, cwin = R.guarded(2304, 4096, 4096, 2, gpu)

    def call(M=512, N=512, K=128, lda=64, ldc=256, epi=0, rpb=None, abc=64, a_str=None, cbc=256, c_str=None, tile=1, C=None, ldr=0):
        lib.drn_gemm_force_tile(tile)
        try:
            rc = lib.drn_gemm_bf16_blocked(a.data_ptr(), w.data_ptr(), C if C is not None else cwin.data_ptr(), M, N, K, lda, 192, ldc,
                                           epi, gate.data_ptr() if epi == 2 else None, res.data_ptr() if epi == 2 else None, ldr,
                                           rpb or M, abc, M * lda if a_str is None else a_str, cbc, M * ldc if c_str is None else c_str,
                                           N_._stream())
            torch.cuda.synchronize()
        finally:
            lib.drn_gemm_force_tile(-1)
        return rc

    refused = {
        "A width not a power of two": call(K=192, abc=96, lda=96),
        "C width not a power of two": call(N=768, cbc=384, ldc=384),
        "A width below 64": call(abc=32, lda=32),
        "C width below 256": call(cbc=128, ldc=128),
        "K not a multiple of the A width": call(K=192, abc=128, lda=128),
        "N not a multiple of the C width": call(N=768, cbc=512, ldc=512),
        "A plane stride not a multiple of 8": call(a_str=512 * 64 + 4),
        "C plane stride not a multiple of 8": call(c_str=512 * 256 + 4),
        "lda below the A width": call(lda=56, a_str=512 * 64),
        "ldc below the C width": call(ldc=248, c_str=512 * 256),
        "M = 64 (128 x 128 kernel)": call(M=64, N=4096, tile=-1),
        "N = 384 (128 x 128 kernel)": call(M=2304, N=384, cbc=0, ldc=384, c_str=0, tile=-1),
        "forced tile 0, A planes": call(M=2304, N=4096, tile=0),
        "forced tile 0, C planes only": call(M=2304, N=4096, abc=0, lda=128, a_str=0, tile=0),
        # the plan's branch for several clips under one launch must refuse like the plan of one clip does
        "gated, two clips, 128 x 128 shape": call(M=300, N=256, epi=2, rpb=150, cbc=0, ldc=256, c_str=0, tile=-1, ldr=4096),
        "gated, ragged clips, 128 x 128 shape": call(M=301, N=256, epi=2, rpb=151, cbc=0, ldc=256, c_str=0, tile=-1, ldr=4096),
        "gated, two clips, forced tile 0": call(M=300, N=512, epi=2, rpb=150, tile=0, ldr=4096),
    }
    assert lib.drn_gemm_tile_choice(300, 256) == 0 and lib.drn_gemm_tile_choice(64, 4096) == 0 and lib.drn_gemm_tile_choice(2304, 384) == 0
    wrong = {k: v for k, v in refused.items() if v != EINVAL}
    assert not wrong, f"accepted (return code): {wrong}"
    assert bool(R.is_sentinel(cbuf).all()), "a refused call wrote to C or its guards"
    assert call() == 0 and call(M=300, N=512, epi=2, rpb=150, ldr=4096) == 0, "the same calls inside the contract run"
    # gemm_blocked_ok <=> an automatic blocked launch with rows_per_batch = M is accepted
    big = torch.empty(9216 * 8192, dtype=BF, device=gpu)
    for M in (64, 256, 1152, 2304, 4608, 9216):
        for N in (256, 384, 4096, 8192):
            big.view(torch.int16).fill_(R.SENTINEL)
            rc = call(M=M, N=N, K=64, cbc=0, ldc=N, c_str=0, tile=-1, C=big.data_ptr())
            assert rc in (0, EINVAL) and (rc == 0) == N_.gemm_blocked_ok(M, N), (M, N, rc)
            assert rc == 0 or bool(R.is_sentinel(big).all()), (M, N)
    print(f"sp-slab-edge refusals: {len(refused)} calls refused, nothing written; gemm_blocked_ok agrees at 24 shapes")


# the last shape has more 16-byte chunks than the launch has threads (at most 4096 blocks of 256): the grid-stride loop's second trip
PERMUTE_SHAPES = [(1, 1, 8), (3, 1, 8), (1, 5, 16), (7, 8, 512), (8, 300, 4096)]
assert 8 * 300 * (4096 // 8) > 4096 * 256


@pytest.mark.parametrize("shape", PERMUTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_permute_021_edges(pkg, gpu, shape):
    A, B, C = shape
    lib = pkg.native.load_library()
    n = A * B * C
    x = torch.arange(n, dtype=torch.int32).mul_(40503).to(torch.int16).view(A, B, C).to(gpu)     # every element its own bits
    want = x.permute(1, 0, 2).contiguous()
    outs = []
    for _ in (0, 1):
        buf, win = R.guarded(1, n, n, 1, gpu)
        assert lib.drn_permute_021(x.data_ptr(), win.data_ptr(), A, B, C, pkg.native._stream()) == 0
        torch.cuda.synchronize()
        R.assert_guard_intact(buf, win)
        outs.append(win.view(torch.int16).view(B, A, C))
    assert torch.equal(outs[0], want) and torch.equal(outs[0], outs[1])
    print(f"sp-slab-edge permute_021 {A}x{B}x{C}: bit-exact")


@pytest.mark.parametrize("C", [16, 128])
def test_permute_021_byte_pairs(pkg, gpu, C):
    """HipDiT._regroup_bytes: e4m3 rows (128 bytes here) and their scale rows (16 bytes) regrouped as bf16 pairs."""
    world, rows = 8, 37
    g = torch.Generator().manual_seed(C)
    src = torch.randint(0, 256, (world, rows, C), generator=g, dtype=torch.uint8).to(gpu)
    outs = []
    for _ in (0, 1):
        buf, win = R.guarded(1, src.numel(), src.numel(), 1, gpu, dtype=torch.uint8)
        pkg.dit_engine.HipDiT._regroup_bytes(src, win.view(rows, world, C))
        torch.cuda.synchronize()
        R.assert_guard_intact(buf, win)
        outs.append(win.view(rows, world, C))
    assert torch.equal(outs[0], src.permute(1, 0, 2)) and torch.equal(outs[0], outs[1])
    print(f"sp-slab-edge permute_021 bytes {world}x{rows}x{C}: bit-exact")


def test_permute_021_refusals_write_nothing(pkg, gpu):
    lib = pkg.native.load_library()
    st = pkg.native._stream()
    x = R.rnd((3, 5, 24), seed=1).to(gpu)
    buf, win = R.guarded(1, x.numel() + 8, x.numel() + 8, 1, gpu)
    before = x.clone()
    assert lib.drn_permute_021(x.data_ptr(), x.data_ptr(), 3, 5, 24, st) == EINVAL                 # in place
    assert lib.drn_permute_021(x.data_ptr(), win.data_ptr(), 3, 10, 12, st) == EINVAL               # C % 8 != 0
    assert lib.drn_permute_021(x.data_ptr(), win.data_ptr() + 8, 3, 5, 24, st) == EINVAL            # y not 16-byte aligned
    assert lib.drn_permute_021(x.data_ptr() + 8, win.data_ptr(), 3, 5, 16, st) == EINVAL            # x not 16-byte aligned
    torch.cuda.synchronize()
    assert bool(R.is_sentinel(buf).all()) and torch.equal(x, before)
    assert lib.drn_permute_021(x.data_ptr(), win.data_ptr(), 3, 5, 24, st) == 0
    torch.cuda.synchronize()


def test_force_hooks_are_back_at_their_defaults(pkg, gpu):
    """The last test of the file (pytest keeps file order): no case above leaves a process-wide override behind."""
    lib = pkg.native.load_library()
    assert lib.drn_gemm_force_res_prefetch(-1) == 1
    assert lib.drn_gemm_tile_choice(18432, 16384) == 1 and lib.drn_gemm_tile_choice(2304, 4096) == 2 and \
        lib.drn_gemm_tile_choice(64, 4096) == 0, "a forced tile was left behind"
