"""The exact-data grid of tests/mx_gemm_refs.py must be exact and must bite (no GPU needed).

For EVERY case tests/test_mx_gemm_edges_gpu.py runs: (a) the exactness budget holds - sum |a| |w| stays below 2^24 grid steps, so
any summation order is exact in fp32 and the expected output is fixed to the bit; (b) a plain-torch stand-in that accumulates
in fp32 K step by K step, slice by slice, equals the expected output exactly; (c) every mutant that applies to the case - a
dropped K step, a stage mix-up, a neighbour's scale, a wrong gate row, an omitted rounding, ... - differs from it in at least
MIN_SHARE of the elements it touches, in every row tile it touches (and, under the GELU epilogue, fails the bound the GPU module
asserts there).  The guard helpers find a store one row past M and 8 columns past N in the bf16 and the uint8 windows."""
import pytest
import torch

import dit_refs as R
import mx_gemm_refs as X

BF = torch.bfloat16

_seen = set(X.GRID_K256 + X.GRID_RING)
GELU_OF_OUT_MX = []
for _c in X.GRID_OUT_MX:
    _g = X.as_gelu_case(_c)
    if _g not in _seen:
        _seen.add(_g)
        GELU_OF_OUT_MX.append(_g)
ALL = X.GRID_K256 + X.GRID_RING + GELU_OF_OUT_MX


def _windowed_res(c, res):
    """The residual where the GPU test puts it: a NaN-guarded window with its own row stride."""
    _, win = R.guarded(c.M, c.N, X.leading_dims(c)[1], 2, "cpu")
    win.copy_(res)
    return win


# ------------------------------------------------------------------------------------------------ the grid itself
def test_grid_covers_the_geometry_it_claims():
    k256 = [c for c in X.GRID_K256 if c.M <= 513 and c.K <= 512 and not c.alias]
    assert {c.M for c in k256} == {1, 255, 256, 257, 511, 512, 513} and {c.N for c in k256} == {256, 512}
    assert {c.K for c in k256} == {128, 256, 384, 512}
    for M in (1, 255, 256, 257, 511, 512, 513):
        assert {c.epi for c in k256 if c.M == M} == {0, 1, 2}, M
        assert {c.K for c in k256 if c.M == M} == {128, 256, 384, 512}, M
    assert any(c.K == 4096 and c.M == 257 and c.N == 256 for c in X.GRID_K256)
    assert any(c.alias and c.M % 256 for c in X.GRID_K256) and any(c.M == 513 and X.clips_of(c) == 3 for c in X.GRID_K256)
    two = [c for c in X.GRID_K256 if c.epi == 2 and c.rpb and X.clips_of(c) == 2 and c.M <= 513]
    assert all(c.rpb == (c.M + 1) // 2 for c in two if not c.alias) and {c.M for c in two} >= {255, 256, 257, 511, 512, 513}
    assert any(c.rpb % 256 for c in two), "a boundary inside a row tile"
    # the tile map: 10 x 3 workgroups, not a multiple of 8, a full band of 8 tile rows and a ragged band of 2
    big = [c for c in X.GRID_K256 if c.M == 2305]
    assert big and all(c.N == 768 and c.K == 128 for c in big)
    tiles_m, tiles_n = -(-2305 // 256), 768 // 256
    assert (tiles_m, tiles_n) == (10, 3) and (tiles_m * tiles_n) % 8 and tiles_m % 8 == 2 and 2305 % 256 == 1
    # the ring kernels: 1 .. 5 K steps per slice - fewer than, equal to and more than the stages of either ring
    for shape in (0, 1):
        ring = [c for c in X.GRID_RING if c.shape == shape]
        assert {c.K // 128 // c.splits for c in ring} == {1, 2, 3, 4, 5}
        st = X.RING_STAGES[shape]
        per = {c.K // 128 // c.splits for c in ring}
        assert min(per) < st - 1 and st - 1 in per and st in per and max(per) > st
        assert {(c.K, c.splits) for c in ring} == set(X.RING_KS) and {(c.M, c.rpb) for c in ring} == set(X.RING_MS)
        for ks in X.RING_KS:
            sub = [c for c in ring if (c.K, c.splits) == ks]
            assert {(c.M, c.rpb, c.N, c.epi) for c in sub} == {(M, rpb, N, e) for M, rpb in X.RING_MS for N in (256, 512) for e in (0, 1, 2)}
        assert any(c.alias for c in ring) and any(c.strided for c in ring) and any(not c.strided for c in ring)
    assert {(c.shape, c.K, c.splits) for c in X.GRID_SLICES} == {(s, K, n) for s in (0, 1) for K, n in X.RING_KS if n > 1}
    assert len(set(ALL)) == len(ALL)


def test_shift_brings_the_product_near_one():
    for K in (128, 256, 384, 512, 640, 1280, 4096):
        c = X._case("k256", -1, 257, 256, K, 0, False)
        s = X.operands(c).exact.std().item()
        print(f"mx-gemm-edge data K={K}: shift {X.shift_of(K)}, std of the product {s:.3f}")
        assert 0.5 < s < 1.25, (K, s)         # a power-of-two shift lands within sqrt(2) of the target


# ------------------------------------------------------------------------------------------------ every case
def _prove(c):
    ops = X.operands(c)
    budget = X.exactness_budget(ops)
    assert budget < 2.0 ** 24, (X.case_id(c), budget)
    assert torch.equal(ops.exact.float().double(), ops.exact), "the product is exact in fp32"
    gate = res = None
    if c.epi == R.EPI_GATE_RES:
        gate, res = X.gate_res(c)
        res = _windowed_res(c, res)
    want = X.expected(c, ops, gate, res)
    out = X.standin(c, gate, res)
    assert torch.equal(out, want), f"{int((out != want).sum())} elements of the unmutated stand-in differ"
    if c.splits > 1:
        assert torch.equal(X.standin_slices(c), X.expected_slices(c, ops))
    lin = ops.exact.to(BF)
    if c.epi == R.EPI_GELU:
        ok, msg = X.gelu_check(want, lin)
        assert ok, msg
    caught = []
    for m in X.MUTANTS:
        hit = X.mutant_rows(c, m, ops)
        if hit is None:
            continue
        bad = X.standin(c, gate, res, m)
        shares = X.mutant_shares(c, bad, want, hit)
        assert shares and min(shares) >= X.MIN_SHARE, (X.case_id(c), m, shares)
        if c.epi == R.EPI_GELU:
            ok, msg = X.gelu_check(bad, lin)
            assert not ok, (X.case_id(c), m, "passes the GELU bound", msg)
        caught.append(f"{m} {min(shares):.2f}")
    return budget, caught


@pytest.mark.parametrize("c", ALL, ids=X.case_id)
def test_case_is_exact_and_its_mutants_are_caught(c):
    budget, caught = _prove(c)
    print(f"mx-gemm-edge proof {X.case_id(c)}: budget 2^{torch.tensor(budget).log2().item():.1f}, stand-in bit-equal, "
          f"least share per mutant: {', '.join(caught)}")
    assert caught


@pytest.mark.parametrize("mutant", X.MUTANTS)
def test_every_mutant_applies_on_both_kernels(mutant):
    for grid, name in ((X.GRID_K256, "k256"), (X.GRID_RING, "ring")):
        n = sum(X.mutant_rows(c, mutant) is not None for c in grid)
        print(f"mx-gemm-edge mutant {mutant}: applies to {n} of {len(grid)} {name} cases")
        # (the ring kernels take whole 256-row clips only: no ragged tile there)
        assert n > 0 or (mutant, name) == ("ragged_last_row", "ring"), (mutant, name)


@pytest.mark.parametrize("c", X.GRID_SLICES, ids=X.slice_id)
def test_slices_are_exact_and_their_mutants_are_caught(c):
    """fp32 slices of drn_gemm_mxfp8_splitk_partials: slice s of the stand-in is the exact product of its own K range; an
    accumulator mutant shows in at least one slice."""
    ops = X.operands(c)
    assert X.exactness_budget(ops) < 2.0 ** 24
    want = X.expected_slices(c, ops)
    assert torch.equal(X.standin_slices(c), want) and torch.equal(want.double().sum(0), ops.exact)
    T = 128 if c.shape == 1 else 256
    for m in X.ACC_MUTANTS:
        hit = X.mutant_rows(X.MxCase("ring", c.shape, c.M, c.N, c.K, 0, False, False, c.rpb, c.splits, c.seed), m, ops)
        if hit is None:
            continue
        bad = X.standin_slices(c, m)
        best = 0.0
        for s in range(c.splits):
            diff = bad[s] != want[s]
            shares = [diff[t:t + T][hit[t:t + T]].float().mean().item() for t in range(0, c.M, T) if bool(hit[t:t + T].any())]
            best = max(best, min(shares))
        assert best >= X.MIN_SHARE, (X.slice_id(c), m, best)


def test_expected_outputs_are_the_bf16_gemm_reference():
    """The operands are exact in bf16 too, so dit_refs.gemm_ref (the reference of the bf16 kernels' tests: fp64 product, bf16 torch
    ops per epilogue) must give the same bits as the fp32 restatement of the rounding points here."""
    for c in X.GRID_K256:
        if c.M > 513 or c.K > 512:
            continue
        ops = X.operands(c)
        gate, res = X.gate_res(c) if c.epi == R.EPI_GATE_RES else (None, None)
        a, w = ops.da.to(BF), ops.dw.to(BF)
        assert torch.equal(a.double(), ops.da) and torch.equal(w.double(), ops.dw)
        ref, _ = R.gemm_ref(a, w, c.epi, gate, res, c.rpb)
        assert torch.equal(ref, X.expected(c, ops, gate, res)), X.case_id(c)


# ------------------------------------------------------------------------------------------------ guard windows
@pytest.mark.parametrize("mutant", ["row_past_M", "cols_past_N"])
def test_store_outside_the_window_is_caught(mutant):
    wins = [R.guarded(257, 256, 320, 2, "cpu"), R.guarded(1, 512, 512, 2, "cpu"), R.guarded(256, 256, 256, 2, "cpu")]
    wins += list(X.out_mx_windows(257, 256, "cpu")) + list(X.out_mx_windows(1, 512, "cpu"))
    for buf, v in wins:
        assert bool(R.is_sentinel(buf).all())
        v.copy_(torch.zeros(v.shape, dtype=v.dtype))
        R.assert_guard_intact(buf, v)
        assert not bool(R.is_sentinel(v).any())
        X.store_past(buf, v, mutant)
        assert not bool(v.bool().any()), "the window itself is untouched: only the guard can see this"
        with pytest.raises(AssertionError, match="outside the window"):
            R.assert_guard_intact(buf, v)
    (qb, qv), (sb, sv) = X.out_mx_windows(513, 512, "cpu")
    assert qv.is_contiguous() and sv.is_contiguous() and qv.shape == (513, 512) and sv.shape == (513, 16)
    assert qv.storage_offset() % 4 == 0 and sv.storage_offset() % 4 == 0
