"""The grid of tests/test_sp_slab_kernels_gpu.py (dit_refs.GRID_GEMM_BLOCKED) must pass a correct slab GEMM and must bite (no GPU
needed): at EVERY case a bf16 stand-in that reads and writes through the plane addressing of include/drn.h passes what the GPU
test applies (guards and plane gaps intact, result finite, dit_refs.GEMM_BOUND against the fp64 gemm_ref, the residual window
unchanged), and each of seven subtly wrong addressings fails it at the cases named in KILLED_BY."""
import pytest
import torch

import dit_refs as R

BF = torch.bfloat16
SMALL = [c for c in R.GRID_GEMM_BLOCKED if c.M * c.N <= 1 << 20]
BY_ID = {R.blocked_id(c): c for c in R.GRID_GEMM_BLOCKED}


def test_planes_round_trip_and_placement():
    t = R.rnd((5, 512), seed=1)
    p = R.planes_of(t, 128)
    assert p.shape == (4, 5, 128) and torch.equal(p[2], t[:, 256:384]) and torch.equal(R.from_planes(p), t)
    assert torch.equal(R.planes_of(t, 512)[0], t)
    buf, win = R.place_planes(4, 5, 128, 192, 128, "cpu", p)
    assert win.stride() == (5 * 192 + 128, 192, 1) and win.storage_offset() == 2 * 192 and torch.equal(R.from_planes(win), t)
    R.assert_guard_intact(buf, win)
    assert int(R.is_sentinel(buf).sum()) == buf.numel() - t.numel(), "row padding, plane gaps and guard rows hold the sentinel"
    buf[2 * 192 + 5 * 192 + 3] = 0                      # inside the gap between planes 0 and 1
    with pytest.raises(AssertionError, match="outside the window"):
        R.assert_guard_intact(buf, win)
    buf1, win1 = R.place_planes(1, 3, 64, 64, 0, "cpu")
    assert win1.shape == (1, 3, 64) and win1.is_contiguous()


def test_grid_holds_what_it_is_meant_to():
    G = R.GRID_GEMM_BLOCKED
    assert len(set(map(R.blocked_id, G))) == len(G)
    for tile, h in ((1, 256), (2, 144)):
        f = [c for c in G if c.tile == tile]
        for M in (h - 1, h, h + 1, 2 * h + 1):
            assert {(c.epi, c.layout) for c in f if c.M == M} >= {(e, l) for e in (0, 1, 2) for l in ("a", "c", "ac")}, (tile, M)
        assert {(c.K, c.abc) for c in f if c.abc} >= {(64, 64), (128, 64), (128, 128), (192, 64), (4096, 64), (4096, 128), (4096, 2048)}
        assert {(c.N, c.cbc) for c in f if c.cbc} == {(512, 256), (1024, 256), (1024, 512)}
        assert {c.padded for c in f} == {True, False}
        assert any(c.alias and c.layout == "a" for c in f) and any(c.epi == 2 and c.layout == "c" and not c.alias for c in f)
        assert {c.M for c in f if c.rpb == (c.M + 1) // 2} == {h + 1, 2 * h + 1}
    pre = [c for c in G if c.pre]
    assert pre and all(c.tile == 1 and c.M == 512 and c.K == 4096 and c.rpb % 256 == 0 and c.epi == 2 for c in pre)
    auto = [c for c in G if c.tile < 0]
    assert {(c.M, c.N, c.N // c.cbc) for c in auto if c.layout == "c"} == \
        {(M, N, P) for M in (2304, 4608, 9216) for N in (4096, 8192) for P in (8, 4, 2)}
    assert all(c.K == 128 for c in auto if c.layout != "a" or c.N != 4096)
    assert any(c.layout == "a" and c.N == 4096 and c.K == 1024 and c.abc == 128 for c in auto)
    for c in G:                                        # every case is inside the entry's contract
        assert c.abc == 0 or (c.abc >= 64 and c.abc & (c.abc - 1) == 0 and c.K % c.abc == 0)
        assert c.cbc == 0 or (c.cbc >= 256 and c.cbc & (c.cbc - 1) == 0 and c.N % c.cbc == 0)
        assert R.gemm_plan_rows(c.M, c.N)[1] != 0 or c.tile > 0, "an automatic case must not take the 128 x 128 kernel"


def test_plan_model_is_the_librarys_and_finds_the_tail_split(pkg):
    """gemm_cost_model against drn_gemm_tile_choice (host only, nothing is launched); the shapes below M = 20000 whose blocked plan
    splits a tail: the band shape 9216 x 8192 and, smallest of all, 4817 x 8192 - both in the grid."""
    lib = pkg.native.load_library()
    for N in (256, 384, 512, 1024, 2048, 4096, 8192, 12288, 16384):
        for M in list(range(1, 20000, 61)) + [64, 144, 255, 256, 1152, 2304, 4608, 4817, 9216, 9472, 9777, 18432]:
            assert R.gemm_cost_model(M, N)[0] == lib.drn_gemm_tile_choice(M, N), (M, N)
    assert R.gemm_plan_rows(9216, 8192) == (8192, 1) and R.gemm_cost_model(1024, 8192)[0] == 2
    assert R.gemm_plan_rows(4817, 8192) == (4096, 1) and R.gemm_cost_model(721, 8192)[0] == 2
    assert all(R.gemm_plan_rows(M, N)[0] == M for N in (4096, 8192) for M in range(1, 4817)), "4817 x 8192 is the smallest"
    assert R.gemm_plan_rows(9472, 4096, blocked=False) == (8192, 1) and R.gemm_plan_rows(9472, 4096) == (9472, 1), \
        "a tail that would take the 128 x 128 kernel is not split off a blocked launch"
    ids = set(BY_ID)
    assert any(i.startswith("auto-M9216-N8192") for i in ids) and any(i.startswith("auto-M4817-N8192") for i in ids)


def _run(c, mutant=None):
    """The GPU test's checks on the stand-in -> None when all pass, else which one failed first."""
    a, w, gate, res, ref, mag = R.blocked_inputs_ref(c)
    wins = R.blocked_windows(c, a, res, "cpu")
    out = R.gemm_blocked_standin(c, wins, w, gate, mutant, slices=2 + c.seed % 5)
    try:
        for key in ("a", "c", "r"):
            if wins[key] is not None:
                R.assert_guard_intact(*wins[key])
    except AssertionError:
        return "guard"
    if not bool(torch.isfinite(out.float()).all()):
        return "not finite"
    if wins["r"] is not None and not torch.equal(wins["r"][1][0], res):
        return "residual written"
    ok, msg = R.ulp_diff_ok(out, ref, mag=mag, **R.GEMM_BOUND[c.epi])
    return None if ok else f"bound ({msg})"


@pytest.mark.parametrize("c", R.GRID_GEMM_BLOCKED, ids=R.blocked_id)
def test_blocked_standin_passes(c):
    why = _run(c)
    assert why is None, why


# mutant -> cases that must catch it (each named case is checked; the test prints every case that does).  Where a mutant touches
# memory outside the window the guard or the sentinel finds it: "guard" = assert_guard_intact, "not finite" = a sentinel was read
# or an element of the window was never written.
KILLED_BY = {
    # padded planes: plane p is read 128 p elements early, out of the gap / the row padding (contiguous planes cannot tell)
    "a_plane_stride_ignored": ["tile1-M255-N1024-K4096-epi2-a-a128-c0-pad-alias", "tile2-M289-N512-K192-epi2-a-a64-c0-pad-alias"],
    # padded: the sentinel of the row padding is read; contiguous: the next row's values, and the guard rows' sentinel at the end
    "a_koff_no_wrap": ["tile1-M513-N512-K192-epi2-a-a64-c0-pad-alias", "tile2-M144-N512-K128-epi1-a-a64-c0-contig"],
    # every K step from plane 0: wrong values wherever A has two planes or more
    "a_plane_of_tile": ["tile1-M257-N512-K128-epi2-a-a64-c0-pad-alias-rpb129", "tile2-M289-N1024-K192-epi2-ac-a64-c512-pad-rpb145"],
    # the second column tile lands in plane 0: plane 1 keeps its sentinel (N / 2-wide planes: wrong from the third tile on)
    "c_plane_neighbour": ["tile1-M513-N1024-K128-epi2-c-a0-c256-pad", "tile2-M145-N1024-K192-epi2-ac-a64-c512-contig-rpb73"],
    # rows at stride N run into the row padding, the gap and the next plane
    "c_ld_plain": ["tile1-M513-N1024-K128-epi2-c-a0-c256-pad", "tile2-M289-N1024-K128-epi2-c-a0-c256-pad"],
    # only a shape whose plan splits a tail can tell: rows past the first 4096 of planes >= 1
    "tail_rows_plane0": ["auto-M4817-N8192-K128-epi0-ac-a64-c1024-pad", "auto-M4817-N8192-K128-epi2-a-a64-c0-contig-alias"],
    # R is plain whatever C is: with C planes the plane formula reads other rows of R, its padding and past its end
    "res_read_as_planes": ["tile1-M513-N1024-K128-epi2-c-a0-c256-pad", "tile2-M145-N1024-K192-epi2-ac-a64-c512-contig-rpb73"],
}


def test_every_mutant_has_named_killers():
    assert set(KILLED_BY) == set(R.BLOCKED_MUTANTS)
    for mutant, ids in KILLED_BY.items():
        assert ids and all(i in BY_ID for i in ids), (mutant, [i for i in ids if i not in BY_ID])


@pytest.mark.parametrize("mutant", R.BLOCKED_MUTANTS)
def test_blocked_mutants_are_caught(mutant):
    named = [BY_ID[i] for i in KILLED_BY[mutant]]
    caught = {}
    for c in SMALL + [c for c in named if c not in SMALL]:
        why = _run(c, mutant)
        if why is not None:
            caught[R.blocked_id(c)] = why.split(" (")[0]
    print(f"sp-slab-edge mutant {mutant}: caught by {len(caught)} cases: " + ", ".join(f"{k} [{v}]" for k, v in caught.items()))
    for c in named:
        assert R.blocked_id(c) in caught, f"{mutant} survives {R.blocked_id(c)}"
    if mutant != "tail_rows_plane0":
        assert all(_run(c) is None for c in named[:1]), "the same case passes the correct stand-in"
