"""The launch plan of the bf16 GEMM (csrc/gemm_plan.h), host only - nothing is launched.  drn_gemm_plan_describe is the planner the
GEMM entries execute; it, drn_gemm_plan_choice, drn_gemm_tile_choice and drn_gemm_splitk_choice are held to
tests/golden/gemm_plans.json, a table recorded from the three older queries of the commit before the planner existed (a plain,
contiguous clip: every tile kernel, the tail split, the 384-row tile, every switch and every forced tile).  What those queries could
not show - blocked layouts, ragged clips, row strides past the 384-row kernel's 32-bit test, the few-token kernel as a launch, the
slice kernel of a split-K product - is held to the independent model in dit_refs.py."""
import ctypes
import json
import os
import subprocess
import sys

import dit_refs as R
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plans.json")
ALIAS = {3: 1, 4: 1}                                   # forced tiles 3 and 4 are the 256 x 256 kernel: describe reports the kernel


def _table():
    with open(GOLDEN) as f:
        return json.load(f)


def describe(lib, M, N, K, ld=None, epi=R.EPI_NONE, rpb=0, abc=0, cbc=0, splits=1, cap=64):
    """drn_gemm_plan_describe -> [(kernel, first row, rows, rows_per_batch)] or None (refused)."""
    lda, ldw, ldc, ldr = ld or (abc or K, K, cbc or N, N)
    out = (ctypes.c_int64 * (4 * cap))()
    n = lib.drn_gemm_plan_describe(M, N, K, lda, ldw, ldc, ldr, epi, rpb, abc, cbc, splits, out, cap)
    assert n <= cap
    return None if n < 0 else [tuple(out[4 * i:4 * i + 4]) for i in range(n)]


def queries(lib, cases):
    """Per case [one clip's chain of drn_gemm_plan_choice, tile choice, split-K choice, the first plan_choice of the call, describe]."""
    out = []
    for M, N, K, rpb in cases:
        Mb, r, chain, rest = rpb or M, ctypes.c_int64(-1), [], rpb or M
        first = [lib.drn_gemm_plan_choice(M, N, K, rpb, ctypes.byref(r)), r.value]
        while rest > 0 and len(chain) < 16:
            chain.append([lib.drn_gemm_plan_choice(rest, N, K, 0, ctypes.byref(r)), r.value])
            rest -= max(r.value, 1)
        out.append([chain, lib.drn_gemm_tile_choice(Mb, N), lib.drn_gemm_splitk_choice(Mb, N, K), first, describe(lib, M, N, K, rpb=rpb)])
    return out


def check_run(run, got):
    """One run of the table (an environment, a forced tile) against what the library answers under it."""
    force, tall_on = run["force_tile"], run["env"].get("DRN_GEMM_TALL") != "0" and run["force_tile"] < 0
    for (M, N, K, rpb, chain, tile, splitk), (g_chain, g_tile, g_splitk, g_first, g_desc) in zip(run["cases"], got):
        what = (run["env"], force, M, N, K, rpb)
        assert (g_chain, g_tile, g_splitk, g_first) == (chain, tile, splitk, chain[0]), what
        Mb = rpb or M
        # the few-token kernel: the model, which the recorded split-K choice confirms wherever that kernel splits or stands alone
        tall = R.gemm_tall_slices(Mb, N, K) if tall_on else 0
        if tall:
            assert splitk == tall, what
        if tall == 1 and M % 256 == 0:
            want = [(6, 0, M, rpb or M)]
        elif len(chain) == 1:
            want = [(ALIAS.get(chain[0][0], chain[0][0]), 0, M, Mb)]
            if want[0][0] == 5 and not R.gemm384_ok(M, N, K, max(N, K)):
                want = None                            # a forced 384-row tile on rows it cannot take: refused
        else:
            want, row = [], 0
            for b in range(M // Mb):
                for t, rows in chain:
                    want.append((ALIAS.get(t, t), row, rows, rows))
                    row += rows
        assert g_desc == (None if want is None else [list(x) for x in want]), what
        if g_desc is not None:
            assert_plan_invariants(g_desc, M, what)


def assert_plan_invariants(plan, M, what):
    row = 0
    for kernel, row0, rows, rpb in plan:
        assert row0 == row and rows > 0 and rpb > 0, what               # the launches tile [0, M) exactly, in order
        row += rows
        if kernel == 5:                                                 # whole 384-row tiles, each inside one clip
            assert rows % 384 == 0 and (rpb >= rows or rpb % 384 == 0), what
        if kernel == 6:
            assert len(plan) == 1, what
    assert row == M, what


_CHILD = (
    "import json, sys\n"
    "sys.path[:0] = [{root!r}, {tests!r}]\n"
    "from __graft_entry__ import load_package\n"
    "import test_gemm_plan_cpu as T\n"
    "lib = load_package().native.load_library()\n"
    "print(json.dumps(T.queries(lib, json.loads(sys.argv[1]))))\n")


def test_table_is_the_parents(pkg):
    t = _table()
    assert len(t["parent"]) == 40 and 100 < sum(len(r["cases"]) for r in t["runs"]) < 500
    assert {r["force_tile"] for r in t["runs"]} == set(range(-1, 6))
    assert {f"{k}={v}" for r in t["runs"] for k, v in r["env"].items()} == set(t["grid"]["switches"])


def test_forced_tiles_and_defaults_match_the_table(pkg):
    lib = pkg.native.load_library()
    assert not any(k.startswith("DRN_GEMM") or k == "DRN_SPLITK256" for k in os.environ), "the table's default run has no switch set"
    for run in (r for r in _table()["runs"] if not r["env"]):
        lib.drn_gemm_force_tile(run["force_tile"])
        try:
            got = queries(lib, [c[:4] for c in run["cases"]])
        finally:
            lib.drn_gemm_force_tile(-1)
        check_run(run, json.loads(json.dumps(got)))


def test_switches_match_the_table(pkg):
    """Every switch in a child process of its own (the settings are read once per process), all started together."""
    runs = [r for r in _table()["runs"] if r["env"]]
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    procs = []
    for run in runs:
        env = {k: v for k, v in os.environ.items() if not (k.startswith("DRN_GEMM") or k == "DRN_SPLITK256")}
        env.update(run["env"])
        procs.append(subprocess.Popen([sys.executable, "-c", code, json.dumps([c[:4] for c in run["cases"]])], env=env,
                                      stdout=subprocess.PIPE, text=True))
    for run, p in zip(runs, procs):
        out, _ = p.communicate()
        assert p.returncode == 0, run["env"]
        check_run(run, json.loads(out.strip().split("\n")[-1]))


def _same(lib, M, N, K, **kw):
    """describe == the model; returns the plan."""
    blocked = bool(kw.get("abc") or kw.get("cbc"))
    got = describe(lib, M, N, K, **kw)
    ld = kw.get("ld") or (kw.get("abc") or K, K, kw.get("cbc") or N, N)
    want = R.gemm_plan_launches(M, N, K, ld=ld, epi=kw.get("epi", R.EPI_NONE), rpb=kw.get("rpb", 0), blocked=blocked)
    assert got == want, (M, N, K, kw, got, want)
    if got is not None:
        assert_plan_invariants(got, M, (M, N, K, kw))
    return got


def test_model_agrees_with_the_table(pkg):
    """The model that the tests below lean on, on the table's default run: the same launches as the recorded chains."""
    lib = pkg.native.load_library()
    for M, N, K, rpb, chain, _, _ in _table()["runs"][0]["cases"]:
        plan = R.gemm_plan_launches(M, N, K, rpb=rpb)
        if plan[0][0] != 6:
            assert [[t, n] for t, r, n, _ in plan if r < (rpb or M)] == ([[chain[0][0], M]] if len(chain) == 1 else chain), (M, N, K, rpb)
        assert plan == describe(lib, M, N, K, rpb=rpb)


def test_blocked_layouts(pkg):
    """No 128 x 128 tail, no 384-row tile, refused where the 128 x 128 kernel would be needed."""
    lib = pkg.native.load_library()
    seen = set()
    for M in (64, 256, 300, 2304, 4817, 9216, 9472, 18431, 18432):
        for N, K in ((4096, 4096), (8192, 128), (4096, 16384), (16384, 4096), (12288, 4096), (384, 4096)):
            for kw in (dict(abc=64), dict(cbc=256), dict(abc=128, cbc=1024)) if N % 512 == 0 else (dict(abc=64),):
                plan = _same(lib, M, N, K, **kw)
                seen.add(None if plan is None else tuple(k for k, *_ in plan))
                assert plan is None or all(k in (1, 2) for k, *_ in plan)
    assert {None, (1,), (2,), (1, 2)} <= seen
    assert describe(lib, 9472, 4096, 4096) == [(1, 0, 8192, 8192), (0, 8192, 1280, 1280)]          # plain: a 128 x 128 tail ...
    assert describe(lib, 9472, 4096, 4096, cbc=1024) == [(1, 0, 9472, 9472)]                       # ... in planes: none
    assert describe(lib, 18432, 4096, 16384) == [(5, 0, 18432, 18432)] and describe(lib, 18432, 4096, 16384, abc=64)[0][0] == 1
    lib.drn_gemm_force_tile(5)
    try:
        assert describe(lib, 768, 512, 128) == [(5, 0, 768, 768)] and describe(lib, 768, 512, 128, cbc=256) is None
    finally:
        lib.drn_gemm_force_tile(-1)


def test_ragged_and_batched_clips(pkg):
    lib = pkg.native.load_library()
    G = R.EPI_GATE_RES
    # ragged: one launch with the tile of the whole problem, rows_per_batch passed through - no tail split, no 384-row tile
    assert _same(lib, 4817, 8192, 128, epi=G, rpb=2000) == [(1, 0, 4817, 2000)]
    assert _same(lib, 18432, 4096, 16384, epi=G, rpb=10000) == [(1, 0, 18432, 10000)]
    assert _same(lib, 2304, 4096, 4096, epi=G, rpb=1000) == [(2, 0, 2304, 1000)]
    assert _same(lib, 300, 4096, 4096, epi=G, rpb=200) == [(0, 0, 300, 200)]
    assert _same(lib, 256, 12288, 4096, epi=G, rpb=100) == [(6, 0, 256, 100)]
    # clips in planes: the same route (one launch), refused where that launch would be the 128 x 128 kernel's
    assert _same(lib, 4608, 4096, 1024, epi=G, rpb=2304, abc=128) == [(2, 0, 4608, 2304)]
    assert _same(lib, 512, 4096, 1024, epi=G, rpb=256, abc=128) is None
    # whole clips: the plan of one clip - in one launch for all of them, or repeated clip by clip
    assert _same(lib, 2 * 4817, 8192, 128, epi=G, rpb=4817, ld=(192, 128, 8256, 8320)) == \
        [(1, 0, 4096, 4096), (2, 4096, 721, 721), (1, 4817, 4096, 4096), (2, 8913, 721, 721)]
    assert _same(lib, 5 * 18432, 4096, 16384, epi=G, rpb=18432) == [(5, 0, 5 * 18432, 18432)]
    assert _same(lib, 5 * 256, 16384, 4096, epi=G, rpb=256) == [(6, 0, 1280, 256)]
    assert _same(lib, 3 * 2304, 4096, 4096, rpb=2304) == [(2, 0, 6912, 2304)]
    for M, rpb in ((2 * 9472, 9472), (5 * 4817, 4817), (18432, 0), (18432, 20000), (18431, 7)):
        for N, K in ((4096, 4096), (8192, 128), (4096, 16384), (384, 4096)):
            for epi in (R.EPI_NONE, G):
                _same(lib, M, N, K, epi=epi, rpb=rpb or (M if epi == G else 0))


def test_row_strides_past_the_384_row_kernels_reach(pkg):
    lib = pkg.native.load_library()
    M, N, K = 18432, 4096, 16384
    far = ((1 << 30) - 4096) // 384                    # 384 rows of `far` elements + 4096: 2^31 bytes, one too many
    assert far % 8 == 0 and (384 * far + 4096) * 2 == 1 << 31
    split = [(1, 0, 16384, 16384), (2, 16384, 2048, 2048)]
    assert _same(lib, M, N, K, ld=(K, K, N, N)) == [(5, 0, M, M)]
    assert _same(lib, M, N, K, ld=(far - 8, K, N, N)) == [(5, 0, M, M)]
    assert _same(lib, M, N, K, ld=(far, K, N, N)) == split
    assert _same(lib, M, N, K, ld=(K, far, N, N)) == split and _same(lib, M, N, K, ld=(K, K, far, N)) == split
    assert _same(lib, M, N, K, ld=(K, K, N, far), epi=R.EPI_GATE_RES, rpb=M) == split
    assert _same(lib, M, N, K, ld=(K, K, N, far)) == [(5, 0, M, M)]             # no residual: its stride is not an operand's
    lib.drn_gemm_force_tile(5)
    try:
        assert describe(lib, M, N, K, ld=(far, K, N, N)) is None and describe(lib, M, N, K) == [(5, 0, M, M)]
        assert describe(lib, 2 * 768, 512, 128, epi=R.EPI_GATE_RES, rpb=768) == [(5, 0, 1536, 768)]
        assert describe(lib, 768, 512, 128, epi=R.EPI_GATE_RES, rpb=500) is None          # a tile across two clips
    finally:
        lib.drn_gemm_force_tile(-1)


def test_refused_arguments_and_slices(pkg):
    lib = pkg.native.load_library()
    assert describe(lib, 0, 256, 64) == []
    for bad in (dict(M=-1), dict(N=100), dict(K=96), dict(ld=(60, 64, 256, 256)), dict(ld=(64, 56, 256, 256)), dict(ld=(64, 64, 248, 256)),
                dict(epi=3), dict(epi=R.EPI_GATE_RES, rpb=0), dict(epi=R.EPI_GATE_RES, rpb=8, ld=(64, 64, 256, 128)), dict(abc=48),
                dict(cbc=128), dict(splits=3), dict(splits=128), dict(splits=2, cbc=256)):
        kw = dict(dict(M=256, N=256, K=64), **bad)
        assert describe(lib, kw.pop("M"), kw.pop("N"), kw.pop("K"), **kw) is None, bad
    assert lib.drn_gemm_plan_describe(4817, 8192, 128, 128, 128, 8192, 0, 0, 0, 0, 0, 1, None, 0) == 2        # the count alone
    # the slices of a split-K product: the few-token kernel, the 256-row slices or the 128 x 128 slices - the kernel whose rule names
    # that split count for one clip's rows (the model: gemm_tall_slices; the counts: the table's split-K choices)
    for M, rpb in ((256, 0), (512, 256)):
        assert describe(lib, M, 4096, 4096, rpb=rpb, splits=4) == [(6, 0, M, rpb)]
        assert describe(lib, M, 4096, 16384, rpb=rpb, splits=16) == [(1, 0, M, rpb)]
        assert describe(lib, M, 12288, 4096, rpb=rpb, splits=4) == [(1, 0, M, rpb)]
        assert describe(lib, M, 4096, 4096, rpb=rpb, splits=2) == [(0, 0, M, rpb)]
    for force, want in ((0, 0), (1, 0), (4, 1)):
        lib.drn_gemm_force_tile(force)
        try:
            assert describe(lib, 256, 4096, 16384, splits=16) == [(want, 0, 256, 0)]
        finally:
            lib.drn_gemm_force_tile(-1)
