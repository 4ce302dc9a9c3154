"""Where the GEMM dispatcher takes the 384 x 256 tile (csrc/gemm384.hip, tile kernel 5): drn_gemm_plan_choice, host only - nothing
is launched.  The tile is enabled per shape, only where an interleaved A/B measured it faster than the plan before it
(profiles/gemm384.txt); everywhere else, and everywhere under DRN_GEMM384=0, the plan is the one drn_gemm_tile_choice describes."""
import ctypes
import os
import subprocess
import sys

from conftest import ROOT

TILE384 = 5
S = 18432
# the four block linears of the headline step (cfg 3, 18 432 tokens): (N, K), and whether the A/B enabled the tile for them
HEADLINE = {"qkv": (12288, 4096), "out-proj": (4096, 4096), "mlp-up": (16384, 4096), "mlp-down": (4096, 16384)}
ENABLED = ("mlp-down",)     # the HEADLINE shapes on csrc/gemm_plan.h's kGemm384Measured list (profiles/gemm384.txt: the others tie)


def _plan(lib, M, N, K, rpb=0):
    rows = ctypes.c_int64(-1)
    tile = lib.drn_gemm_plan_choice(M, N, K, rpb, ctypes.byref(rows))
    return tile, rows.value


def test_headline_shapes(pkg):
    lib = pkg.native.load_library()
    for name, (N, K) in HEADLINE.items():
        tile, rows = _plan(lib, S, N, K)
        if name in ENABLED:
            assert (tile, rows) == (TILE384, S), name
        else:
            assert tile == lib.drn_gemm_tile_choice(S, N) == 1, name
        # a batch of 5 clips of 18 432 rows: the plan of one clip
        assert _plan(lib, 5 * S, N, K, S) == (tile, rows), name


def test_other_shapes_keep_their_plan(pkg):
    lib = pkg.native.load_library()
    for M in (256, 1024, 2048, 2304, 4608, 6912, 9216, 18431):
        for N, K in HEADLINE.values():
            tile, rows = _plan(lib, M, N, K)
            assert tile == lib.drn_gemm_tile_choice(M, N) and tile != TILE384, (M, N, K)
            assert 0 < rows <= M
    # 72 x 16 tiles of 256^2 = 4.5 rounds: 4 whole rounds, then a tail (144-row bands) - as before
    assert _plan(lib, S, 4096, 4096) == ((TILE384, S) if "out-proj" in ENABLED else (1, 16384))
    assert lib.drn_gemm_tile_choice(S, 16384) == 1 and lib.drn_gemm_tile_choice(2304, 4096) == 2


def test_forced_tile_is_reported_and_released(pkg):
    lib = pkg.native.load_library()
    lib.drn_gemm_force_tile(TILE384)
    try:
        assert _plan(lib, 768, 512, 128) == (TILE384, 768)
    finally:
        lib.drn_gemm_force_tile(-1)
    assert _plan(lib, 768, 512, 128)[0] != TILE384
    assert lib.drn_gemm_plan_choice(0, 256, 64, 0, None) == -1 and lib.drn_gemm_plan_choice(256, 100, 64, 0, None) == -1


def test_switch(pkg):
    """DRN_GEMM384=0: the plan before this tile, everywhere; DRN_GEMM384=2 (A/B runs): every shape whose 384-row tiling fills whole
    rounds or costs fewer round-equivalents, measured or not - and still nothing else."""
    code = (
        "import ctypes, sys\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from __graft_entry__ import load_package\n"
        "lib = load_package().native.load_library()\n"
        "def plan(M, N, K):\n"
        "    r = ctypes.c_int64(-1)\n"
        "    return lib.drn_gemm_plan_choice(M, N, K, 0, ctypes.byref(r)), r.value\n"
        "shapes = [(M, N, K) for M in (256, 384, 768, 1024, 2304, 18431, 18432) for N, K in ((12288, 4096), (4096, 4096), (16384, 4096), (4096, 16384))]\n"
        "print([plan(*s) for s in shapes])\n"
        "print([lib.drn_gemm_tile_choice(M, N) for M, N, K in shapes])\n")

    def run(value):
        env = dict(os.environ)
        env.pop("DRN_GEMM384", None)
        if value is not None:
            env["DRN_GEMM384"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.strip().split("\n")
        return eval(out[-2]), eval(out[-1])

    off, old = run("0")
    assert [t for t, _ in off] == old and all(t != TILE384 for t in old)
    every, _ = run("2")
    n = len(every)
    assert [p for p in every[n - 4:]] == [(TILE384, S)] * 4                    # M = 18 432: all four linears in whole rounds
    assert every[:n - 4] == off[:n - 4]                                       # no other M here changes its plan
    default, _ = run(None)
    want = [(TILE384, S) if name in ENABLED else o for name, o in zip(HEADLINE, off[n - 4:])]
    assert default[:n - 4] == off[:n - 4] and default[n - 4:] == want
