"""QKV and MLP-up of the DiT forward at 18 432 tokens run in whole rounds of the 256 CUs: 48 x 48 = 2304 and 48 x 64 = 3072 workgroups
of the 384 x 256 tile are 9 and 12 rounds, where 256^2 tiles are 13.5 (paid as 14) and 18 (profiles/harvest_18k.txt).  The forward asks
for that through GemmShape::measured384 (csrc/gemm_plan.h, drn_gemm_bf16_measured384); what every other caller gets is unchanged.
Host only, nothing is launched: drn_gemm_plan_describe for the plans of the C ABI, a small C++ program over gemm_plan.h for the flag.

The sweep equals tests/golden/gemm_plans_before_qkv_rounds.json, the same sweep recorded from the planner of the commit before
(regenerate: `python tests/test_qkv_rounds_cpu.py OUT.json` with that commit's library)."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

if __name__ != "__main__":
    from conftest import GOLDEN, ROOT

FIXTURE = "gemm_plans_before_qkv_rounds.json"
K384 = 5
MS = ((256, 0), (1024, 0), (2304, 0), (4608, 0), (18432, 0), (36864, 18432))        # (rows, rows of one clip; 0 = one clip)
NS, KS = (4096, 12288, 16384), (4096, 16384)
LAYOUTS = {"plain": (0, 0), "a_blocked": (1024, 0), "c_blocked": (0, 1024), "both_blocked": (1024, 1024)}


def describe(lib, M, N, K, epilogue, rpb, a_cols, c_cols):
    out = (ctypes.c_int64 * 64)()
    n = lib.drn_gemm_plan_describe(M, N, K, K, K, N, N, epilogue, rpb if rpb else M, a_cols, c_cols, 1, out, 16)
    assert n <= 16
    return n if n < 0 else [list(out[4 * i:4 * i + 4]) for i in range(n)]


def sweep(lib):
    plans = {}
    for M, rpb in MS:
        for N in NS:
            for K in KS:
                for epilogue in (0, 1, 2):
                    for layout, (a_cols, c_cols) in LAYOUTS.items():
                        plans[f"M{M} rpb{rpb} N{N} K{K} epi{epilogue} {layout}"] = describe(lib, M, N, K, epilogue, rpb, a_cols, c_cols)
    return plans


def test_every_plan_of_the_abi_is_the_one_before(pkg):
    lib = pkg.native.load_library()
    with open(os.path.join(GOLDEN, FIXTURE)) as f:
        before = json.load(f)
    now = sweep(lib)
    assert len(now) == 6 * 3 * 2 * 3 * 4 and now == before, sorted(k for k in set(now) | set(before) if now.get(k) != before.get(k))


_PROGRAM = r"""
#include <stdio.h>
#include "gemm_plan.h"
// argv-free: one line per case, "name: kernel row0 rows rpb; ..." or "name: refused"
static void plan(const char* name, const GemmSettings& s, GemmShape p) {
    printf("%s:", name);
    GemmLaunch L{0, 0, p.M, p.rows_per_batch};
    for (int64_t row = 0; row < p.M; row += L.rows) {
        if (gemm_plan_next(s, p, row, &L) != DRN_OK) { printf(" refused\n"); return; }
        printf(" %d %lld %lld %lld;", L.kernel, (long long)L.row0, (long long)L.rows, (long long)L.rows_per_batch);
    }
    printf("\n");
}
static GemmShape shape(int64_t M, int64_t N, int64_t K, int epi, int64_t rpb, bool measured) {
    GemmShape p{M, N, K, K, K, N, N, epi, rpb, {62, 0, 62, 0}};
    p.measured384 = measured;
    return p;
}
int main() {
    GemmSettings s, off, forced;
    off.mode384 = 0;
    forced.set_force(1);
    const int64_t S = 18432;
    plan("qkv", s, shape(S, 12288, 4096, DRN_EPI_NONE, S, true));
    plan("qkv plain", s, shape(S, 12288, 4096, DRN_EPI_NONE, S, false));
    plan("qkv two clips", s, shape(2 * S, 12288, 4096, DRN_EPI_NONE, S, true));
    plan("mlp-up", s, shape(S, 16384, 4096, DRN_EPI_GELU, S, true));
    plan("mlp-up plain", s, shape(S, 16384, 4096, DRN_EPI_GELU, S, false));
    plan("qkv switched off", off, shape(S, 12288, 4096, DRN_EPI_NONE, S, true));
    plan("qkv forced tile", forced, shape(S, 12288, 4096, DRN_EPI_NONE, S, true));
    plan("band", s, shape(2304, 4096, 4096, DRN_EPI_NONE, 2304, true));          // 96 tiles of 384 x 256: dearer than 144-row tiles
    plan("ragged", s, shape(18431, 12288, 4096, DRN_EPI_NONE, 18431, true));     // not whole 384-row tiles
    GemmShape b = shape(S, 12288, 4096, DRN_EPI_NONE, S, true);
    b.blk[2] = 10, b.blk[3] = S * 1024;                                          // C in planes of 1024 columns
    plan("qkv in planes", s, b);
    return 0;
}
"""


def _cxx():
    for name in ("g++", "c++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    hipcc = shutil.which("hipcc")
    assert hipcc, "no C++ compiler found"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")):
        if os.path.exists(cand):
            return cand
    raise AssertionError("no C++ compiler found")


def test_the_forwards_flag_takes_whole_rounds_and_nothing_else(tmp_path):
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(_PROGRAM)
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "diffusionrenderer-comfyui_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.strip().split("\n"):
        name, _, rest = line.partition(":")
        got[name] = None if "refused" in rest else [[int(v) for v in rec.split()] for rec in rest.split(";") if rec.strip()]
    S = 18432
    assert got["qkv"] == [[K384, 0, S, S]] and (S // 384) * (12288 // 256) == 9 * 256
    assert got["mlp-up"] == [[K384, 0, S, S]] and (S // 384) * (16384 // 256) == 12 * 256
    assert got["qkv two clips"] == [[K384, 0, 2 * S, S]]                       # the plan of one clip, in one launch
    one_256 = [[1, 0, S, S]]
    assert got["qkv plain"] == got["mlp-up plain"] == got["qkv switched off"] == got["qkv forced tile"] == got["qkv in planes"] == one_256
    assert got["band"] == [[2, 0, 2304, 2304]]
    assert got["ragged"] is not None and all(rec[0] != K384 for rec in got["ragged"])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package
    with open(sys.argv[1], "w") as f:
        json.dump(sweep(load_package().native.load_library()), f, indent=0, sort_keys=True)
