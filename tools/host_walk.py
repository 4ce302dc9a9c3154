#!/usr/bin/env python3
"""Host walk: libdrn's launch logic on the CPU under ASan and UBSan (host walk; profiles/host_walk.txt).

Compiles the HOST half of every csrc/*.hip (hipcc --cuda-host-only: no device code, seconds) with the sanitizers, links it with
the recording stand-in for the HIP runtime (tests/host/hip_recorder.cpp) and the table-driven program (tests/host/host_walk*.cpp)
using plain clang++ - never against libamdhip64 - and runs the program.  Nothing here touches a GPU or Python's address space.

    python tools/host_walk.py                  build (if stale) and run; exit status of the program
    python tools/host_walk.py --list           the entries the program covers
    python tools/host_walk.py --build-only
    python tools/host_walk.py -- ARGS...       ARGS go to the program
"""
import argparse
import concurrent.futures
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusionrenderer-comfyui_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
OUT = os.path.join(ROOT, "build", "host_walk")
EXE = os.path.join(OUT, "host_walk")

# implicit-conversion is on as well: the library's host code was made clean under it (profiles/host_walk.txt, finding 12)
SAN = ["-fsanitize=address,undefined,float-cast-overflow,implicit-conversion", "-fno-sanitize-recover=all"]
FLAGS = ["-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer"] + SAN
JOBS = min(16, os.cpu_count() or 1)
# families added in files of their own ride behind an existing family: main()'s call of the wrapped function goes to the
# __wrap_ function the new file defines, which runs the old family (__real_) and then its own (tests/host/host_walk_edits.cpp)
WRAPS = ["_ZN2hw15family_picturesEv"]


def _rocm():
    for cand in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if cand and os.path.isdir(os.path.join(cand, "include", "hip")):
            return cand
    hipcc = shutil.which("hipcc")
    if hipcc:
        return os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    raise SystemExit("host_walk: no ROCm installation found (hipcc is needed for the host-only compile)")


def _clangxx(rocm):
    for cand in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")):
        if os.path.exists(cand):
            return cand
    found = shutil.which("clang++")
    if not found:
        raise SystemExit("host_walk: clang++ not found")
    return found


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _run(cmd):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise SystemExit("host_walk: failed: %s\n%s" % (" ".join(cmd), p.stdout))


def build(verbose=False):
    """-> (path of the program, seconds spent compiling; 0.0 when nothing was stale)"""
    rocm = _rocm()
    cxx = _clangxx(rocm)
    os.makedirs(OUT, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hpp"))]
    headers.append(os.path.join(ROOT, "include", "drn.h"))
    host_headers = [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".h")]
    me = os.path.abspath(__file__)
    inc = ["-I", os.path.join(ROOT, "include"), "-I", CSRC]
    jobs = []
    lib_objs = []
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith(".hip"):
            continue
        src, obj = os.path.join(CSRC, f), os.path.join(OUT, f[:-4] + ".o")
        lib_objs.append(obj)
        if _newer(obj, [src, me] + headers):
            jobs.append(["hipcc", "--cuda-host-only", "--offload-arch=gfx950", "-fPIE", "-Wno-unused-result"] + FLAGS + inc +
                        ["-c", src, "-o", obj])
    prog_objs = []
    for f in sorted(os.listdir(HOST)):
        if not f.endswith(".cpp"):
            continue
        src, obj = os.path.join(HOST, f), os.path.join(OUT, "t_" + f[:-4] + ".o")
        prog_objs.append(obj)
        if _newer(obj, [src, me, os.path.join(ROOT, "include", "drn.h")] + host_headers):
            jobs.append([cxx, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", HOST, "-fPIE"] + FLAGS + inc +
                        ["-c", src, "-o", obj])
    t0 = time.time()
    if jobs:
        if verbose:
            print("host_walk: compiling %d files with %d jobs" % (len(jobs), JOBS), file=sys.stderr)
        with concurrent.futures.ThreadPoolExecutor(JOBS) as pool:
            list(pool.map(_run, jobs))
    stubs_c = os.path.join(OUT, "fatbin_stubs.c")
    stubs_o = os.path.join(OUT, "fatbin_stubs.o")
    if jobs or _newer(EXE, lib_objs + prog_objs):
        # a host-only object still refers to the device image it would have embedded: one dummy definition each
        nm = shutil.which("nm") or os.path.join(os.path.dirname(cxx), "llvm-nm")
        names = set()
        for line in subprocess.check_output([nm, "-u"] + lib_objs, text=True).split("\n"):
            parts = line.split()
            if parts and parts[-1].startswith("__hip_fatbin_"):
                names.add(parts[-1])
        with open(stubs_c, "w") as fh:
            for n in sorted(names):
                fh.write("const char %s[8] = {0};\n" % n)
        cc = os.path.join(os.path.dirname(cxx), "clang")      # the C driver beside clang++
        _run([cc if os.path.exists(cc) else cxx, "-x", "c", "-c", stubs_c, "-o", stubs_o])
        _run([cxx] + SAN + ["-g", "-o", EXE] + ["-Wl,--wrap=" + w for w in WRAPS] + prog_objs + lib_objs + [stubs_o])
    return EXE, (time.time() - t0 if jobs else 0.0)


def run(args=()):
    """-> CompletedProcess of the program (stdout, stderr captured as text)"""
    env = dict(os.environ)
    env.setdefault("ASAN_OPTIONS", "detect_leaks=1:abort_on_error=0")
    env.setdefault("UBSAN_OPTIONS", "print_stacktrace=1")
    return subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--gemm-cases", help="text file of GEMM plan cases (tests/test_host_walk_cpu.py writes it from the golden)")
    ap.add_argument("rest", nargs="*")
    a = ap.parse_args()
    _, secs = build(verbose=True)
    if secs:
        print("host_walk: built in %.1f s" % secs, file=sys.stderr)
    if a.build_only:
        return 0
    args = (["--list"] if a.list else []) + list(a.rest)
    if a.gemm_cases:
        args += ["--gemm-cases", a.gemm_cases]
    t0 = time.time()
    p = run(args)
    sys.stdout.write(p.stdout)
    sys.stderr.write(p.stderr)
    print("host_walk: ran in %.2f s, exit %d" % (time.time() - t0, p.returncode), file=sys.stderr)
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
