"""The host walk: libdrn's launch logic on the CPU under ASan and UBSan (tools/host_walk.py; DESIGN.md, host walk).

tools/host_walk.py compiles the HOST half of csrc/*.hip with the sanitizers, links it with the recording stand-in for the HIP runtime
(tests/host/hip_recorder.cpp) and the table-driven program (tests/host/host_walk*.cpp) and runs it: every launching entry of
include/drn.h gets a valid call and its refusals one at a time, the forward sequencer is walked through its workspaces, cuts, reruns
and injected failures, the plans are compared with the launches, and the sizes no GPU run reaches are walked for their grids.

Nothing here runs on a GPU and nothing is loaded into Python: the program is a process of its own.  Sanitizers do not run on the GPU
machines, so the module skips where a GPU is visible (and where hipcc is absent); everywhere else it must run.
"""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _gpu_visible():
    if os.path.exists("/dev/kfd"):
        return True
    try:
        import torch
        return bool(torch.cuda.is_available())
    except Exception:
        return False


pytestmark = [
    pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is needed for the host-only compile"),
    pytest.mark.skipif(_gpu_visible(), reason="sanitizer builds are not run on a machine with a GPU"),
]


@pytest.fixture(scope="module")
def walk():
    import host_walk
    host_walk.build()
    return host_walk


@pytest.fixture(scope="module")
def run(walk):
    """ONE run of the whole program, shared by the tests below."""
    return walk.run()


def launching_entries():
    """Every entry of include/drn.h that takes a `stream`: the launching entries."""
    text = open(os.path.join(ROOT, "include", "drn.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = []
    for m in re.finditer(r"\b(drn_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text):
        if re.search(r"void\s*\*\s*stream\s*$", m.group(2).strip()):
            names.append(m.group(1))
    return names


def test_the_header_parse_finds_the_entries():
    names = launching_entries()
    assert len(names) == len(set(names)) and len(names) >= 69
    for known in ("drn_gemm_bf16", "drn_dit_forward", "drn_dit_forward_range", "drn_cl_to_planar", "drn_ensemble_reduce_affine_u8",
                  "drn_env_project_seq"):
        assert known in names
    assert "drn_attention_plan" not in names and "drn_timer_create" not in names


def test_every_launching_entry_is_walked(walk):
    """The coverage rule: --list names every entry of drn.h that takes a stream; an entry added without a case fails here."""
    p = walk.run(["--list"])
    assert p.returncode == 0 and p.stderr == ""
    listed = p.stdout.split()
    assert len(listed) == len(set(listed))
    missing = sorted(set(launching_entries()) - set(listed))
    assert not missing, f"launching entries without a host-walk case: {missing}"
    assert not sorted(set(listed) - set(launching_entries())), "the program lists a name that is not a launching entry"


def test_the_walk_is_clean(run):
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stderr == "", run.stderr[-4000:]            # a sanitizer report goes to stderr
    assert "FAIL" not in run.stdout


def test_the_tally_matches_the_tables(run):
    lines = run.stdout.splitlines()
    assert lines[-1].startswith("tally ")
    tally = {k: int(v) for k, v in zip(*[iter(lines[-1].split()[1:])] * 2)}
    assert set(tally) >= {"entries", "cases", "ok", "refusals", "injected", "host_only", "launches", "attribute_calls"}
    cases = [ln for ln in lines if ln.startswith("case ")]
    assert tally["cases"] == len(cases)
    assert tally["entries"] == len(launching_entries())
    n_ok = sum(1 for ln in cases if re.search(r"\bOK +launches \d+$", ln))
    n_ref = sum(1 for ln in cases if re.search(r"\bEINVAL launches 0$", ln))
    assert n_ok + n_ref == len(cases)                      # every case line is one of the two outcomes
    assert tally["refusals"] == n_ref and tally["ok"] <= n_ok      # (the cut and injection lines are OK lines of many calls each)
    # every launching entry has its valid base call and at least one refusal of its own
    for name in launching_entries():
        own = [ln for ln in cases if ln.startswith("case %s: " % name)]
        if name == "drn_dit_forward":                      # its valid calls are section C's
            own += [ln for ln in cases if ln.startswith("case forward ") and "workspaces as the sizers say" in ln]
        assert any(re.search(r"\bOK +launches [1-9]", ln) for ln in own), name
        assert any("EINVAL" in ln for ln in own), name
    # section C: all five shapes, every precision mode, every workspace one byte short
    fw = [ln for ln in cases if ln.startswith("case forward ")]
    for shape in ("D 256 L 2 x fcm heads 2 S 128 B 1", "D 256 L 2 x fcm heads 2 S 128 B 3", "D 2048 L 2 x fcm heads 16 S 256 B 1",
                  "D 4096 L 28 x fcm heads 32 S 256 B 1", "D 4096 L 28 x fcm heads 32 S 18432 B 1"):
        for mode in ("precision 0 fused 0 attn 0", "precision 0 fused 0 attn 1", "precision 1 fused 0 attn 0",
                     "precision 1 fused 0 attn 1", "precision 1 fused 1 attn 0", "precision 1 fused 1 attn 1"):
            mine = [ln for ln in fw if f"forward {shape} {mode}:" in ln]
            assert any("workspaces as the sizers say" in ln for ln in mine), (shape, mode)
            assert any("every cut" in ln for ln in mine), (shape, mode)
            if mode.startswith("precision 1"):
                assert any("AQ | AS one byte short" in ln and "EINVAL" in ln for ln in mine), (shape, mode)
            if "fused 1" in mode:
                assert any("UQ | US one byte short" in ln and "EINVAL" in ln for ln in mine), (shape, mode)
            if mode.endswith("attn 1"):
                assert any("mx_attn one byte short" in ln and "EINVAL" in ln for ln in mine), (shape, mode)
            if "L 2 " in shape:
                assert any("a failure injected at every launch" in ln for ln in mine), (shape, mode)
    assert any("gemm_ws one byte short" in ln for ln in fw) and any("attn_ws one byte short" in ln for ln in fw)
    assert tally["injected"] > 0 and tally["host_only"] > 0 and tally["launches"] > tally["ok"]
    m = re.search(r"^attention plans walked (\d+)$", run.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 5 * 40                 # five head counts x the sweep of S up to 20 000


def test_the_program_does_not_link_the_hip_runtime(walk):
    out = subprocess.run(["ldd", walk.EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    assert "amdhip64" not in out and "libhsa" not in out, out


def test_gemm_plans_equal_launches(walk, tmp_path):
    """Section B: the cases of tests/golden/gemm_plans.json, handed to the program as text, under every forced tile (one process)
    and every switch recorded there (a process each: the switches are read once)."""
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_plans.json")))
    clean = {k: v for k, v in os.environ.items() if not (k.startswith("DRN_GEMM") or k == "DRN_SPLITK256")}
    by_env = {}
    for r in table["runs"]:
        by_env.setdefault(json.dumps(r["env"], sort_keys=True), []).append(r)
    assert len(by_env) == 1 + len(table["grid"]["switches"])
    for key, runs in by_env.items():
        path = tmp_path / "plans.txt"
        rows = [(r["force_tile"], c[0], c[1], c[2], c[3]) for r in runs for c in r["cases"]]
        path.write_text("".join("%d %d %d %d %d\n" % row for row in rows))
        env = dict(clean, **json.loads(key))
        p = subprocess.run([walk.EXE, "--gemm-cases", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
        assert p.returncode == 0 and p.stderr == "", (key, p.stdout[-1500:], p.stderr[-3000:])
        m = re.search(r"^plans lines (\d+) products (\d+) launches (\d+) refusals (\d+)$", p.stdout, flags=re.M)
        assert m and int(m.group(1)) == len(rows) and int(m.group(2)) >= 9 * len(rows) and int(m.group(3)) > 0, (key, p.stdout[-500:])
