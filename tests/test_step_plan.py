"""The fused train step's planning (csrc/hbk_mlp_plan.h) on the CPU.

tests/step_plan_check.cpp includes that header alone. It is built here as a
stand-alone program with AddressSanitizer and UBSan and run as a child process:
for a grid of batch sizes, stream widths (CUs), network depths and forced knobs
it asserts the plan's invariants (layout regions ascending, aligned and disjoint;
split counts within the partial slabs; job table, k1c and k2 grid bounds) and
prints every field of every plan. The output must equal, exactly, the table
recorded from the tree before the planning was split out of hbk_mlp_fused.hip
(tests/golden/step_plan_parent.json).
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hey-buddy_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "step_plan_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_plan_parent.json")


def _compilers():
    """The C++ compiler beside the project's hipcc, then the system ones."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    beside = [os.path.join(os.path.dirname(hipcc), n) for n in ("amdclang++", "clang++")]
    system = [shutil.which(n) for n in ("c++", "g++", "clang++")]
    return [c for c in beside + system if c and os.path.exists(c)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_plan") / "step_plan_check")
    errors = []
    for cxx in _compilers():
        # The sanitizer runtimes are linked statically, so the program runs in whatever environment
        # the suite runs in: clang does that by default (and rejects gcc's flags), gcc when told to.
        is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", *static, "-I", CSRC, SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{' '.join(cmd)}\n{r.stderr}")
    pytest.fail("no C++ compiler built tests/step_plan_check.cpp with the sanitizers:\n" + "\n".join(errors))


def test_plans_hold_their_invariants_and_equal_the_recorded_table(checker):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HBK_")}  # (the knobs' defaults)
    r = subprocess.run([checker], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]  # no invariant message, no sanitizer report
    got = json.loads(r.stdout)
    want = json.load(open(GOLDEN))
    assert got["fields"] == want["fields"]
    assert len(got["rows"]) == len(want["rows"]) >= 500
    for g, w in zip(got["rows"], want["rows"]):
        assert g == w, dict(zip(["knobs", "B", "NG", "cus"], w[:4]))
