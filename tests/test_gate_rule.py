"""The train step's accumulation gate (csrc/hbk_mlp_gate.h: one function, used by gate_kernel,
k4_update_kernel and, under HBK_STEP_GATE_SKIP, the weight-gradient kernels) on the CPU.

tests/gate_rule_check.cpp includes that header alone. It is built here as a stand-alone
program with AddressSanitizer and UBSan and run as a child process over walks of n_sel; its
acc_samples, acc_steps, t, fire and scale must equal, exactly, the rule of
tests/step_oracle_cases.py's gated_walk (lines 341-348: the reference's trainer.py:443-465)
restated below in float32.
"""
import os
import subprocess

import numpy as np
import pytest

from test_step_plan import _compilers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hey-buddy_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "gate_rule_check.cpp")

WALKS = [
    [0], [127], [128], [1], [1100],
    [0, 0, 0], [127, 0, 1], [127, 1],  # 128 reached exactly on the second step (n_sel = 0 steps in between)
    [128, 128, 127, 128],              # crosses after 1 step, again, then after 2
    [100, 28], [100, 27, 1], [60, 60, 8],  # crosses after 2 and after 3 steps, exactly at 128
    [60, 60, 40, 0, 300, 90],          # gated_walk's own
    [50, 50, 27, 0, 0, 1, 500, 3],     # crosses after 3 steps with empty steps inside the run
    [101, 99, 80, 113, 102, 100, 97, 103],  # the headline's range: every second step fires
    [1] * 130,                         # 128 steps of one row: acc_steps reaches 128
]


def rule(walk):
    """gated_walk's gate in float32 -> rows (acc_samples, acc_steps, t, fire, scale bits)."""
    f = np.float32
    acc_samples, acc_steps, t = f(0), f(1), f(0)
    out = []
    for n in walk:
        n = f(n)
        fire, scale = f(0), f(0)
        if n > 0:
            acc_samples = f(acc_samples + n)
            if acc_samples < 128:
                acc_steps = f(acc_steps + f(1))
            else:
                fire, scale = f(1), f(f(1) / f(n * acc_steps))
                acc_steps, acc_samples, t = f(1), f(0), f(t + f(1))
        out.append((float(acc_samples), float(acc_steps), float(t), float(fire), int(np.float32(scale).view(np.uint32))))
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gate_rule") / "gate_rule_check")
    errors = []
    for cxx in _compilers():
        is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", *static, "-I", CSRC, SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{' '.join(cmd)}\n{r.stderr}")
    pytest.fail("no C++ compiler built tests/gate_rule_check.cpp with the sanitizers:\n" + "\n".join(errors))


def test_rule_restated_matches_gated_walk_flags():
    """The restatement itself, against what the oracle's walk records (fired, steps used)."""
    fired = [r[3] for r in rule([60, 60, 40, 0, 300, 90])]
    assert fired == [0, 0, 1, 0, 1, 0]
    assert [r[1] for r in rule([60, 60, 40, 0, 300, 90])] == [2, 3, 1, 1, 1, 2]


def test_gate_header_matches_the_rule(checker):
    text = "".join(" ".join(str(n) for n in w) + "\n" for w in WALKS)
    r = subprocess.run([checker], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]  # no sanitizer report
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == sum(len(w) for w in WALKS)
    it = iter(rows)
    for wi, walk in enumerate(WALKS):
        for si, want in enumerate(rule(walk)):
            got = next(it)
            assert (int(got[0]), int(got[1])) == (wi, si)
            assert tuple(float(v) for v in got[2:6]) == want[:4], (walk, si, got, want)
            assert int(got[6], 16) == want[4], (walk, si, got, want)
    # the walks cover what they are meant to: no fire, fire at once, after 2 and after 3 steps
    runs = set()
    for walk in WALKS:
        n = 0
        for r_ in rule(walk):
            n += 1
            if r_[3]:
                runs.add(n)
                n = 0
    assert {1, 2, 3} <= runs
