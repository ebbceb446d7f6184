"""The augmentation units' host logic (csrc/hbk_augment_plan.h) on the CPU.

tests/augment_plan_check.cpp includes that header alone. It is built here as a
stand-alone program with AddressSanitizer and UBSan and run as a child process.
It asserts the invariants of the pitch shift's geometry, workspace layout and
launch grids (offsets ascending, aligned, regions disjoint and large enough for
what the kernels address in them; positive grids; nw <= 128, taps <=
HBK_PITCH_SHIFT_MAX_TAPS), of the band-stop and colored-noise layouts and of
the reverb tables (every float against the formula restated there, 256-B
aligned table starts, zero unmapped slots, one allocation), and prints every
geometry, layout and grid. The output must equal, exactly, the table recorded
from the tree before the host block was split out of hbk_augment.hip
(tests/golden/augment_plan_parent.json; DESIGN.md says how it was made).
"""
import json
import os
import subprocess

import pytest

from test_step_plan import _compilers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hey-buddy_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "augment_plan_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "augment_plan_parent.json")

PITCH_CASES = [(23040, 16000, 128, 125), (23040, 16000, 125, 128), (126, 16000, 128, 125), (125, 16000, 128, 125),
               (1 << 24, 16000, 128, 125), ((1 << 24) + 1, 16000, 128, 125), (23040, 22050, 128, 125),
               (23040, 16000, 3, 2), (23040, 16000, 0, 125), (23040, 16000, 128, 0)]
ACCEPTED = PITCH_CASES[:3] + PITCH_CASES[4:5]
COLORED_CASES = [(0, 4), (5, 1), (5, 2), (4, 4), (5, 4), (1 << 20, 3)]
BAND_STOP_CASES = [(1, 1, 1, 1), (5, 2, 3, 5), (300, 3, 7, 256)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("augment_plan") / "augment_plan_check")
    errors = []
    for cxx in _compilers():
        # (static sanitizer runtimes, as tests/test_step_plan.py)
        is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", *static, "-I", CSRC, SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{' '.join(cmd)}\n{r.stderr}")
    pytest.fail("no C++ compiler built tests/augment_plan_check.cpp with the sanitizers:\n" + "\n".join(errors))


@pytest.fixture(scope="module")
def table(checker):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HBK_")}
    r = subprocess.run([checker], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]  # no invariant message, no sanitizer report
    return json.loads(r.stdout)


def test_layouts_hold_their_invariants_and_equal_the_recorded_table(table):
    want = json.load(open(GOLDEN))
    assert table.keys() == want.keys()
    for key in want:
        if isinstance(want[key], list):
            assert len(table[key]) == len(want[key]), key
            for g, w in zip(table[key], want[key]):
                assert g == w, (key, {k: v for k, v in w.items() if not isinstance(v, (list, dict))})
        else:
            assert table[key] == want[key], key
    # what the table must hold: the issue's cases, in order, the refusals by status and text
    assert [(c["L"], c["sample_rate"], c["num"], c["den"]) for c in want["pitch"]] == PITCH_CASES
    for c in want["pitch"]:
        case = (c["L"], c["sample_rate"], c["num"], c["den"])
        assert (c["rc"] == 0) == (case in ACCEPTED), case
        if c["rc"] == 0:
            assert [k["n"] for k in c["calls"]] == [1, 2, 3, 65535]
    err = {(c["L"], c["sample_rate"], c["num"], c["den"]): (c["rc"], c["error"]) for c in want["pitch"]}
    assert err[125, 16000, 128, 125] == err[(1 << 24) + 1, 16000, 128, 125] == \
        (-1, "hbk: invalid argument: clip length must be in (125, 2^24]")
    assert err[23040, 16000, 0, 125] == err[23040, 16000, 128, 0] == \
        (-1, "hbk: invalid argument: shift num / den must be positive")
    assert err[23040, 22050, 128, 125] == (-3, "hbk: pitch shift supports 16 kHz (n_fft 250, hop 7), got 22050")
    assert err[23040, 16000, 3, 2][0] == -3 and "3/2 resamples 8000 -> 5333 (8020 taps)" in err[23040, 16000, 3, 2][1]
    assert [(c["n_clips"], c["clips_per_noise"]) for c in want["colored"]] == COLORED_CASES
    assert [c["total"] for c in want["colored"]][:2] == [0, 0]
    assert [(c["n"], c["filters"], c["spectra"], c["blocks"]) for c in want["band_stop"]] == BAND_STOP_CASES
    assert want["table_values_checked"] == 90 + 128 + 11521 + 80 + 100 + 4001


def test_totals_equal_the_loaded_library(table):
    """The two host-only size functions of the library answer what the header's layouts total."""
    from heybuddy._native import lib
    h = lib()
    for c in table["pitch"]:
        for n in (1, 2, 3, 65535):
            want = {k["n"]: k["total"] for k in c.get("calls", [])}.get(n, 0)  # 0: a refused geometry
            assert h.hbk_pitch_shift_workspace_size(n, c["L"], c["sample_rate"], c["num"], c["den"]) == want, (c["L"], n)
    for c in table["colored"]:
        assert h.hbk_colored_noise_workspace_size(c["n_clips"], c["clips_per_noise"]) == c["total"]
