"""The mel unit's host logic (csrc/hbk_mel_plan.h) on the CPU.

tests/mel_plan_check.cpp includes that header alone. It is built here as a
stand-alone program with AddressSanitizer and UBSan and run as a child process
on a file of raw f32 written here: the windows W0-W2 and the banks B0-B5 and M2
of tests/test_mel_routes.py. For every window, bank and knob set it builds the
plan's tables, asserts their invariants (the table buffer's regions; both filter
layouts against the filterbank; the twiddles against the formula; the SoA
table's rows against the tables they are built from) and prints status, scalars,
routes, offsets, start bins and table hashes; then the refusals of
hbk_mel_plan_create, the argument checks of hbk_mel_frames and the launch grid
of every route. The output must equal, exactly, the table recorded from the
tree before the host block was moved out of hbk_mel.hip
(tests/golden/mel_plan_parent.json; DESIGN.md says how it was made).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import test_mel_routes as R
from test_step_plan import _compilers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hey-buddy_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "mel_plan_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mel_plan_parent.json")

KNOBS = {"none": {}, "V1": {"HBK_MEL_V1": "1"}, "MFMA": {"HBK_MEL_MFMA": "1"}, "V4=1": {"HBK_MEL_V4": "1"},
         "V4=8": {"HBK_MEL_V4": "8"}, "V4=0": {"HBK_MEL_V4": "0"}}
ARG = "hbk: invalid argument: "
REFUSALS = [("window NULL", R.HBK_ERR_ARG, ARG + "window/fbank is NULL"),
            ("fbank NULL", R.HBK_ERR_ARG, ARG + "window/fbank is NULL"),
            ("n_fft 256", R.HBK_ERR_ARG, ARG + "n_fft must be 512"),
            ("hop 0", R.HBK_ERR_ARG, ARG + "hop must be positive"),
            ("hop -160", R.HBK_ERR_ARG, ARG + "hop must be positive"),
            ("n_mels 0", R.HBK_ERR_ARG, ARG + "n_mels must be even and <= 32"),
            ("n_mels 34", R.HBK_ERR_ARG, ARG + "n_mels must be even and <= 32"),
            ("n_mels 3", R.HBK_ERR_ARG, ARG + "n_mels must be even and <= 32"),
            ("out_div 0", R.HBK_ERR_ARG, ARG + "out_div must be non-zero"),
            ("17 taps", R.HBK_ERR_UNSUPPORTED, "hbk: mel filter spans 17 bins (> 16 supported)")]
CALL_REFUSALS = {"n_clips -1": "negative size", "n_frames -1": "negative size", "pcm NULL": "pcm/out is NULL",
                 "out NULL": "pcm/out is NULL", "odd stride": "clip_stride and hop must be even (float2 loads)",
                 "odd hop": "clip_stride and hop must be even (float2 loads)",
                 "pcm + 4": "pcm/out must be 8-byte aligned", "out + 4": "pcm/out must be 8-byte aligned",
                 "one frame too many": "frames exceed clip_stride", "2^31 frames": "more than 2^31 frames in one call"}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mel_plan") / "mel_plan_check")
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
    pytest.fail("no C++ compiler built tests/mel_plan_check.cpp with the sanitizers:\n" + "\n".join(errors))


@pytest.fixture(scope="module")
def table(checker, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mel_plan_in") / "inputs.f32")
    with open(path, "wb") as f:
        for name in R.WINDOWS:
            f.write(np.ascontiguousarray(R.window(name), dtype=np.float32).tobytes())
        for name in R.BANKS:
            f.write(np.ascontiguousarray(R.bank(name), dtype=np.float32).tobytes())
    env = {k: v for k, v in os.environ.items() if not k.startswith("HBK_")}
    r = subprocess.run([checker, path], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]  # no invariant message, no sanitizer report
    return json.loads(r.stdout)


def test_tables_hold_their_invariants_and_equal_the_recorded_table(table):
    want = json.load(open(GOLDEN))
    assert table.keys() == want.keys()
    for key in want:
        assert len(table[key]) == len(want[key]), key
        for g, w in zip(table[key], want[key]):
            assert g == w, (key, w.get("case", w.get("route")))
    # what the table must hold: every window x bank x knob set, in order; the launch grids of every route
    assert [c["case"] for c in want["plans"]] == [f"W{w} {b} {k}" for w in range(3) for b in R.BANKS for k in KNOBS]
    assert [c["route"] for c in want["launches"]] == [1, 2, 3, 4, 8]
    assert all(len(c["grids"]) == 6 * 3 for c in want["launches"])
    grids = {c["route"]: c["grids"] for c in want["launches"]}
    # 1,833 frames on 4, 64 and 256 CUs, the default route: 58 groups of 32 on at most 2 blocks per CU
    assert grids[2][12:15] == [[32, 58, 8, 512], [32, 58, 58, 512], [32, 58, 58, 512]]
    assert grids[8][17] == [64, 1 << 25, 512, 512]  # 2^31 - 1 frames, 256 CUs: two 8-wave blocks per CU


def test_routes_equal_the_restated_rule(table):
    """For every bank and knob set, the header's route and scalars are route_on_host's."""
    plans = {c["case"]: c for c in table["plans"]}
    for wi, wname in enumerate(R.WINDOWS):
        for bname in R.BANKS:
            for kname, env in KNOBS.items():
                c = plans[f"W{wi} {bname} {kname}"]
                host = R.route_on_host(R.bank(bname), env)
                assert c["rc"] == 0 and c["error"] == "", c["case"]
                # route: [variant 0, variant 1]; HBK_MEL_MFMA only sets the variant a v2 plan starts on
                assert c["route"] == [host["kernel"], 3 if host["kernel"] != 1 else 1], c["case"]
                assert c["variant"] == int(kname == "MFMA" and host["kernel"] != 1), c["case"]
                assert (c["taps"], c["nk2"], c["need256"]) == (host["taps"], host["nk2"], host["need256"]), c["case"]
                assert len(c["lo"]) == host["n_mels"]
                assert c["edge0"] == int(host["kernel"] != 1 and R.window_edge0(R.window(wname))), c["case"]
            assert plans[f"W{wi} {bname} none"]["route"][0] == R.EXPECTED_ROUTE[bname][0]


def test_refusals_carry_their_codes_and_texts(table):
    assert [(c["case"], c["rc"], c["error"]) for c in table["refusals"]] == REFUSALS
    calls = {c["case"]: c for c in table["calls"]}
    for case, c in calls.items():
        if case in CALL_REFUSALS:
            assert (c["rc"], c["error"], c["total"]) == (R.HBK_ERR_ARG, ARG + CALL_REFUSALS[case], 0), case
        else:
            assert c["rc"] == 0 and c["error"] == "", case
    assert set(CALL_REFUSALS) < set(calls)
    assert calls["13 x 141"]["total"] == 1833 and calls["frames fit"]["total"] == 8
    assert calls["n_clips 0, pcm NULL"]["total"] == calls["n_frames 0"]["total"] == 0
