"""The generic classifier path's layout and launch geometry (csrc/hbk_mlp_layout.h) on the CPU.

tests/mlp_layout_check.cpp includes that header alone. It is built here as a stand-alone
program with AddressSanitizer and UBSan and run as a child process: for every plan of
tools/make_mlp_layout_golden.py (the default dims at 0..3 layers, layer 32 / hidden 24, and
(40, 8, 5, 0), gated and plain, and two half plans) at B in {1, 17, 300, 1100} it asserts the
parameter blocks, the workspace regions, every GEMM's grid and split and the row / column /
element-wise grids against arithmetic of its own, and prints them. Here the printed table and
what libhbk.so answers through the ABI are both compared with tests/golden/mlp_layout_parent.json,
recorded through the ABI at the commit before the header existed.
"""
import importlib.util
import json
import os
import subprocess

import pytest

from test_step_plan import CSRC, ROOT, _compilers

SRC = os.path.join(ROOT, "tests", "mlp_layout_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mlp_layout_parent.json")
BATCHES = [1, 17, 300, 1100]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["batches"] == BATCHES and len(g["plans"]) == 14
    return g["plans"]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mlp_layout") / "mlp_layout_check")
    errors = []
    for cxx in _compilers():
        is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
               "-I", CSRC, SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            break
        errors.append(f"{' '.join(cmd)}\n{r.stderr}")
    else:
        pytest.fail("no C++ compiler built tests/mlp_layout_check.cpp with the sanitizers:\n" + "\n".join(errors))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]  # no invariant message, no sanitizer report
    params, batch = {}, {}
    for line in r.stdout.splitlines():
        (kind, *key), *rest = [part.split() for part in line.split("|")]
        key = tuple(map(int, key))
        if kind == "params":
            params[key] = (int(rest[0][0]), list(map(int, rest[1])))
        else:
            assert kind == "batch"
            batch[key] = {"total": int(rest[0][0]), "rows": list(map(int, rest[1])), "gemms": rest[2]}
    return params, batch


def _key(plan):
    return (*plan["dims"], plan["gated"], plan["half"])


def _fused(plan):  # hbk_mlp_workspace_size then also reserves the fused step's workspace
    return plan["dims"][:3] == [1536, 96, 64] and plan["dims"][3] <= 2 and plan["gated"] and not plan["half"]


def test_check_program_agrees_with_the_parent(table, golden):
    params, batch = table
    assert len(params) == len(golden) and len(batch) == len(golden) * len(BATCHES)
    generic = 0
    for plan in golden:
        n_params, offsets = params[_key(plan)]
        assert offsets == plan["offsets"], plan["dims"]
        if plan["half"]:  # the bank follows the block the header lays out
            assert plan["half_offsets"][0][0] == n_params
        else:
            assert n_params == plan["n_params"], plan["dims"]
        for B, want in zip(BATCHES, plan["workspace_bytes"]):
            got = batch[(*_key(plan), B)]["total"] * 4
            if _fused(plan):
                assert got <= want
            else:
                assert got == want, (plan["dims"], B)
                generic += 1
    assert generic == (14 - 3) * len(BATCHES)
    assert params[(1536, 96, 64, 2, 1, 0)][0] == 256417 and params[(1536, 96, 64, 2, 0, 0)][0] == 139425


def test_row_grids_and_splits_of_the_trace_cases(table):
    """The three batch sizes the launch geometry was compared at on the GPU."""
    _, batch = table
    plain = (1536, 96, 64, 2, 0, 0)
    assert batch[(*plain, 17)]["rows"] == [5, 1, 4, 5]      # ln, loss, rpb, cs
    assert batch[(*plain, 300)]["rows"] == [75, 2, 4, 75]
    assert batch[(*plain, 1100)]["rows"] == [275, 5, 5, 220]
    splits = lambda B: [int(g.split(":")[1].split(",")[2]) for g in batch[(*plain, B)]["gemms"]]  # noqa: E731
    assert max(splits(17)[2::6] + splits(17)[4::6]) == 1    # K = 17 rows: no split over the batch
    assert min(splits(300)[2::6] + splits(300)[4::6]) > 1   # every weight gradient splits the batch
    half = (1536, 96, 64, 2, 1, 1)
    fwd = [g for i, g in enumerate(batch[(*half, 1100)]["gemms"]) if i % 6 < 2]
    assert all(g.split(":")[1].split(",")[2] == "1" for g in fwd)  # a half plan's forward never splits


def test_library_answers_as_the_parent(golden):
    spec = importlib.util.spec_from_file_location("make_mlp_layout_golden",
                                                  os.path.join(ROOT, "tools", "make_mlp_layout_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    got = tool.record()
    assert got["batches"] == BATCHES
    for g, want in zip(got["plans"], golden):
        assert g == want, want["dims"]
