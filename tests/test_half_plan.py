"""The half-layer bank's geometry (csrc/hbk_mlp_half_plan.h) on the CPU.

tests/half_plan_check.cpp includes that header alone. It is built here as a stand-alone
program with AddressSanitizer and UBSan and run as a child process: for the default dims and
layer 32 / hidden 24, at B in {1, 17, 130, 1100}, it asserts the offsets, the workspace
regions and the launch grids against arithmetic of its own and prints them. Here the printed
table is compared with the same quantities worked out in Python, and the offsets with what
libhbk.so reports for such plans (hbk_mlp_half_layout, hbk_mlp_workspace_size).
"""
import os
import subprocess

import pytest

from test_step_plan import CSRC, ROOT, _compilers

SRC = os.path.join(ROOT, "tests", "half_plan_check.cpp")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("half_plan") / "half_plan_check")
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
        pytest.fail("no C++ compiler built tests/half_plan_check.cpp with the sanitizers:\n" + "\n".join(errors))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]  # no invariant message, no sanitizer report
    return r.stdout.splitlines()


def _up(n, m):
    return (n + m - 1) // m * m


def _expected(layer, hid, B):
    K, nh = 768, 16
    stride = 2 * K + 2 * hid * K + 2 * hid + layer * hid + layer
    hg = _up(B * nh * 2, 64)
    u = hg + _up(B * nh * 2 * hid, 64)
    dhg = u + _up(B * nh * hid, 64)
    xd = dhg + _up(B * nh * 2 * hid, 64)
    part = xd + _up(B * 1536, 64)
    total = part + _up(nh * B * layer, 64)
    t = lambda n: (n + 63) // 64  # noqa: E731
    tiles = t(nh * hid) * t(layer)
    splits = max(1, min((256 + tiles - 1) // tiles if tiles < 256 else 1, (B + 63) // 64))
    ks = max(64, _up((B + splits - 1) // splits, 64))
    rpb = max(4, (B + 63) // 64)
    return (f"{layer} {hid} {B} | {stride} {16 * stride} | 0 {hg} {u} {dhg} {xd} {part} {total} | hg {t(2 * hid)} {t(B)} 16 "
            f"out {t(layer)} {t(B)} 16 dwo {t(nh * hid)} {t(layer)} {(B + ks - 1) // ks}/{ks} du {t(nh * hid)} {t(B)} "
            f"cs {(B + rpb - 1) // rpb}/{rpb} dwhg {t(K)} {t(2 * hid)} 16")


def test_offsets_workspace_and_grids(table):
    cases = [(96, 64, B) for B in (1, 17, 130, 1100)] + [(32, 24, B) for B in (1, 17, 130, 1100)]
    assert len(table) == len(cases)
    for line, (layer, hid, B) in zip(table, cases):
        assert line == _expected(layer, hid, B)
    assert table[3].split("|")[1].split() == ["106208", str(16 * 106208)]  # the reference's count per branch


def test_library_reports_the_header_layout(table):
    from heybuddy.kernels import MlpPlan
    for layer, hid, layers, base, row in ((96, 64, 2, 256417, 3), (32, 24, 1, 81769, 7)):
        plan = MlpPlan(1536, layer, hid, layers, half_layers=True)
        plain = MlpPlan(1536, layer, hid, layers)
        assert plain.n_params == base
        stride = int(table[row].split("|")[1].split()[0])
        K = 768
        for h, o in enumerate(plan.half_offsets):
            b = base + h * stride
            assert o == [b, b + K, b + 2 * K, b + 2 * K + 2 * hid * K, b + 2 * K + 2 * hid * K + 2 * hid,
                         b + stride - layer], h
        assert plan.n_params == base + 16 * stride
        # the workspace grows by at least the bank's regions (plain fused plans reserve the fused step's)
        bank = int(table[row].split("|")[2].split()[-1]) * 4
        assert plan.workspace_bytes(1100) >= bank
        if not plain.fused:
            assert plan.workspace_bytes(1100) == plain.workspace_bytes(1100) + bank
