"""The embedding planner (csrc/hbk_embed_plan.h) on the CPU.

tests/embed_plan_check.cpp includes that header alone. It is built here as a
stand-alone program with AddressSanitizer and UBSan and run as a child process
on graph files written here: SE20 with the reference's window starts, the
generic and the wide graph of tests/test_embed.py, and five graphs that must be
refused. For both precisions and the knob sets of its case list it asserts the
plan's invariants (LDS regions ascending, aligned and inside 160 KB; table
offsets inside their blob; gather indices below n_src; workspace buffers that
hold every chain's output; positive task counts) and prints every plan: kernel
values, the scalar fields of the argument structs, launch geometry and a hash
of each packed blob. The output must equal, exactly, the table recorded from the
tree before the planner was split out of hbk_embed.hip (then the stack's one unit)
(tests/golden/embed_plan_parent.json; DESIGN.md says how it was made).
"""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from test_step_plan import _compilers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hey-buddy_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "embed_plan_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "embed_plan_parent.json")


def _conv(kh, kw, cin, cout, w, b, act=1, alpha=0.2):
    return (0, kh, kw, cin, cout, act, float(alpha), np.asarray(w, np.float32).ravel(), np.asarray(b, np.float32))


def _pool(ph, pw):
    return (1, ph, pw, 0, 0, 0, 0.0, np.zeros(0, np.float32), np.zeros(0, np.float32))


def _ops_of(graph):
    from heybuddy.embedding_graph import Conv
    return [_conv(o.kh, o.kw, o.cin, o.cout, o.weight, o.bias, 1 if o.act == "leaky_relu" else 0, o.alpha)
            if isinstance(o, Conv) else _pool(o.ph, o.pw) for o in graph.ops]


def _rand_conv(rng, kh, kw, cin, cout, act=1):
    w = rng.standard_normal((kh, kw, cin, cout)) * np.sqrt(2.0 / (kh * kw * cin))
    return _conv(kh, kw, cin, cout, w, rng.standard_normal(cout) * 0.1, act)


def _write(path, in_h, in_w, starts, ops):
    with open(path, "wb") as f:
        f.write(struct.pack(f"<4i{len(starts)}i", in_h, in_w, len(starts), len(ops), *starts))
        for kind, kh, kw, cin, cout, act, alpha, w, b in ops:
            f.write(struct.pack("<8if", kind, kh, kw, cin, cout, act, w.size, b.size, alpha))
            f.write(w.astype("<f4").tobytes())
            f.write(b.astype("<f4").tobytes())


def graph_files(folder):
    """The graphs of the table, in its order: (file, in_h, in_w, starts, ops)."""
    import test_embed as E
    from heybuddy.embedding_graph import WINDOW_STARTS, se20_graph
    se20, rng = _ops_of(se20_graph()), np.random.default_rng(31)
    big = list(se20)
    w = big[0][7].copy()
    w[0] = 7e4  # outside the split-f16 range: refused in split, planned in exact
    big[0] = big[0][:7] + (w,) + big[0][8:]
    cases = [
        ("se20", 76, 32, WINDOW_STARTS, se20),
        ("generic", 20, 12, (0,), _ops_of(E._generic_graph())),
        ("wide", 20, 12, (0,), _ops_of(E._wide_graph())),
        # a conv whose cin is not its input's channel count
        ("bad_channels", 20, 12, (0,), [_rand_conv(rng, 2, 3, 1, 12), _rand_conv(rng, 1, 1, 13, 40), _pool(2, 2),
                                        _rand_conv(rng, 9, 5, 40, 33, 0)]),
        # a kernel taller than what is left of the window
        ("bad_collapse", 20, 12, (0,), [_rand_conv(rng, 2, 3, 1, 12), _rand_conv(rng, 25, 1, 12, 8), _pool(2, 2),
                                        _rand_conv(rng, 1, 5, 8, 33, 0)]),
        ("bad_weight", 76, 32, WINDOW_STARTS, big),
        # a pool followed by a pool
        ("bad_pool", 20, 12, (0,), [_rand_conv(rng, 2, 3, 1, 12), _pool(2, 1), _pool(1, 2), _rand_conv(rng, 3, 2, 12, 8),
                                    _pool(1, 2), _rand_conv(rng, 7, 2, 8, 33, 0)]),
        # one output row of 598 positions x 64 channels: more than a CU's LDS in either precision
        ("bad_lds", 4, 600, (0,), [_rand_conv(rng, 2, 3, 1, 64), _rand_conv(rng, 1, 3, 64, 64), _pool(3, 596),
                                   _rand_conv(rng, 1, 1, 64, 8, 0)]),
    ]
    paths = []
    for name, in_h, in_w, starts, ops in cases:
        paths.append(os.path.join(folder, name + ".bin"))
        _write(paths[-1], in_h, in_w, tuple(starts), ops)
    return paths


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("embed_plan") / "embed_plan_check")
    errors = []
    for cxx in _compilers():
        # (static sanitizer runtimes, as tests/test_step_plan.py; the header needs _Float16: clang, or gcc >= 13)
        is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", *static, "-I", CSRC, SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{' '.join(cmd)}\n{r.stderr}")
    pytest.fail("no C++ compiler built tests/embed_plan_check.cpp with the sanitizers:\n" + "\n".join(errors))


def test_plans_hold_their_invariants_and_equal_the_recorded_table(checker, tmp_path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HBK_")}
    r = subprocess.run([checker, *graph_files(str(tmp_path))], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]  # no invariant message, no sanitizer report
    got, want = json.loads(r.stdout)["cases"], json.load(open(GOLDEN))["cases"]
    assert [(c["graph"], c["precision"], c["knobs"]) for c in got] == \
        [(c["graph"], c["precision"], c["knobs"]) for c in want]
    assert len(got) == 13 + 6 + 6 + 5 * 2  # se20, generic, wide, the refused graphs (embed_plan_check.cpp for_each_case)
    for g, w in zip(got, want):
        where = (w["graph"], w["precision"], w["knobs"])
        assert g.keys() == w.keys(), where
        for key in w:
            assert g[key] == w[key], (where, key)
    # what the table must hold: every pattern kernel, both generic ones, and the five refusals
    kernels = {c[k]["kernel"].split("/")[0] for case in want for prog in ("clip", "win") if prog in case
               for c in case[prog]["chains"] for k in ("base", "pattern") if k in c}
    assert kernels == {"exact", "x3", "p0", "p0s", "p1", "p1s", "p2s", "t3s"}
    refused = {(c["graph"], c["precision"]): c["error"] for c in want if c["rc"]}
    assert set(refused) == {(g, p) for g in ("bad_channels", "bad_collapse", "bad_pool", "bad_lds")
                            for p in ("split", "exact")} | {("bad_weight", "split")}
    assert "bad conv op" in refused["bad_channels", "split"] and "collapses" in refused["bad_collapse", "exact"]
    assert "65504" in refused["bad_weight", "split"] and "followed by a conv" in refused["bad_pool", "split"]
    assert "does not fit in LDS" in refused["bad_lds", "split"] and "does not fit in LDS" in refused["bad_lds", "exact"]
