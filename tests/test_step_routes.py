"""The train step's route table (tests/step_route_cases.py) on the CPU: it is complete, every
forced knob is honoured by the planner, and every oracle-side precondition of its layouts holds.

tests/step_routes_check.cpp includes csrc/hbk_mlp_plan.h alone, reads the cases from stdin and
prints plan_step()'s plan for each; it is built here exactly as tests/test_step_plan.py builds
its checker (AddressSanitizer and UBSan, static runtimes, a child process). The kernel's split
rule (which compiled body a split runs for the live tiles of a layout) is restated in
step_route_cases.split_bodies; the live tiles come from the float64 oracle.

Complete means: all 14 k3s pairs; per pair a dense case in which the input-layer job runs all
NST0 steps and one in which a generic job runs all NST1; every body length of either job kind,
and in fact every (pair, job kind, body) the dispatch instantiates (93 k3s_body<> in all);
per pair a sparse case with an odd number of live tiles (a half-filled last step) and a case
with a split past the live list (the zero-slab branch); k1c's four K chunks at RT 1, a middle
RT and the maximum; k1b's six K splits; depths 0, 1 and 2 under v1 and v2; pre_tiles 1 to 4.
The sets are asserted equal to the full ones, so removing any of these from the table fails.

HBK_K3_PAIR = 0 / 1 is honoured only while the batch has one split (k3s_plan: at most one
split per 128 rows), so for pairs 0 and 1 the zero-slab branch runs only when no tile is live:
their "split past the list" case is none-32 / none-64, and their odd-live case is a separate
one. From pair 2 on the one-<B> layouts (one live tile) are both at once, and sparse-273 /
sparse-545 add the half-filled last step of a longer list.
"""
import json
import os
import subprocess

import pytest

import step_route_cases as rc
from test_step_plan import CSRC, ROOT, _compilers

SRC = os.path.join(ROOT, "tests", "step_routes_check.cpp")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_routes") / "step_routes_check")
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
    pytest.fail("no C++ compiler built tests/step_routes_check.cpp with the sanitizers:\n" + "\n".join(errors))


def run_checker(exe, cases):
    """name -> plan (the fields of hbk_mlp_step_plan_info) for every case."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("HBK_")}  # (the knobs come from the case lines)
    r = subprocess.run([exe], input="\n".join(rc.case_line(c) for c in cases) + "\n", capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    plans = {p["name"]: p for p in json.loads(r.stdout)}
    assert list(plans) == [c.name for c in cases]
    return plans


@pytest.fixture(scope="module")
def table(checker):
    cases = rc.cases()
    return cases, run_checker(checker, cases)


def coverage(cases, plans):
    """What the table reaches, from the planner's plans and the oracle's live tiles."""
    cov = {"pairs": set(), "full_in": set(), "full_gen": set(), "body_in": set(), "body_gen": set(), "odd": set(),
           "zero_slab": set(), "k1c": set(), "ks": set(), "depth": set(), "pre": set(), "pair_bodies": set()}
    for c in cases:
        pl = plans[c.name]
        cov["ks"].add(pl["KS"])
        cov["depth"].add((pl["NG"], pl["variant"]))
        if pl["variant"] != 2:
            continue
        cov["pre"].add(pl["pre_tiles"])
        if not rc.is_step(c):
            continue
        cov["k1c"].add((pl["KC"], pl["RT"]))
        p = pl["k3s_pair"]
        cov["pairs"].add(p)
        n_live = len(rc.live_tiles(rc.layout(c.layout)))
        route = rc.k3s_route(pl, n_live)
        for kind, nst in (("in", pl["NST0"]), ("gen", pl["NST1"])):
            q, body, tiles = route[kind]
            if body is not None:
                cov[f"body_{kind}"].add(body)
                cov["pair_bodies"].add((p, kind, body))
            if n_live == pl["rt"] and q == nst == body:  # dense: every tile live, a split of all nst steps
                cov[f"full_{kind}"].add(p)
        if n_live < pl["rt"] and n_live % 2 == 1 and all(any(t % 2 for t in route[k][2]) for k in route):
            cov["odd"].add(p)  # (sparse) the last walked step of either job kind holds one tile
        if n_live < pl["rt"] and all(0 in route[k][2] for k in route):
            cov["zero_slab"].add(p)  # a split of either job kind past the live list
    return cov


def test_the_table_is_complete(table):
    cases, plans = table
    cov = coverage(cases, plans)
    every = set(range(len(rc.PAIRS)))
    assert cov["pairs"] == every
    assert cov["full_in"] == every and cov["full_gen"] == every
    assert cov["body_in"] == set(rc.BODIES_IN) == {p[0] for p in rc.PAIRS} | set(rc.SHORT_IN)
    assert cov["body_gen"] == set(rc.BODIES_GEN) == {p[1] for p in rc.PAIRS} | {1, 2, 4, 8}
    assert cov["odd"] == every and cov["zero_slab"] == every
    assert cov["pair_bodies"] == rc.all_pair_bodies() and len(cov["pair_bodies"]) == 49 + 44  # every k3s_body<>
    for kc, rt_max in rc.K1C_RT_MAX.items():
        rts = {rt for k, rt in cov["k1c"] if k == kc}
        assert 1 in rts and rt_max in rts and any(1 < rt < rt_max for rt in rts), (kc, rts)
        assert max(rts) == rt_max
    assert cov["ks"] >= set(rc.KS_ALL)
    forward = {c.B: plans[c.name] for c in cases if c.layout.startswith("forward:")}
    assert {B: pl["KS"] for B, pl in forward.items()} == dict(rc.FORWARD_KS)  # (what the GPU test asserts per batch)
    assert set(rc.FORWARD_KS.values()) == set(rc.KS_ALL) and all(pl["variant"] == 1 for pl in forward.values())
    assert cov["depth"] == {(ng, v) for ng in (2, 3, 4) for v in (1, 2)}
    assert cov["pre"] >= {1, 2, 3, 4}
    print(f"{len(cases)} cases; (pair, job kind, body) instantiations reached: {len(cov['pair_bodies'])}")


def test_every_forced_knob_is_honoured(table):
    """The plan the checker prints takes what the case forces: a pair the planner would silently replace (its
    splits past the workspace's slabs) fails here, before any GPU run."""
    cases, plans = table
    for c in cases:
        pl, kn = plans[c.name], c.knobs
        assert (pl["NG"], pl["cus"]) == (c.NG, c.cus) and pl["Bp"] == (c.B + 15) // 16 * 16
        if "HBK_STEP" in kn:
            assert pl["variant"] == kn["HBK_STEP"], c.name
        if "HBK_K3_PAIR" in kn:
            assert pl["k3s_pair"] == kn["HBK_K3_PAIR"], c.name
            assert (pl["NST0"], pl["NST1"]) == rc.PAIRS[kn["HBK_K3_PAIR"]], c.name
        if "HBK_K3_R" in kn:  # the first pair whose input-layer split has >= R rows
            first = next(q for q, p in enumerate(rc.PAIRS) if 32 * p[0] >= kn["HBK_K3_R"])
            assert pl["k3s_pair"] == first, c.name
        if "HBK_K1_KC" in kn:
            assert (pl["KC"], pl["KS"]) == (kn["HBK_K1_KC"], 1536 // kn["HBK_K1_KC"]), c.name
        if "HBK_K1_RT" in kn:
            assert pl["RT"] == kn["HBK_K1_RT"] <= rc.K1C_RT_MAX[pl["KC"]], c.name
        if "HBK_PRE_TILES" in kn:
            assert pl["variant"] == 2 and pl["pre_tiles"] == kn["HBK_PRE_TILES"], c.name
        if c.where == "worker":
            assert kn.get("HBK_STEP") == 2 and c.cus == 64, c.name
        else:  # the main process latches no knob: only per-call ones
            assert set(kn) <= set(rc.PER_CALL_KNOBS), c.name
        if pl["variant"] == 2:
            assert pl["sparse"] == 1 and pl["S1"] <= pl["S0"] == pl["slabs"], c.name
    # the default plans of narrower train streams ("split:48", "split:32"): kernels no other test runs
    assert (plans["width48-dense-1100"]["KC"], plans["width48-dense-1100"]["RT"]) == (384, 6)
    assert plans["width48-dense-1100"]["k3s_pair"] == 11
    assert (plans["width32-dense-1100"]["k3s_pair"], plans["width32-dense-1100"]["RT"]) == (7, 9)


def test_layout_preconditions_hold_on_the_oracle(table):
    """Margins, n_sel and the parameter sets' classes, on the oracle alone; and the dense batch sizes of
    step_route_cases.DENSE_B are the smallest at which the pair's job runs all its compiled steps."""
    cases, plans = table
    w = rc.sc.world()
    for L, (n_u, n_s) in ((0, (1284, 2231)), (1, (1281, 2270))):
        D, W = rc.depth_params(L)
        U, S = w.classify(W)
        assert (len(U), len(S)) == (n_u, n_s)
        prob = rc.omlp.forward(D, w.x)[0]
        assert len(rc.omlp.select_high_loss(prob, w.y)) == rc.sc.N_CAND  # the plain model selects every row
        assert sum(1 for k in D if k.endswith(".0.weight")) == L
    seen = {}
    for c in cases:
        if rc.is_step(c):
            assert rc.layout(c.layout).B == c.B, c.name
            if c.layout not in seen:
                seen[c.layout] = rc.check_layout(c.layout)
            sets = {2: ("D0", "W0"), 3: ("D1", "W1"), 4: ("P0", "Q")}[c.NG]  # the case's depth is its parameters'
            assert rc.params_name(rc.layout(c.layout).params) in sets
    assert seen["none-32"] == seen["none-64"] == seen["L0/none-800"] == seen["L1/none-800"] == 0
    assert seen["sparse-32"] == seen["one-273"] == seen["one-545"] == 16  # one whole tile
    for key in ("sparse-32", "one-273", "one-545"):
        assert len(rc.live_tiles(rc.layout(key))) == 1
    assert seen["L0/few-801"] == seen["L1/few-801"] == 100
    lay = rc.layout("k1c-273")
    assert lay.dropout and list(lay.idx[[3, 140, 272]]) == [w.n32, 2 ** 31 - 1, -w.n16 - 1]
    assert not lay.x[[3, 140, 272]].any() and 273 % (16 * 9) != 0  # zero rows; a ragged last block


def test_dense_batch_sizes_are_the_smallest(checker):
    """DENSE_B re-derived with the planner: per pair, the smallest B (64 CUs, NG 4, the pair forced and
    honoured, every tile live) at which the input-layer job / a generic job runs all its compiled steps."""
    cases = [rc.Case(f"p{p}-{B}", B, 4, 64, {"HBK_STEP": 2, "HBK_K3_PAIR": p}, "", "worker", False)
             for p in range(len(rc.PAIRS)) for B in range(1, 1101, 16)]
    plans = run_checker(checker, cases)
    for p, (nst0, nst1) in enumerate(rc.PAIRS):
        first = {}
        for c in cases:
            pl = plans[c.name]
            if c.knobs["HBK_K3_PAIR"] != p or pl["k3s_pair"] != p:
                continue
            route = rc.k3s_route(pl, pl["rt"])
            for kind, nst in (("in", nst0), ("gen", nst1)):
                if route[kind][0] == nst == route[kind][1]:
                    first.setdefault(kind, c.B)
            if route["in"][0] == nst0 and route["gen"][0] == nst1:
                first.setdefault("both", c.B)
        want = (first["both"],) if "both" in first else (first["in"], first["gen"])
        assert rc.DENSE_B[p] == want, (p, first)


def test_gated_walks_fire_and_skip(table):
    """The depth models' six-step walks on the oracle: the composed n_sel, two skips, a fire, an empty step
    (asserted inside gated_walk) from the wide parameters of either depth."""
    for L in (0, 1):
        g = rc.gated_walk(L)
        assert list(g["hist"][:, 0]) == list(rc.sc.GATED_NSEL) and list(g["hist"][:, 2]) == [0, 0, 1, 0, 1, 0]
