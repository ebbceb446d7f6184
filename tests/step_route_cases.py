"""Every kernel instantiation and network depth a train-step plan can pick, as data: the
case table of tests/test_step_routes.py (CPU: the table is complete and every forced knob
is honoured by the planner), tests/test_step_routes_gpu.py and tests/step_routes_worker.py
(GPU: each case against the float64 oracle). Never collected by pytest; numpy only. The
candidates, ``Layout`` and the comparisons are those of tests/step_oracle_cases.py.

A case is (name, B, NG, CUs, knobs, layout, where):
  knobs   the HBK_* environment variables the case sets ("HBK_STEP" is latched per process: the
          worker's cases all carry HBK_STEP=2)
  layout  a key of ``layout()``: the rows of a single step; or "forward:<B>" (inference only)
          and "gated" (the six-step gated walk of step_oracle_cases.gated_walk)
  where   "worker": tests/step_routes_worker.py, a child with HBK_STEP=2 on the 64-CU stream;
          "main": the pytest process (no HBK_STEP: the library's own choice of variant)
The plan of a case comes from tests/step_routes_check.cpp (hbk_mlp_plan.h alone); what the
k3s kernel does with it for a layout's live tiles is restated here (``split_bodies``).

Parameter sets: P0 / Q of step_oracle_cases (two layers: NG = 4) and, per depth L = 0, 1
(NG = L + 2), D{L} = omlp.init_params(seed=11 + L, num_layers=L) in f32 and its "wide" version
W{L} (output weight x 120, output bias minus the median candidate logit). Under D{L} every
candidate is selected; under W0 / W1 the 6,000 candidates classify as U (filtered with margin)
1,284 / 1,281 and S (kept with margin) 2,231 / 2,270.
"""
from __future__ import annotations

from collections import OrderedDict, namedtuple

import numpy as np

import step_oracle_cases as sc
from oracle import mlp as omlp

# kK3sPairs of hey-buddy_amd/csrc/hbk_mlp_plan.h: {input layer's, generic jobs'} 32-row steps per split
PAIRS = ((1, 1), (2, 2), (3, 3), (3, 5), (4, 4), (4, 9), (4, 12), (5, 12), (6, 14), (7, 16), (8, 8), (9, 16),
         (12, 12), (16, 16))
# The shorter compiled bodies of a split (k3s_kernel's kA0 kB0 kC0 / kA1 kB1 kC1 in hbk_mlp_fused.hip)
SHORT_IN, SHORT_GEN = (1, 2, 3), (2, 4, 8)
BODIES_IN = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16)
BODIES_GEN = (1, 2, 3, 4, 5, 8, 9, 12, 14, 16)
K1C_RT_MAX = {64: 9, 96: 9, 192: 9, 384: 6}
KS_ALL = (4, 6, 8, 12, 16, 24)
KNOB_DEFAULTS = OrderedDict((("HBK_STEP", 0), ("HBK_K1_KS", 0), ("HBK_K1_KC", 0), ("HBK_K1_RT", 0), ("HBK_K3_R", 0),
                             ("HBK_K3_PAIR", -1), ("HBK_PRE_TILES", 3)))
PER_CALL_KNOBS = ("HBK_K1_KC", "HBK_K1_RT", "HBK_K3_R", "HBK_K3_PAIR", "HBK_PRE_TILES")

Case = namedtuple("Case", "name B NG cus knobs layout where stale")


def split_bodies(n_live, S, nst, short):
    """What k3s_kernel (hbk_mlp_fused.hip) does with a job of S splits and ``nst`` compiled steps
    when the batch has n_live live 16-row tiles: the splits share the list's 32-row steps evenly,
    q = ceil(ceil(n_live / 2) / S) each; split s walks the live tiles [2 s q, min(2 s q + 2 q,
    n_live)), or writes zero slabs when that range is empty; a walking split runs the shortest
    compiled body that holds q steps: the first of ``short`` that is < nst and >= q, else nst.
    Returns (q, body or None when no split walks, walked tiles per split)."""
    q = ((n_live + 1) // 2 + S - 1) // S
    tiles = [max(0, min(2 * s * q + 2 * q, n_live) - 2 * s * q) for s in range(S)]
    body = next((b for b in short if b < nst and q <= b), nst)
    assert q <= nst, (n_live, S, nst)  # S nst 32-row steps hold the batch
    return q, (body if any(tiles) else None), tiles


def all_pair_bodies():
    """Every (pair, job kind, body) k3s_kernel instantiates: 49 input-layer and 44 generic bodies."""
    out = set()
    for p, (nst0, nst1) in enumerate(PAIRS):
        out |= {(p, "in", b) for b in SHORT_IN if b < nst0} | {(p, "in", nst0)}
        out |= {(p, "gen", b) for b in SHORT_GEN if b < nst1} | {(p, "gen", nst1)}
    return out


def k3s_route(plan, n_live):
    """The two job kinds' (q, body, tiles per split) of a v2 plan (a dict of the checker's) at n_live."""
    return {"in": split_bodies(n_live, plan["S0"], plan["NST0"], SHORT_IN),
            "gen": split_bodies(n_live, plan["S1"], plan["NST1"], SHORT_GEN)}


# ------------------------------------------------------------ parameters ----
_depth = {}


def depth_params(L):
    """(D{L}, W{L}): the plain and the wide parameter set of a model with L layers (see above)."""
    if L not in _depth:
        w = sc.world()
        P = OrderedDict((k, v.astype(np.float32)) for k, v in omlp.init_params(seed=11 + L, num_layers=L).items())
        Q = OrderedDict((k, v.copy()) for k, v in P.items())
        Q["mlp_out.output.weight"] = (Q["mlp_out.output.weight"] * np.float32(120.0)).astype(np.float32)
        Q["mlp_out.output.bias"] = np.zeros_like(Q["mlp_out.output.bias"])
        z = omlp.forward(Q, w.x)[1]
        Q["mlp_out.output.bias"] = np.array([-np.median(z)], np.float32)
        _depth[L] = (P, Q)
    return _depth[L]


def param_sets():
    """name -> parameters: every set a layout refers to."""
    w = sc.world()
    out = OrderedDict((("P0", w.P0), ("Q", w.Q)))
    for L in (0, 1):
        out[f"D{L}"], out[f"W{L}"] = depth_params(L)
    return out


def params_name(params):
    return next(k for k, v in param_sets().items() if v is params)


# --------------------------------------------------------------- layouts ----
def live_tiles(lay):
    """The 16-row tiles of a layout that hold a selected row (k3s's live list, by the oracle)."""
    prob = lay.reference()[2]
    sel = np.zeros(lay.B, bool)
    sel[omlp.select_high_loss(prob, lay.y)] = True
    pad = np.zeros((lay.B + 15) // 16 * 16, bool)
    pad[:lay.B] = sel
    return np.flatnonzero(pad.reshape(-1, 16).any(axis=1))


def _compose(name, params, from_u, seed):
    """Rows from U where from_u, from S elsewhere (classified under ``params``)."""
    U, S = sc.world().classify(params)
    rng = np.random.default_rng(seed)
    u, s = rng.permutation(U), rng.permutation(S)
    from_u = np.asarray(from_u, bool)
    assert from_u.sum() <= len(u) and (~from_u).sum() <= len(s), (name, len(u), len(s))
    rows = np.empty(len(from_u), np.int64)
    rows[from_u] = u[:from_u.sum()]
    rows[~from_u] = s[:(~from_u).sum()]
    lay = sc.Layout(name, params, rows)
    lay.n_kept = int((~from_u).sum())
    return lay


def _depth_layout(tag, kind, seed):
    """dense-1100 / sparse-1100 / few-801 / none-800 of step_oracle_cases.layouts() for depth ``tag``'s
    parameter sets (the plain D for dense, the wide W for the rest)."""
    P, Q = depth_params(tag)
    rng = np.random.default_rng(seed)
    if kind == "dense-1100":
        lay = sc.Layout(f"L{tag}/dense-1100", P, sc._take(rng, sc.N_CAND, 1100))
        lay.n_kept = 1100
        return lay
    if kind == "sparse-1100":
        from_u = np.ones(1100, bool)
        from_u[135] = False
        from_u[144:656] = rng.random(512) < 0.5
        from_u[656:1088] = False
    elif kind == "few-801":
        from_u = np.arange(801) < 701
    else:
        assert kind == "none-800"
        from_u = np.ones(800, bool)
    return _compose(f"L{tag}/{kind}", Q, from_u, seed + 1)


_layouts = {}


def layout(key):
    """The single-step layout ``key`` (built once; preconditions asserted by check_layout)."""
    if key in _layouts:
        return _layouts[key]
    w = sc.world()
    kind, _, arg = key.partition("-")
    if key in ("dense-1100", "sparse-1100", "zero-rows-1100", "few-801", "none-800"):
        lay = sc.layouts()[key]
        lay.n_kept = int(lay.reference()[1][0])
    elif key.startswith("L"):  # L<depth>/<kind>
        L = int(key[1])
        lay = _depth_layout(L, key[3:], 70 + 10 * L)
    elif kind == "dense":  # every row selected, rows of any kind
        B = int(arg)
        lay = sc.Layout(key, w.P0, sc._take(np.random.default_rng(500 + B), sc.N_CAND, B))
        lay.n_kept = B
    elif kind == "d0" or kind == "d1":  # the same at depth 0 / 1
        B, L = int(arg), int(kind[1])
        lay = sc.Layout(key, depth_params(L)[0], sc._take(np.random.default_rng(600 + 10 * L + B), sc.N_CAND, B))
        lay.n_kept = B
    elif kind == "none":  # every row filtered: no live tile, every split writes zeros
        lay = _compose(key, w.Q, np.ones(int(arg), bool), 700 + int(arg))
    elif kind == "one" or key == "sparse-32":
        # one live tile: tile 8 (B = 32: tile 1) kept, every other row filtered. Sixteen selected rows, not one: a
        # single row's loss under Q carries its f32 logit error (up to 4e-5 relative) whole, past the 1e-5 bound
        # in the f32 restatement itself; the row seeds are those of 5 tried that leave 4 x on every bound
        B = int(arg)
        from_u = np.ones(B, bool)
        from_u[(16 if B == 32 else 128):(32 if B == 32 else 144)] = False
        lay = _compose(key, w.Q, from_u, {32: 835, 273: 1077, 545: 1347}[B])
    elif key == "sparse-64":  # tile 0 filtered, one live row in tile 1, tile 2 mixed, tile 3 kept: three live tiles
        from_u = np.ones(64, bool)
        from_u[23] = False
        from_u[32:48] = np.random.default_rng(864).random(16) < 0.5
        from_u[48:] = False
        lay = _compose(key, w.Q, from_u, 865)
    elif key == "sparse-273":
        # tiles 0-7 filtered, tile 8 filtered but row 135, tiles 9-13 a 50 / 50 mix, tile 14 kept, tiles 15-16 and
        # the one-row tail tile 17 filtered: seven live tiles
        from_u = np.ones(273, bool)
        from_u[135] = False
        from_u[144:224] = np.random.default_rng(273).random(80) < 0.5
        from_u[224:240] = False
        lay = _compose(key, w.Q, from_u, 281)
    elif key == "sparse-545":
        # the style of sparse-1100: tiles 0-7 filtered (a whole leading split), tile 8 filtered but row 135,
        # tiles 9-19 a 50 / 50 mix, tiles 20-30 kept, tiles 31-33 and the one-row tail tile 34 filtered: 23 live
        from_u = np.ones(545, bool)
        from_u[135] = False
        from_u[144:320] = np.random.default_rng(545).random(176) < 0.5
        from_u[320:496] = False
        lay = _compose(key, w.Q, from_u, 546)
    elif key == "k1c-273":
        # f32 positives and f16 negatives in seeded order, three out-of-range idx (the first block, the middle, the
        # last row: the ragged last block of every RT), dropout 0.1 through omlp.dropout_keep
        rows = sc._take(np.random.default_rng(2273), sc.N_CAND, 273)
        rows[[3, 140, 272]] = -1
        lay = sc.Layout(key, w.P0, rows, bad_idx=(w.n32, 2 ** 31 - 1, -w.n16 - 1), dropout=True)
        lay.n_kept = 273
    else:
        raise KeyError(key)
    _layouts[key] = lay
    return lay


def check_layout(key):
    """The oracle-side preconditions of a layout: the margins of every row, the number of selected
    rows, and (filtered sets) selected logits inside the f32 loss bound. Returns n_sel."""
    lay = layout(key)
    _, stats, _, z = lay.reference()
    assert sc.margins_ok(z, lay.y), key
    assert stats[0] == lay.n_kept, (key, stats[0], lay.n_kept)
    if params_name(lay.params) in ("Q", "W0", "W1"):
        sel = np.abs(z) < -sc.T
        assert (np.abs(z[sel]) <= 6.0).all() and sel.sum() == lay.n_kept, key
    if key == "k1c-273":
        assert (lay.idx >= 0).sum() >= 40 and (lay.idx < 0).sum() >= 150  # both pools
    return int(stats[0])


# ----------------------------------------------------------------- cases ----
# (B of the dense case in which the input-layer job / a generic job runs all its compiled steps), per pair,
# on 64 CUs at NG = 4: derived with the planner (the smallest such B), asserted by test_step_routes.py
DENSE_B = ((1,), (33,), (65,), (129,), (97,), (513,), (353,), (705,), (833,), (961,), (225,), (257, 481), (353,),
           (481,))
# the sparse layouts of a pair: HBK_K3_PAIR = 0 / 1 / 2-3 is honoured up to 32 / 64 / 288 rows only (at most one
# split per 128 rows: k3s_plan). Pairs 0 and 1 therefore always run ONE split, and their zero-slab branch runs
# only when no tile is live (none-*); from pair 2 on, one live tile leaves every later split past the list.
SPARSE_OF_PAIR = (("sparse-32", "none-32"), ("sparse-64", "none-64")) + (("sparse-273", "one-273"),) * 2 + (
    ("sparse-545", "one-545"),) * 10
SHORT_B = (32, 64, 96, 256)
K1C_CASES = tuple((kc, rt) for kc in (64, 96, 192) for rt in (1, 5, 9)) + ((384, 1), (384, 3), (384, 6))
STREAM_WIDTHS = (32, 48, 128)
# test_fused_forward_matches_oracle's batches (tests/test_mlp_fused_gpu.py) and k1b's K splits for them
FORWARD_KS = OrderedDict(((1, 24), (100, 24), (273, 24), (500, 24), (550, 16), (1000, 16), (1100, 12), (2000, 8),
                          (3000, 6), (5000, 4)))
FORWARD_B = tuple(FORWARD_KS)
DEPTH_KINDS = ("dense-1100", "sparse-1100", "few-801", "none-800")
DEPTH_FORCED_B = (1, 17, 129, 273)
PRE_TILES = (1, 2, 3, 4)
WHOLE_GPU = 256


def cases():
    out = []

    def add(name, B, NG, cus, knobs, lay, where, stale=False):
        out.append(Case(name, B, NG, cus, dict(knobs), lay, where, stale))

    v2 = {"HBK_STEP": 2}
    # a. every k3s pair: dense (full-length bodies) and sparse, forced by HBK_K3_PAIR
    for p in range(len(PAIRS)):
        for B in DENSE_B[p]:
            add(f"pair{p}-dense-{B}", B, 4, 64, {**v2, "HBK_K3_PAIR": p}, f"dense-{B}", "worker")
        for key in SPARSE_OF_PAIR[p]:
            add(f"pair{p}-{key}", layout_rows(key), 4, 64, {**v2, "HBK_K3_PAIR": p}, key, "worker")
    # ... the shorter compiled bodies of every pair (k3s_body<.., 1 / 2 / 3> and <.., 2 / 4 / 8> are instantiated per
    # pair): dense batches of 1, 2, 3 and 8 32-row steps, where the pair is honoured and not already full-length
    for p, (nst0, nst1) in enumerate(PAIRS):
        for B in SHORT_B:
            if B <= (32, 64)[p] if p < 2 else B // 32 < max(nst0, nst1):
                add(f"pair{p}-dense-{B}", B, 4, 64, {**v2, "HBK_K3_PAIR": p}, f"dense-{B}", "worker")
    # ... pairs 12 and 13 also by HBK_K3_R (the first pair whose input-layer split has >= R rows)
    add("k3r384-dense-353", 353, 4, 64, {**v2, "HBK_K3_R": 384}, "dense-353", "worker")
    add("k3r512-sparse-545", 545, 4, 64, {**v2, "HBK_K3_R": 512}, "sparse-545", "worker")
    # ... and one sparse case per job kind's longest bodies from a workspace of 0xFF bytes
    add("pair3-sparse-273-stale", 273, 4, 64, {**v2, "HBK_K3_PAIR": 3}, "sparse-273", "worker", True)
    add("pair9-sparse-545-stale", 545, 4, 64, {**v2, "HBK_K3_PAIR": 9}, "sparse-545", "worker", True)
    # b. k1c: every K chunk at its first, a middle and its last row-tile count
    for kc, rt in K1C_CASES:
        add(f"k1c-{kc}-{rt}", 273, 4, 64, {**v2, "HBK_K1_KC": kc, "HBK_K1_RT": rt}, "k1c-273", "worker")
    add("k1c-384-6-zero-rows-1100", 1100, 4, 64, {**v2, "HBK_K1_KC": 384, "HBK_K1_RT": 6}, "zero-rows-1100", "worker")
    # c. stream widths: the library's own plans
    for n in STREAM_WIDTHS:
        for key in ("dense-1100", "sparse-1100"):
            add(f"width{n}-{key}", 1100, 4, n, {}, key, "main")
    # d. depth: v1 on the whole GPU, v2 on 64 CUs (the library's choice from 800 rows), forced v2 below
    for L in (0, 1):
        for kind in DEPTH_KINDS:
            B = int(kind.split("-")[1])
            add(f"L{L}-v1-{kind}", B, L + 2, WHOLE_GPU, {}, f"L{L}/{kind}", "main")
            add(f"L{L}-v2-{kind}", B, L + 2, 64, {}, f"L{L}/{kind}", "main")
        for B in DEPTH_FORCED_B:
            add(f"L{L}-forced-{B}", B, L + 2, 64, v2, f"d{L}-{B}", "worker")
        add(f"L{L}-v1-gated", sc.GATED_B, L + 2, WHOLE_GPU, {}, "gated", "main")
        add(f"L{L}-v2-gated", sc.GATED_B, L + 2, 64, {}, "gated", "main")
    add("L2-v1-dense-1100", 1100, 4, WHOLE_GPU, {}, "dense-1100", "main")  # (test_train_step_oracle_gpu.py's)
    add("L2-v2-dense-1100", 1100, 4, 64, {}, "dense-1100", "main")
    # e. HBK_PRE_TILES: the gated walk on v2 (3 is the default: test_train_step_oracle_gpu.py's run)
    for n in PRE_TILES:
        add(f"pre{n}-gated", sc.GATED_B, 4, 64, {"HBK_PRE_TILES": n}, "gated", "main")
    # f. k1b: the inference batches on the whole GPU
    for B in FORWARD_B:
        add(f"forward-{B}", B, 4, WHOLE_GPU, {}, f"forward:{B}", "main")
    assert len({c.name for c in out}) == len(out)
    return out


_walks = {}


def gated_walk(L, dtype=np.float64, plan=None):
    """step_oracle_cases.gated_walk from the wide parameters W{L} of depth L (the float64 walk is kept)."""
    start = depth_params(L)[1]
    if dtype is not np.float64 or plan is not None:
        return sc.gated_walk(dtype, plan, start=start)
    if L not in _walks:
        _walks[L] = sc.gated_walk(start=start)
    return _walks[L]


def layout_rows(key):
    return int(key.rsplit("-", 1)[1])


def case_line(c):
    """The case as tests/step_routes_check.cpp reads it."""
    kn = dict(KNOB_DEFAULTS)
    assert set(c.knobs) <= set(kn), c.name
    kn.update(c.knobs)
    return " ".join([c.name, str(c.B), str(c.NG), str(c.cus)] + [str(v) for v in kn.values()])


def is_step(c):
    """A single train step on a layout (not the inference batches, not the gated walk)."""
    return c.layout != "gated" and not c.layout.startswith("forward:")
