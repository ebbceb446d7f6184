"""The live-row layouts of tests/test_step_sparse_gpu.py and its child
(tests/step_sparse_worker.py); never collected by pytest. numpy only.

Every layout runs on the "wide" parameters Q of tests/step_oracle_cases.py: the rows named
live come from S (kept by the high-loss filter with margin), every other row from U
(filtered with margin), so n_sel is the number of live rows and the 16-row tiles without a
live row are exactly the tiles k3s must not walk.

K3S_R: the rows per split of the two k3s jobs as compiled for B = 1,100 on a 64-CU stream
(k3s_kernel<5, 12, 2>: 5 and 12 steps of 32 rows).
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

import step_oracle_cases as sc

K3S_R = (160, 384)


def _layout(name, B, live, u, s):
    w = sc.world()
    m = np.zeros(B, bool)
    m[np.asarray(live, np.int64)] = True
    rows = np.empty(B, np.int64)
    rows[~m] = u[:(~m).sum()]
    rows[m] = s[:m.sum()]
    lay = sc.Layout(name, w.Q, rows)
    lay.live = m
    return lay


def _odd_tiles(B):
    r = np.arange(B)
    return r[((r // 16) % 2 == 1) & (r % 3 == 0)]  # dead rows inside the live tiles too


def _check(out):
    for lay in out.values():
        _, stats, _, z = lay.reference()
        assert sc.margins_ok(z, lay.y), lay.name
        assert stats[0] == lay.live.sum(), (lay.name, stats[0], lay.live.sum())
    return out


def _pools(seed):
    w = sc.world()
    U, S = w.classify(w.Q)
    rng = np.random.default_rng(seed)
    return rng, rng.permutation(U), rng.permutation(S)


_layouts = None


def layouts() -> "OrderedDict[str, sc.Layout]":
    """The layouts at the batch sizes where the library itself picks v2 (B >= 800)."""
    global _layouts
    if _layouts is not None:
        return _layouts
    rng, u, s = _pools(47)
    out = OrderedDict()

    def add(name, B, live):
        out[name] = _layout(name, B, live, u, s)

    add("none-1100", 1100, [])
    add("one-front-1100", 1100, [3])
    add("one-tail-1100", 1100, [1099])  # the last, partial tile (rows 1088 .. 1099)
    for n in (32, 33, K3S_R[0], K3S_R[0] + 1, K3S_R[1], K3S_R[1] + 1):
        add(f"first-{n}-1100", 1100, np.arange(n))
    add("odd-tiles-1100", 1100, _odd_tiles(1100))
    add("all-1100", 1100, np.arange(1100))
    add("scattered-800", 800, np.sort(rng.choice(800, 90, replace=False)))
    _layouts = _check(out)
    return out


def forced_layouts() -> "OrderedDict[str, sc.Layout]":
    """The child's layouts below the library's v2 threshold (HBK_STEP=2)."""
    rng, u, s = _pools(48)
    out = OrderedDict()
    out["one-tail-273"] = _layout("one-tail-273", 273, [272], u, s)  # the last, partial tile (row 272 alone)
    out["ends-17"] = _layout("ends-17", 17, [0, 16], u, s)
    out["tail-17"] = _layout("tail-17", 17, [16], u, s)
    return _check(out)
