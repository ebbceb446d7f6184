"""tests/golden/mlp_layout_parent.json: what the library answers, through the ABI and
without a GPU, about the classifier's parameter layout and workspace size for the plans of
tests/test_mlp_layout.py. Recorded at the commit before csrc/hbk_mlp_layout.h took the
layout over from hbk_mlp.hip, so that the test holds the header to the former arithmetic.

    python tools/make_mlp_layout_golden.py [--check]

Per plan: n_params, the hbk_mlp_layout offsets, the hbk_mlp_half_layout offsets (half plans)
and hbk_mlp_workspace_size in bytes at each batch size. --check compares with the stored
file instead of writing it.
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hey-buddy_amd"))

PATH = os.path.join(ROOT, "tests", "golden", "mlp_layout_parent.json")
BATCHES = (1, 17, 300, 1100)
# (d_in, layer, hidden, n_layers): the default dims at every depth, a narrow architecture, and
# one in which nothing is a multiple of 4, 16 or 64
DIMS = [(1536, 96, 64, L) for L in range(4)] + [(1536, 32, 24, 1), (40, 8, 5, 0)]
HALF_DIMS = [(1536, 96, 64, 2), (1536, 32, 24, 1)]


def record() -> dict:
    from heybuddy.kernels import MlpPlan
    plans = []
    for gated in (True, False):
        for dims in DIMS:
            p = MlpPlan(*dims, gated=gated, activation="silu" if gated else "relu")
            plans.append({"dims": list(dims), "gated": int(gated), "half": 0, "n_params": p.n_params,
                          "offsets": p.offsets, "workspace_bytes": [p.workspace_bytes(B) for B in BATCHES]})
    for dims in HALF_DIMS:
        p = MlpPlan(*dims, half_layers=True)
        plans.append({"dims": list(dims), "gated": 1, "half": 1, "n_params": p.n_params, "offsets": p.offsets,
                      "half_offsets": p.half_offsets, "workspace_bytes": [p.workspace_bytes(B) for B in BATCHES]})
    return {"batches": list(BATCHES), "plans": plans}


def main() -> None:
    got = record()
    if "--check" in sys.argv:
        with open(PATH) as f:
            want = json.load(f)
        sys.exit(0 if got == want else "the library's layout differs from " + PATH)
    with open(PATH, "w") as f:
        f.write('{"batches": %s,\n"plans": [\n' % json.dumps(got["batches"]))
        f.write(",\n".join(json.dumps(p) for p in got["plans"]))
        f.write("\n]}\n")
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
