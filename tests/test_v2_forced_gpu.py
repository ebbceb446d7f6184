"""The v2 train step (k1s / k1c / k2 / k3s) forced at the batch sizes where the library picks
v1 (HBK_STEP=2, read once per process: one fresh child, tests/v2_forced_worker.py, on the
64-CU train stream), so that v2 is pinned to the float64 oracle and to the reference's own
fixtures, not only to v1:

* single steps at B = 1, 15, 16, 17, 33, 129, 273, 550 (dense rows on the golden parameters)
  and a sparse layout at B = 273 (the first 128 rows filtered, the rest mixed, on the "wide"
  parameters of tests/step_oracle_cases.py) against oracle.mlp.flat_bucket, with the bounds
  of tests/test_train_step_oracle_gpu.py;
* the B = 96 step of tests/golden/classifier.npz, the 24-step train_epoch (batches of 8 to 300
  rows: the gate skips and fires) and the 3-stage WakeWordTrainer.__call__ of
  classifier_stages.npz, each with exactly the bounds of its v1 test
  (test_fused_grads_match_reference, test_train_epoch_matches_reference,
  test_three_stage_training_matches_reference: the same helper functions).
The child asserts step_variant == 2 at every batch size it runs.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import step_oracle_cases as sc
from oracle import golden_classifier as gc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "v2_forced_worker.py")
FORCED_B = (1, 15, 16, 17, 33, 129, 273, 550)


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("v2_forced") / "out.npz")
    pr = subprocess.Popen([sys.executable, WORKER, out], env=dict(os.environ, HBK_STEP="2"), cwd=ROOT,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        log, _ = pr.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        pr.kill()
        pr.communicate()
        raise
    assert pr.returncode == 0, log[-4000:]
    return np.load(out)


@pytest.fixture(scope="module")
def layouts():
    return sc.forced_layouts()


def _grads(forced, tag, params):
    return {k: forced[f"{tag}/g/{k}"] for k in params}


def test_v2_ran_at_every_batch_size(forced):
    ran = set(int(b) for b in forced["batches"])
    assert set(FORCED_B) | {96, 1100} | set(gc.EPOCH_SIZES) <= ran, sorted(ran)


@pytest.mark.parametrize("name", [f"dense-{B}" for B in FORCED_B] + ["sparse-273"])
def test_forced_v2_step_matches_oracle(name, forced, layouts):
    lay = layouts[name]
    tag = f"step/{name}"
    sc.check_bucket(lay, _grads(forced, tag, lay.params), forced[f"{tag}/stats"], forced[f"{tag}/prob"])


def test_forced_v2_step_matches_reference(forced):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "classifier.npz"))
    params = gc.golden_inputs()[0]
    n_sel = int(gold["n_sel"])
    sc.check_step_against_gold(gold, params, forced["b96/stats"], forced["b96/prob"],
                               {k: v / n_sel for k, v in _grads(forced, "b96", params).items()})


def test_forced_v2_train_epoch_matches_reference(forced):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "classifier.npz"))
    params = gc.golden_inputs()[0]
    e = {k: forced[f"epoch/{k}"] for k in ("lr", "hlr", "loss", "rec", "fp")}
    sc.check_epoch_against_gold(gold, params, e["lr"], e["hlr"], e["loss"], e["rec"], e["fp"],
                                {k: forced[f"epoch/final/{k}"] for k in params})


def test_forced_v2_three_stage_training_matches_reference(forced):
    from test_stages_gpu import STAGE_HISTORIES
    gold = np.load(os.path.join(ROOT, "tests", "golden", "classifier_stages.npz"))
    params = gc.golden_inputs()[0]
    sc.check_stages_against_gold(gold, params, {k: forced[f"stages/{k}"] for k in STAGE_HISTORIES},
                                 forced["stages/sizes"], {k: forced[f"stages/final/{k}"] for k in params})
