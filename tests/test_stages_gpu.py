"""WakeWordTrainer.__call__ (3 stages, reference trainer.py:764-1007) on the
HIP path against the reference's own run (tests/golden/classifier_stages.npz,
oracle/golden_classifier.py:make_stages): batch sizes 1100 -> 550 -> 273
(training.py:215-231), LR x 0.5 and steps x 2 per stage, validation every 4
steps with the dynamic negative weight (x2 while the validation false-positive
rate is above 1.5 / hour) and its carry-over into the next stage.

Tolerances (f32 on both sides, summation order differs):
* schedules and counts (lr, negative weight, high-loss rate, batch sizes,
  validation false positives / hour, recalls): exact up to float printing
  (1e-6 relative);
* loss history: 2e-4 relative (the oracle test's bound);
* parameters after 56 Adam steps: Adam's update is ~lr * sign(m / sqrt(v)),
  so a gradient at the fp32 noise floor flips the sign of a whole lr-sized
  step; bound: 99.5 % of elements within 2e-4 absolute, every element within
  2 * sum(lr) (the most two opposite-sign trajectories can drift apart).
"""
import numpy as np
import pytest
import torch

import step_oracle_cases as cases
from oracle import golden_classifier as gc

pytestmark = pytest.mark.gpu

STAGE_HISTORIES = ("lr", "nw", "hlr", "vfp", "vrecall", "recall", "fp", "loss")


class StageIterator:
    """The fixture's batches: gc.SeqPool pools taken in the reference's order,
    with the reference's multiply_batch_size."""

    def __init__(self, pools):
        self.shares = list(gc.STAGE_SHARES)
        self.pools = [gc.SeqPool(p) for p in pools]
        self.sizes = []

    def multiply_batch_size(self, ratio):
        self.shares = [max(1, int(n * ratio)) for n in self.shares]

    def __iter__(self):
        while True:
            xs = [p.take(n) for p, n in zip(self.pools, self.shares)]
            y = np.concatenate([np.ones(self.shares[0]), np.zeros(sum(self.shares[1:]))]).astype(np.int64)
            self.sizes.append(sum(self.shares))
            yield torch.from_numpy(np.concatenate(xs)), torch.from_numpy(y)


def test_three_stage_training_matches_reference(tmp_path):
    from heybuddy.trainer import WakeWordTrainer
    gold = np.load("tests/golden/classifier_stages.npz")
    params = gc.golden_inputs()[0]
    pools, val, test = gc.stage_inputs()
    it = StageIterator(pools)
    tr = WakeWordTrainer(checkpoint_dir=str(tmp_path), device="cuda")
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    tr.model.dropout.p = 0.0
    validation = [(torch.from_numpy(x), torch.from_numpy(y)) for x, y in val]
    testing = [(torch.from_numpy(x), torch.from_numpy(y)) for x, y in test]
    h = tr(it, validation=validation, testing=testing, num_steps=gc.STAGE_STEPS,
           validation_steps=gc.STAGE_VAL_STEPS, checkpoint_steps=100000, name="stages")
    sd = tr.model.state_dict()
    cases.check_stages_against_gold(gold, params, {k: h[k].numpy() for k in STAGE_HISTORIES}, it.sizes,
                                    {k: sd[k].cpu().numpy() for k in params})
