"""Classifier on the HIP path vs the reference's own outputs (golden fixture).

Tolerances: logits 1e-4 absolute (north star); gradients 1e-4 of each
tensor's max |g|; Adam (first step) — every update is lr * m/(sqrt(v)+eps),
i.e. ~lr * sign(g) for |g| >> eps, so parameters agree to 1e-6 except where
|g| sits at the fp32 noise floor and the sign of g is arbitrary: there the
difference is bounded by 2 lr; such elements must be < 0.1 %.
"""
import os

import numpy as np
import pytest
import torch

import step_oracle_cases as cases
from oracle import golden_classifier as gc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classifier.npz")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def inputs():
    return gc.golden_inputs()


def _model(params):
    from heybuddy.wakeword import WakeWordMLPModel
    m = WakeWordMLPModel()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m.dropout.p = 0.0
    return m.cuda()


def test_state_dict_roundtrip_and_views(inputs):
    params = inputs[0]
    m = _model(params)
    sd = m.state_dict()
    assert list(sd) == list(params)
    for k, v in params.items():
        np.testing.assert_array_equal(sd[k].cpu().numpy(), v)
    assert m.flat_parameters.numel() == 256417


def test_forward_logits_match_reference(gold, inputs):
    params, x, y, _ = inputs
    m = _model(params)
    z = m.logits(torch.from_numpy(x).cuda()).cpu().numpy()
    np.testing.assert_allclose(z, gold["logit"], rtol=0, atol=1e-4)
    p = m(torch.from_numpy(x).cuda()).cpu().numpy()[:, 0]
    np.testing.assert_allclose(p, gold["prob"], rtol=1e-4, atol=1e-6)


def test_train_step_grads_and_adam(gold, inputs):
    params, x, y, _ = inputs
    m = _model(params)
    plan = m.plan
    flat = m.flat_parameters
    bucket = torch.zeros(plan.n_params + plan.N_STATS, device="cuda")
    plan.train_fwd_bwd(flat, torch.from_numpy(x).cuda().reshape(len(x), -1), torch.from_numpy(y), bucket,
                       neg_weight=2.0)
    stats = bucket[plan.n_params:].cpu().numpy()
    n_sel = int(gold["n_sel"])
    assert int(stats[0]) == n_sel
    np.testing.assert_allclose(stats[1] / n_sel, float(gold["loss"]), rtol=1e-5)
    g = plan.views(bucket[:plan.n_params] / n_sel)
    for k in params:
        ref = gold[f"grad/{k}"]
        scale = np.abs(ref).max() + 1e-12
        np.testing.assert_allclose(g[k].cpu().numpy() / scale, ref / scale, rtol=0, atol=1e-4, err_msg=k)
    # gate (fires: n_sel >= 128 or not?) then Adam with the trainer's first step
    mm, vv = torch.zeros_like(flat), torch.zeros_like(flat)
    state = torch.tensor([0.0, 1.0, 0.0, 0.0], device="cuda")
    if n_sel < 128:
        state[0] = 128.0  # pretend earlier steps accumulated: the gate must fire now
    ctrl = torch.zeros(4, device="cuda")
    hist = torch.zeros((1, 8), device="cuda")
    plan.gate_adam(flat, bucket, mm, vv, state, ctrl, hist, 1e-3)
    h = hist.cpu().numpy()[0]
    assert h[2] == 1.0 and h[0] == n_sel
    new = plan.views(flat)
    bad = total = 0
    for k in params:
        d = np.abs(new[k].cpu().numpy() - gold[f"adam1/{k}"])
        assert d.max() <= 2.05e-3, k
        bad += int((d > 1e-6).sum())
        total += d.size
    assert bad / total < 1e-3, f"{bad} of {total} parameters differ by > 1e-6"


def test_train_epoch_matches_reference(gold, inputs, tmp_path):
    from heybuddy.trainer import WakeWordTrainer
    params, _, _, batches = inputs
    tr = WakeWordTrainer(checkpoint_dir=str(tmp_path))
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    tr.model.dropout.p = 0.0
    data = [(torch.from_numpy(xb), torch.from_numpy(yb)) for xb, yb in batches]
    out = tr.train_epoch(data, num_steps=24, warmup_steps=4, hold_steps=8, validation_steps=1000,
                         checkpoint_steps=100000)
    lr, nw, loss, hlr, rec, fp = [t.numpy() for t in out[:6]]
    sd = tr.model.state_dict()
    cases.check_epoch_against_gold(gold, params, lr, hlr, loss, rec, fp, {k: sd[k].cpu().numpy() for k in params})
    # checkpoint + resume round trip keeps the Adam state
    tr.save_checkpoint("t")
    tr2 = WakeWordTrainer(checkpoint_dir=str(tmp_path))
    tr2.resume("t")
    assert torch.equal(tr2._m, tr._m) and torch.equal(tr2.model.flat_parameters, tr.model.flat_parameters)


def test_graph_steps_equal_eager_steps(inputs, tmp_path, monkeypatch):
    """The captured-hipGraph step (default) and the eager step launch the same
    kernels; lr (warmup schedule), neg_weight and the dropout seed reach the
    graph through the device scalars, so 10 steps with dropout on must agree.
    Not bit for bit: split-K GEMMs and the loss statistics accumulate with
    float atomics (order varies run to run, eager or not). Loss history to
    1e-4; parameters: Adam turns fp32-noise-floor gradients into +-lr steps
    (module docstring), so < 0.1 % of them may differ by more than 1e-5.
    A wrong lr, neg_weight or dropout seed moves the losses by >> 1e-4."""
    from heybuddy.trainer import WakeWordTrainer
    params, _, _, batches = inputs
    data = [(torch.from_numpy(xb), torch.from_numpy(yb)) for xb, yb in batches][:10]
    runs = []
    for graphs in ("1", "0"):
        monkeypatch.setenv("HBK_MLP_GRAPHS", graphs)
        tr = WakeWordTrainer(checkpoint_dir=str(tmp_path / graphs))
        tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        tr.model.dropout.p = 0.1
        torch.manual_seed(0)
        import random
        random.seed(3)  # train_epoch's dropout seed base
        out = tr.train_epoch(data, num_steps=10, warmup_steps=4, hold_steps=3, validation_steps=1000,
                             checkpoint_steps=100000, negative_weight_schedule=[1.0, 2.0, 0.5] * 4)
        torch.cuda.synchronize()
        runs.append((tr.model.flat_parameters.clone(), tr._m.clone(), tr._v.clone(), out[2].clone(),
                     len(getattr(tr, "_graphs", {}))))
        lr_sum = float(out[0].sum())  # the schedule's: the same in both runs
    (p1, m1, v1, l1, ng), (p0, m0, v0, l0, _) = runs
    assert ng >= 1
    np.testing.assert_allclose(l1.numpy(), l0.numpy(), rtol=1e-4, atol=1e-6)
    d = (p1 - p0).abs()
    assert float((d > 1e-5).float().mean()) < 1e-3 and float(d.max()) <= min(2e-2, 2 * lr_sum)
    assert float(((m1 - m0).abs() > 1e-5 * m0.abs().max()).float().mean()) < 1e-3
