"""The half-layer classifier (use_half_layers) on the HIP path: hbk_mlp_half.hip through
hbk_mlp_forward / hbk_mlp_train_fwd_bwd / hbk_mlp_gate_adam, the model and the trainer.

References: the reference's own results (tests/golden/classifier_half*.npz) at B = 96 and
for the 24-step epoch, and the float64 restatement (tests/half_layers_cases.py, itself pinned
to that fixture in tests/test_half_layers.py) at every other shape. Bounds are those of
tests/test_classifier_gpu.py: logits 1e-4 absolute, probabilities rtol 1e-4 / atol 1e-6,
gradients 1e-4 of each tensor's max, loss 1e-5.

Shapes: B = 1 (a single row), 17 (one past a 16-row MFMA tile), 130 (across the 64- and 128-row
tile edges, ragged tail), and layer 32 / hidden 24 / 1 layer (2 H = 48: no multiple of 16).

Dropout: the generic kernels draw their mask from splitmix64 (uniform01 in hbk_mlp_internal.h),
which half_layers_cases.generic_dropout_keep restates; oracle.mlp.dropout_keep restates the fused
kernels' hash, which no kernel on this path uses. The mask is applied to the whole [16, 96] input
BEFORE the gather, so the test fails if a branch and norm_in see different masks.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

import half_layers_cases as hc
import step_oracle_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return hc.load_gold()


@pytest.fixture(scope="module")
def inputs():
    return hc.golden_inputs()


def _model(params, layer_dim=96, num_layers=2):
    from heybuddy.wakeword import WakeWordMLPModel
    m = WakeWordMLPModel(layer_dim=layer_dim, num_layers=num_layers, use_half_layers=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m.dropout.p = 0.0
    return m.cuda()


@pytest.fixture(scope="module")
def model(inputs):
    return _model(inputs[0])


def _check_forward(m, params, x, keep=None, p=0.0, seed=0):
    xr = x.astype(np.float64)
    if keep is not None:
        xr = xr * keep.reshape(x.shape) / (1.0 - p)
    prob, z, _ = hc.forward(params, xr)
    gp, gz = m.plan.forward(m.flat_parameters, torch.from_numpy(x).cuda().reshape(len(x), -1), dropout_p=p,
                            seed=seed, logits=True)
    np.testing.assert_allclose(gz.cpu().numpy(), z, rtol=0, atol=1e-4)
    np.testing.assert_allclose(gp.cpu().numpy(), prob, rtol=1e-4, atol=1e-6)


def test_forward_matches_the_reference(gold, inputs, model):
    params, x, _, _ = inputs
    z = model.logits(torch.from_numpy(x).cuda()).cpu().numpy()
    np.testing.assert_allclose(z, gold["logit"], rtol=0, atol=1e-4)
    p = model(torch.from_numpy(x).cuda()).cpu().numpy()[:, 0]
    np.testing.assert_allclose(p, gold["prob"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("B", [1, 17, 130])
def test_forward_matches_the_restatement(inputs, model, B):
    _check_forward(model, inputs[0], hc.rows(B)[0])


def test_forward_small_architecture():
    params = hc.small_inputs(32, 1)
    _check_forward(_model(params, 32, 1), params, hc.rows(17)[0])


def test_two_forward_runs_are_bit_identical(inputs, model):
    x = torch.from_numpy(hc.rows(130)[0]).cuda().reshape(130, -1)
    runs = [model.plan.forward(model.flat_parameters, x, dropout_p=0.1, seed=77, logits=True) for _ in range(2)]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0], runs[1][0])


def test_forward_with_dropout_shares_one_mask(inputs, model):
    x = hc.rows(17)[0]
    seed = 123456789
    keep = hc.generic_dropout_keep(seed, 17, 1536, 0.1)
    assert 0.05 < 1.0 - keep.mean() < 0.15
    _check_forward(model, inputs[0], x, keep=keep, p=0.1, seed=seed)


def _train_fwd_bwd(m, x, y, neg_weight, threshold=1e-4):
    plan = m.plan
    bucket = torch.zeros(plan.n_params + plan.N_STATS, device="cuda")
    plan.train_fwd_bwd(m.flat_parameters, torch.from_numpy(x).cuda().reshape(len(x), -1), torch.from_numpy(y), bucket,
                       neg_weight=neg_weight, threshold=threshold)
    stats = bucket[plan.n_params:].cpu().numpy()
    return {k: v.cpu().numpy() for k, v in plan.views(bucket[:plan.n_params]).items()}, stats


def _check_grads(got, want, n_sel, names):
    for k in names:
        ref = np.asarray(want[k])
        scale = np.abs(ref).max() + 1e-12
        np.testing.assert_allclose(got[k] / n_sel / scale, ref / scale, rtol=0, atol=1e-4, err_msg=k)


def test_train_step_loss_and_gradients(gold, inputs, model):
    params, x, y, _ = inputs
    got, stats = _train_fwd_bwd(model, x, y, 2.0)
    n_sel = int(gold["n_sel"])
    assert int(stats[0]) == n_sel
    np.testing.assert_allclose(stats[1] / n_sel, float(gold["loss"]), rtol=1e-5)
    stored = [k for k in params if f"grad/{k}" in gold]
    assert len(stored) >= 6 * 16 + 2
    _check_grads(got, {k: gold[f"grad/{k}"] for k in stored}, n_sel, stored)
    loss, n, grads, _ = hc.step(params, x, y, neg_weight=2.0)  # (normalised by n_sel, like the fixture's)
    assert n == n_sel
    _check_grads(got, grads, n_sel, list(params))


def test_train_step_with_the_filter_dropping_rows(inputs, model):
    params = inputs[0]
    x, y = hc.rows(130, seed=45)  # (no probability of this batch within 2e-4 of the threshold)
    thr = 0.35  # between the batch's probabilities: negatives below it and positives above 1 - thr drop out
    grads, n_sel, wl, prob = hc.bucket(params, x, y, neg_weight=2.0, threshold=thr)
    assert 0 < n_sel < 130, (n_sel, prob.min(), prob.max())
    got, stats = _train_fwd_bwd(model, x, y, 2.0, threshold=thr)
    assert int(stats[0]) == n_sel
    np.testing.assert_allclose(stats[1], wl, rtol=1e-5)
    _check_grads(got, grads, 1.0, list(params))


def test_train_epoch_matches_the_reference(gold, inputs, tmp_path):
    from heybuddy.trainer import WakeWordTrainer
    params, _, _, batches = inputs
    tr = WakeWordTrainer(checkpoint_dir=str(tmp_path), use_half_layers=True)
    assert tr.model.use_half_layers and not tr.model.plan.fused
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    tr.model.dropout.p = 0.0
    data = [(torch.from_numpy(xb), torch.from_numpy(yb)) for xb, yb in batches]
    out = tr.train_epoch(data, num_steps=24, warmup_steps=4, hold_steps=8, validation_steps=1000,
                         checkpoint_steps=100000)
    lr, nw, loss, hlr, rec, fp = [t.numpy() for t in out[:6]]
    sd = tr.model.state_dict()
    stored = [k for k in params if f"epoch_final/{k}" in gold]
    assert len(stored) >= 6 * 16 + 2
    # histories with check_epoch_against_gold's bounds; final parameters on the stored subset: at most
    # 0.5 % of the entries off by more than 2e-4 (the reference's own float32 / float64 runs: none)
    cases.check_epoch_against_gold(gold, stored, lr, hlr, loss, rec, fp, {k: sd[k].cpu().numpy() for k in stored})
    # checkpoint + resume round trip keeps the Adam state, the new parameters' included
    tr.save_checkpoint("t")
    tr2 = WakeWordTrainer(checkpoint_dir=str(tmp_path), use_half_layers=True)
    tr2.resume("t")
    assert torch.equal(tr2._m, tr._m) and torch.equal(tr2._v, tr._v)
    assert torch.equal(tr2.model.flat_parameters, tr.model.flat_parameters)
    assert float(tr._m[256417:].abs().max()) > 0.0


def test_graph_steps_equal_eager_steps(inputs, tmp_path, monkeypatch):
    """The form and bounds of tests/test_classifier_gpu.py's test of the same name, on a few
    130-row steps with dropout on: the captured step reads lr, neg_weight and the dropout seed
    (which the bank's forward AND backward kernels use) from the device scalars."""
    from heybuddy.trainer import WakeWordTrainer
    params = inputs[0]
    data = []
    for i in range(4):
        x, y = hc.rows(130, seed=50 + i)
        data.append((torch.from_numpy(x), torch.from_numpy(y)))
    runs = []
    for graphs in ("1", "0"):
        monkeypatch.setenv("HBK_MLP_GRAPHS", graphs)
        tr = WakeWordTrainer(checkpoint_dir=str(tmp_path / graphs), use_half_layers=True)
        tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        tr.model.dropout.p = 0.1
        torch.manual_seed(0)
        random.seed(3)  # train_epoch's dropout seed base
        out = tr.train_epoch(data, num_steps=4, warmup_steps=2, hold_steps=1, validation_steps=1000,
                             checkpoint_steps=100000, negative_weight_schedule=[1.0, 2.0, 0.5, 1.0])
        torch.cuda.synchronize()
        runs.append((tr.model.flat_parameters.clone(), tr._m.clone(), tr._v.clone(), out[2].clone(),
                     len(getattr(tr, "_graphs", {}))))
        lr_sum = float(out[0].sum())
    (p1, m1, v1, l1, ng), (p0, m0, v0, l0, _) = runs
    assert ng >= 1
    np.testing.assert_allclose(l1.numpy(), l0.numpy(), rtol=1e-4, atol=1e-6)
    d = (p1 - p0).abs()
    start = torch.from_numpy(np.concatenate([v.ravel() for v in params.values()])).cuda()
    assert float((p1 - start).abs().max()) > 0.0  # the steps did update
    assert float((d > 1e-5).float().mean()) < 1e-3 and float(d.max()) <= min(2e-2, 2 * lr_sum)
    assert float(((m1 - m0).abs() > 1e-5 * m0.abs().max()).float().mean()) < 1e-3


def test_train_cli_with_half_layers(tmp_path, monkeypatch):
    """`heybuddy train --use-half-layers`: a short run through the generic step and the trainer's batch
    loop for validation / testing; the checkpoint it leaves is a half-layer one and converts to ONNX."""
    import os

    from click.testing import CliRunner

    from heybuddy.__main__ import main
    from heybuddy.dataset import precalculated as pc
    from heybuddy.wakeword import WakeWordMLPModel
    ckpt = tmp_path / "ckpt"
    monkeypatch.setattr(pc, "LOCAL_DIR", str(tmp_path / "precalculated"))
    args = ["train", "hey buddy", "--use-half-layers", "--steps", "8", "--stages", "1", "--validation-steps", "4",
            "--checkpoint-steps", "8", "--positive-samples", "600", "--adversarial-samples", "600",
            "--negative-samples", "2000", "--validation-negative-samples", "1000", "--validation-samples", "200",
            "--testing-positive-samples", "200", "--testing-adversarial-samples", "200",
            "--logging-steps", "4", "--checkpoint-dir", str(ckpt), "--seed", "5"]
    res = CliRunner().invoke(main, args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    heads = [f for f in os.listdir(ckpt) if f.startswith("hey_buddy") and f.endswith(".pt")
             and not f.endswith("_optimizer.pt")]
    assert heads, os.listdir(ckpt)
    m = WakeWordMLPModel.from_file(str(ckpt / heads[0]))
    assert m.use_half_layers and m.flat_parameters.numel() == hc.N_PARAMS
    assert bool(torch.isfinite(m.flat_parameters).all())
    res = CliRunner().invoke(main, ["convert", str(ckpt / heads[0])])
    assert res.exit_code == 0, res.output
    back = WakeWordMLPModel.from_file(str(ckpt / heads[0])[:-3] + ".onnx")
    assert back.use_half_layers and torch.equal(back.flat_parameters, m.flat_parameters)


def test_predict_and_fused_entry_points(model):
    from heybuddy import _native
    clip = (np.random.default_rng(0).standard_normal(23040) * 0.05).astype(np.float32)  # 1.44 s
    scores = model.predict(clip, return_scores=True)
    assert len(scores) == 1 and 0.0 <= float(scores[0]) <= 1.0
    # the fused step does not cover such a plan: a status and a message, no launch
    lib = _native.lib()
    plan = model.plan
    dev = torch.device("cuda")
    bucket = torch.zeros(plan.n_params + plan.N_STATS, device=dev)
    state = plan.new_state(dev)
    x = torch.zeros((16, 1536), device=dev)
    y = torch.zeros(16, device=dev)
    ws = torch.empty(plan.workspace_bytes(16), dtype=torch.uint8, device=dev)
    rc = lib.hbk_mlp_step_fwd_bwd(plan._handle, model.flat_parameters.data_ptr(), x.data_ptr(), 16, None, 0, None, 0,
                                  y.data_ptr(), 0, 16, state.data_ptr(), 0, None, 0, 1.0, 1e-4, 0.5, 0.0, 0,
                                  bucket.data_ptr(), None, 1, 0, ws.data_ptr(), ws.numel(), None)
    assert rc == -3  # HBK_ERR_UNSUPPORTED
    assert b"half layers" in lib.hbk_last_error()
    need = ctypes.c_int64()
    assert lib.hbk_mlp_eval_workspace_size(plan._handle, 16, ctypes.byref(need)) == -3
    assert b"half layers" in lib.hbk_last_error()
    torch.cuda.synchronize()
