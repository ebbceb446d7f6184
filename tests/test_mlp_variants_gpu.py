"""The plain MLP (use_gating=False) and every activation on the HIP path: the activation kernels of
hbk_mlp_act.hip on their own, then through hbk_mlp_forward / hbk_mlp_train_fwd_bwd /
hbk_mlp_gate_adam, the model, the trainer and the command line.

References: torch on the CPU in float64 for the activation kernels; the reference's own results
(tests/golden/classifier_variants_*.npz) at B = 96 and for the 24-step epochs; the float64
restatement (tests/mlp_variants_cases.py, itself pinned to that fixture in
tests/test_mlp_variants.py) at every other shape. Model-level bounds are those of
tests/test_classifier_gpu.py: logits 1e-4 absolute, probabilities rtol 1e-4 / atol 1e-6,
gradients 1e-4 of each tensor's max, loss 1e-5.

Activation kernels: with E = max |got - f64| / (1 + |f64|), the device's E must be at most
max(8 E_cpu, 2^-22), E_cpu being torch's own CPU float32 result in the same measure on the same
inputs (the largest over the four shapes). The factor 8: the device libm and torch's vectorised
CPU math each carry a few ulp per call and the derivative forms chain up to four calls; the floor
covers relu and identity, where E_cpu is 0 or one rounding. Measured maxima: DESIGN.md, row a11.

Shapes: (1, 8), (3, 24), (17, 64) and (16400, 64) = 1,049,600 elements, one past what 4,096
blocks x 256 threads cover without the stride loop. Model shapes: B = 1, 17 (one past a 16-row
MFMA tile), 130 (across the 64- and 128-row tile edges), layer 32 / hidden 24 / 1 layer (H no
multiple of 16, the plain hidden GEMM narrower than a tile), and no hidden layer at all.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

import mlp_variants_cases as vc
import step_oracle_cases as cases
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

VARIANTS = pytest.mark.parametrize("gated,act", vc.VARIANTS, ids=[vc.key(g, a) for g, a in vc.VARIANTS])
EPOCH_VARIANTS = pytest.mark.parametrize("gated,act", vc.EPOCH_VARIANTS,
                                         ids=[vc.key(g, a) for g, a in vc.EPOCH_VARIANTS])
THREE = pytest.mark.parametrize("gated,act", [(False, "silu"), (False, "gelu"), (True, "mish")],
                                ids=["plain_silu", "plain_gelu", "gated_mish"])
ALL14 = [(g, a) for a in vc.ACTIVATIONS for g in (True, False)]


@pytest.fixture(scope="module")
def gold():
    return vc.load_gold()


_models = {}


def _model(gated, act, params, layer_dim=96, num_layers=2):
    from heybuddy.wakeword import WakeWordMLPModel
    m = WakeWordMLPModel(layer_dim=layer_dim, num_layers=num_layers, use_gating=gated, activation=act)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m.dropout.p = 0.0
    return m.cuda()


def _gold_model(gated, act):
    if (gated, act) not in _models:
        _models[gated, act] = _model(gated, act, vc.golden_inputs(gated)[0])
    return _models[gated, act]


# --------------------------------------------------------- activation kernels ----
ACT_SHAPES = [(1, 8), (3, 24), (17, 64), (16400, 64)]
H_GRID = [0.0] + [s * v for v in (1e-4, 0.5, 1, 3, 5, 10, 19.9, 20.1, 30, 88, 100) for s in (1, -1)]
TORCH_F = {"silu": torch.nn.functional.silu, "relu": torch.nn.functional.relu, "gelu": torch.nn.functional.gelu,
           "mish": torch.nn.functional.mish, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
           "identity": lambda t: t}


def _act_inputs(rows, H):
    rng = np.random.default_rng(1000 * rows + H)
    n = rows * H
    h = np.concatenate([np.asarray(H_GRID), 2.0 * rng.standard_normal(max(n - len(H_GRID), 0))])[:n]
    return (h.reshape(rows, H).astype(np.float32), (3.0 * rng.standard_normal((rows, H))).astype(np.float32),
            (3.0 * rng.standard_normal((rows, H))).astype(np.float32))


def _torch_ref(act, gated, h, g, du, dtype):
    """(u, dhg) of torch on the CPU: F's forward, autograd's backward."""
    ht = torch.from_numpy(h).to(dtype).requires_grad_(True)
    gt = torch.from_numpy(g).to(dtype).requires_grad_(True)
    u = TORCH_F[act](ht) * gt if gated else TORCH_F[act](ht) + 0 * gt
    u.backward(torch.from_numpy(du).to(dtype))
    dhg = torch.cat([ht.grad, gt.grad], dim=1) if gated else ht.grad
    return u.detach().double().numpy(), dhg.double().numpy()


def _measure(got, ref):
    return float((np.abs(got - ref) / (1.0 + np.abs(ref))).max())


@pytest.mark.parametrize("gated,act", ALL14, ids=[vc.key(g, a) for g, a in ALL14])
def test_activation_kernels(gated, act):
    from heybuddy.kernels import mlp_activation, mlp_activation_backward
    e_dev, e_cpu = [0.0, 0.0], [0.0, 0.0]
    for rows, H in ACT_SHAPES:
        h, g, du = _act_inputs(rows, H)
        assert rows * H < len(H_GRID) or set(np.float32(H_GRID).tolist()) <= set(h.ravel().tolist())
        ref = _torch_ref(act, gated, h, g, du, torch.float64)
        cpu = _torch_ref(act, gated, h, g, du, torch.float32)
        hg = torch.from_numpy(np.concatenate([h, g], axis=1) if gated else h).cuda()
        u = mlp_activation(hg, act, gated)
        dhg = mlp_activation_backward(torch.from_numpy(du).cuda(), hg, act, gated)
        assert u.shape == (rows, H) and dhg.shape == hg.shape
        got = (u.cpu().numpy().astype(np.float64), dhg.cpu().numpy().astype(np.float64))
        for d in range(2):
            assert np.isfinite(got[d]).all(), (rows, H, "forward" if d == 0 else "backward")
            e_dev[d] = max(e_dev[d], _measure(got[d], ref[d]))
            e_cpu[d] = max(e_cpu[d], _measure(cpu[d], ref[d]))
    print(f"\nactivation {vc.key(gated, act)}: forward E_dev {e_dev[0]:.3e} E_cpu {e_cpu[0]:.3e}, "
          f"backward E_dev {e_dev[1]:.3e} E_cpu {e_cpu[1]:.3e}")
    for d in range(2):
        assert e_dev[d] <= max(8.0 * e_cpu[d], 2.0 ** -22), (d, e_dev[d], e_cpu[d])


# ----------------------------------------------------------------- forward ----
def _check_forward(m, params, x, gated, act, keep=None, p=0.0, seed=0):
    xr = x.astype(np.float64)
    if keep is not None:
        xr = xr * keep.reshape(x.shape) / (1.0 - p)
    prob, z, _ = vc.forward(params, xr, gated, act)
    gp, gz = m.plan.forward(m.flat_parameters, torch.from_numpy(x).cuda().reshape(len(x), -1), dropout_p=p,
                            seed=seed, logits=True)
    np.testing.assert_allclose(gz.cpu().numpy(), z, rtol=0, atol=1e-4)
    np.testing.assert_allclose(gp.cpu().numpy(), prob, rtol=1e-4, atol=1e-6)


@VARIANTS
def test_forward_matches_the_reference(gold, gated, act):
    g = vc.variant_gold(gold, gated, act)
    x = torch.from_numpy(vc.golden_inputs(gated)[1]).cuda()
    m = _gold_model(gated, act)
    assert not m.plan.fused
    np.testing.assert_allclose(m.logits(x).cpu().numpy(), g["logit"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(m(x).cpu().numpy()[:, 0], g["prob"], rtol=1e-4, atol=1e-6)


@THREE
@pytest.mark.parametrize("B", [1, 17, 130])
def test_forward_matches_the_restatement(gated, act, B):
    _check_forward(_gold_model(gated, act), vc.golden_inputs(gated)[0], vc.rows(B)[0], gated, act)


@THREE
def test_forward_small_architecture(gated, act):
    params = vc.small_inputs(gated, 32, 1)
    assert params["mlp_in.hidden.weight"].shape == (24, 1536)
    _check_forward(_model(gated, act, params, 32, 1), params, vc.rows(17)[0], gated, act)


@THREE
def test_forward_without_hidden_layers(gated, act):
    params = vc.without_gate(omlp.init_params(seed=23, num_layers=0), gated)
    _check_forward(_model(gated, act, params, 96, 0), params, vc.rows(17)[0], gated, act)


def test_forward_with_dropout(gold):
    gated, act = False, "silu"
    x = vc.rows(17)[0]
    seed = 123456789
    keep = vc.generic_dropout_keep(seed, 17, 1536, 0.1)
    assert 0.05 < 1.0 - keep.mean() < 0.15
    m = _gold_model(gated, act)
    _check_forward(m, vc.golden_inputs(gated)[0], x, gated, act, keep=keep, p=0.1, seed=seed)
    # training mode draws a new mask per call, evaluation mode none
    xt = torch.from_numpy(x).cuda()
    clean = vc.forward(vc.golden_inputs(gated)[0], x, gated, act)[0]
    m.dropout.p = 0.1
    try:
        m.train()
        random.seed(1)
        a, b = m(xt).cpu().numpy()[:, 0], m(xt).cpu().numpy()[:, 0]
        assert np.abs(a - b).max() > 1e-3 and np.abs(a - clean).max() > 1e-3
        m.eval()
        np.testing.assert_allclose(m(xt).cpu().numpy()[:, 0], clean, rtol=1e-4, atol=1e-6)
    finally:
        m.dropout.p = 0.0
        m.train()


# -------------------------------------------------------------- train step ----
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


@VARIANTS
def test_train_step_loss_and_gradients(gold, gated, act):
    g = vc.variant_gold(gold, gated, act)
    params, x, y, _ = vc.golden_inputs(gated)
    got, stats = _train_fwd_bwd(_gold_model(gated, act), x, y, 2.0)
    n_sel = int(g["n_sel"])
    assert int(stats[0]) == n_sel
    np.testing.assert_allclose(stats[1] / n_sel, float(g["loss"]), rtol=1e-5)
    stored = [k for k in params if f"grad/{k}" in g]
    assert stored == [k for k, v in params.items() if vc.stored(k, v.size)]
    _check_grads(got, {k: g[f"grad/{k}"] for k in stored}, n_sel, stored)
    # every tensor, the ones the fixture leaves out included, against the restatement
    _, n, grads, _ = vc.step(params, x, y, gated, act, neg_weight=2.0)
    assert n == n_sel
    _check_grads(got, grads, n_sel, list(params))


def test_train_step_with_the_filter_dropping_rows():
    gated, act = False, "silu"
    params = vc.golden_inputs(gated)[0]
    x, y = vc.rows(130, seed=45)
    thr = 0.45  # (no probability of this batch within 1e-2 of thr or 1 - thr): 53 of 130 rows stay
    grads, n_sel, wl, prob = vc.bucket(params, x, y, gated, act, neg_weight=2.0, threshold=thr)
    assert 0 < n_sel < 130, (n_sel, prob.min(), prob.max())
    got, stats = _train_fwd_bwd(_gold_model(gated, act), x, y, 2.0, threshold=thr)
    assert int(stats[0]) == n_sel
    np.testing.assert_allclose(stats[1], wl, rtol=1e-5)
    _check_grads(got, grads, 1.0, list(params))


# ------------------------------------------------------------------ trainer ----
@EPOCH_VARIANTS
def test_train_epoch_matches_the_reference(gold, gated, act, tmp_path):
    from heybuddy.trainer import WakeWordTrainer
    g = vc.variant_gold(gold, gated, act)
    params, _, _, batches = vc.golden_inputs(gated)
    tr = WakeWordTrainer(checkpoint_dir=str(tmp_path), use_gating=gated, activation=act)
    assert tr.model.use_gating == gated and tr.model.activation == act and not tr.model.plan.fused
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    tr.model.dropout.p = 0.0
    data = [(torch.from_numpy(xb), torch.from_numpy(yb)) for xb, yb in batches]
    out = tr.train_epoch(data, num_steps=24, warmup_steps=4, hold_steps=8, validation_steps=1000,
                         checkpoint_steps=100000)
    lr, nw, loss, hlr, rec, fp = [t.numpy() for t in out[:6]]
    assert 1 < len(np.unique(g["epoch/loss"])) < 24  # the gate both skipped and fired
    sd = tr.model.state_dict()
    stored = [k for k in params if f"epoch_final/{k}" in g]
    assert stored == [k for k, v in params.items() if vc.stored(k, v.size)]
    cases.check_epoch_against_gold(g, stored, lr, hlr, loss, rec, fp, {k: sd[k].cpu().numpy() for k in stored})
    # checkpoint + resume round trip keeps the Adam state
    tr.save_checkpoint("t")
    tr2 = WakeWordTrainer(checkpoint_dir=str(tmp_path), use_gating=gated, activation=act)
    tr2.resume("t")
    assert torch.equal(tr2._m, tr._m) and torch.equal(tr2._v, tr._v)
    assert torch.equal(tr2.model.flat_parameters, tr.model.flat_parameters)
    assert tr._m.numel() == vc.N_PARAMS[gated] and float(tr._m.abs().max()) > 0.0


def test_graph_steps_equal_eager_steps(tmp_path, monkeypatch):
    """The form and bounds of tests/test_classifier_gpu.py's test of the same name, on a few
    130-row steps of the plain SiLU model with dropout on."""
    from heybuddy.trainer import WakeWordTrainer
    params = vc.golden_inputs(False)[0]
    data = []
    for i in range(4):
        x, y = vc.rows(130, seed=50 + i)
        data.append((torch.from_numpy(x), torch.from_numpy(y)))
    runs = []
    for graphs in ("1", "0"):
        monkeypatch.setenv("HBK_MLP_GRAPHS", graphs)
        tr = WakeWordTrainer(checkpoint_dir=str(tmp_path / graphs), use_gating=False)
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


def test_train_cli_without_gating(tmp_path, monkeypatch):
    """`heybuddy train --no-use-gating`: a short run through the generic step and the trainer's batch
    loop for validation / testing; `predict` and `convert` then work on the plain checkpoint it leaves."""
    import os

    from click.testing import CliRunner

    from heybuddy.__main__ import main
    from heybuddy.dataset import precalculated as pc
    from heybuddy.wakeword import WakeWordMLPModel
    ckpt = tmp_path / "ckpt"
    monkeypatch.setattr(pc, "LOCAL_DIR", str(tmp_path / "precalculated"))
    args = ["train", "hey buddy", "--no-use-gating", "--steps", "8", "--stages", "1", "--validation-steps", "4",
            "--checkpoint-steps", "8", "--positive-samples", "600", "--adversarial-samples", "600",
            "--negative-samples", "2000", "--validation-negative-samples", "1000", "--validation-samples", "200",
            "--testing-positive-samples", "200", "--testing-adversarial-samples", "200",
            "--logging-steps", "4", "--checkpoint-dir", str(ckpt), "--seed", "5"]
    res = CliRunner().invoke(main, args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    heads = [f for f in os.listdir(ckpt) if f.startswith("hey_buddy") and f.endswith(".pt")
             and not f.endswith("_optimizer.pt")]
    assert heads, os.listdir(ckpt)
    head = str(ckpt / heads[0])
    m = WakeWordMLPModel.from_file(head)
    assert m.use_gating is False and m.flat_parameters.numel() == 139425
    assert bool(torch.isfinite(m.flat_parameters).all())
    res = CliRunner().invoke(main, ["convert", head])
    assert res.exit_code == 0, res.output
    back = WakeWordMLPModel.from_file(head[:-3] + ".onnx")
    assert back.use_gating is False and torch.equal(back.flat_parameters, m.flat_parameters)
    clip = str(tmp_path / "clip.npy")
    np.save(clip, (np.random.default_rng(0).standard_normal(40000) * 0.05).astype(np.float32))
    res = CliRunner().invoke(main, ["predict", head, clip, "--threshold", "2.0"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert "No wake-word utterances detected" in res.output  # (no score exceeds 2)


def test_plain_plan_at_the_default_dimensions(tmp_path):
    """Its dimensions are the fused kernels', its layout is not: every fused entry point refuses it."""
    from heybuddy import _native
    from heybuddy.trainer import WakeWordTrainer
    m = _gold_model(False, "silu")
    clip = (np.random.default_rng(0).standard_normal(23040) * 0.05).astype(np.float32)  # 1.44 s
    scores = m.predict(clip, return_scores=True)
    assert len(scores) == 1 and 0.0 <= float(scores[0]) <= 1.0
    lib = _native.lib()
    plan = m.plan
    assert (plan.d_in, plan.layer_dim, plan.hidden, plan.n_layers) == (1536, 96, 64, 2) and not plan.fused
    v = ctypes.c_int32()
    assert lib.hbk_mlp_step_variant(plan._handle, 1100, None, ctypes.byref(v)) == -3  # HBK_ERR_UNSUPPORTED
    assert b"gated SiLU" in lib.hbk_last_error()
    need = ctypes.c_int64()
    assert lib.hbk_mlp_eval_workspace_size(plan._handle, 16, ctypes.byref(need)) == -3
    assert b"gated SiLU" in lib.hbk_last_error()
    info = (ctypes.c_int32 * 19)()
    assert lib.hbk_mlp_step_plan_info(plan._handle, 1100, None, info, 19) == -3
    dev = torch.device("cuda")
    bucket = torch.zeros(plan.n_params + plan.N_STATS, device=dev)
    state = plan.new_state(dev)
    x = torch.zeros((16, 1536), device=dev)
    y = torch.zeros(16, device=dev)
    ws = torch.empty(plan.workspace_bytes(16), dtype=torch.uint8, device=dev)
    rc = lib.hbk_mlp_step_fwd_bwd(plan._handle, m.flat_parameters.data_ptr(), x.data_ptr(), 16, None, 0, None, 0,
                                  y.data_ptr(), 0, 16, state.data_ptr(), 0, None, 0, 1.0, 1e-4, 0.5, 0.0, 0,
                                  bucket.data_ptr(), None, 1, 0, ws.data_ptr(), ws.numel(), None)
    assert rc == -3
    mv = torch.zeros(plan.n_params, device=dev)
    rc = lib.hbk_mlp_step_update(plan._handle, m.flat_parameters.data_ptr(), bucket.data_ptr(), mv.data_ptr(),
                                 mv.data_ptr(), state.data_ptr(), 0, None, 0, 1e-3, 0.9, 0.999, 1e-8, None, 0,
                                 None, 0, None)
    assert rc == -3
    tr = WakeWordTrainer(checkpoint_dir=str(tmp_path), use_gating=False)
    with pytest.raises(NotImplementedError):
        tr.train_indexed(None, None, None)
    torch.cuda.synchronize()
