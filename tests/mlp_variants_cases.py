"""Inputs and float64 restatement of the classifier's block variants: the plain MLP
(use_gating=False, reference modules/multi_layer_perceptron.py:18-74) and the gated one
(:76-124) with every activation of get_activation (util/modeling_util.py:74-115). Shared by
tests/test_mlp_variants.py (CPU), tests/test_mlp_variants_gpu.py and
tools/make_mlp_variants_golden.py. oracle/mlp.py restates gated SiLU only.

The fixture tests/golden/classifier_variants_*.npz (load_gold) stores the reference's results
only, under "<variant>/...", a variant being "gated_gelu", "plain_silu", ...: every input is
regenerated from seeds. Parameters, x, y and the epoch's batches are
oracle.golden_classifier.golden_inputs(); a plain variant drops the ``*.gate.*`` tensors (the
reference's plain state dict is the gated one without them).

The restatement is numpy float64 on oracle.mlp's pieces (LayerNorm and its backward, the
filter, the loss, Adam, the schedule). ``onnx_eval`` evaluates the node types
heybuddy.util.onnx_util.write_wakeword_onnx emits.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict

import numpy as np

from half_layers_cases import generic_dropout_keep, rows  # noqa: F401  (re-exported)
from oracle import golden_classifier as gc
from oracle import mlp as omlp
from oracle.mlp import Adam, learning_rate, step_loss_and_dz

ACTIVATIONS = ("silu", "relu", "gelu", "mish", "tanh", "sigmoid", "identity")
# the 13 variants this work adds (gated SiLU is the default architecture: tests/golden/classifier.npz)
VARIANTS = [(g, a) for g in (True, False) for a in ACTIVATIONS if not (g and a == "silu")]
EPOCH_VARIANTS = [(False, "silu"), (False, "relu"), (False, "mish"), (True, "gelu")]
N_PARAMS = {True: 256417, False: 139425}
# gradient / final-parameter records the fixture stores: every tensor of at most 1,536 elements, and
STORED_MAX = 1536
STORED_BIG = ("layers.1.1.hidden.weight", "mlp_in.output.weight")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def key(gated: bool, act: str) -> str:
    return f"{'gated' if gated else 'plain'}_{act}"


def stored(name: str, size: int) -> bool:
    return size <= STORED_MAX or name in STORED_BIG


def gold_path(gated: bool) -> str:
    """Two files, each under the 1 MiB a committed file may have: the gated and the plain variants."""
    return os.path.join(GOLDEN, f"classifier_variants_{'gated' if gated else 'plain'}.npz")


def load_gold() -> dict:
    """The whole fixture as one {"<variant>/<record>": array}."""
    out = {}
    for gated in (True, False):
        with np.load(gold_path(gated)) as f:
            out.update({k: f[k] for k in f.files})
    return out


def variant_gold(gold: dict, gated: bool, act: str) -> dict:
    """One variant's records, without the prefix."""
    pre = key(gated, act) + "/"
    return {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre)}


def without_gate(params, gated: bool):
    return OrderedDict((k, v) for k, v in params.items() if gated or ".gate." not in k)


_cache = {}


def golden_inputs(gated: bool):
    """(params, x [96, 16, 96], y, epoch batches) of the fixture for a gated / plain model."""
    if "gold" not in _cache:
        _cache["gold"] = gc.golden_inputs()
    params, x, y, batches = _cache["gold"]
    return without_gate(params, gated), x, y, batches


def small_inputs(gated: bool, layer_dim: int = 32, num_layers: int = 1):
    """Parameters of a non-default architecture, the base of half_layers_cases.small_inputs
    (layer 32 -> hidden 24: no multiple of 16, narrower than a 64-wide GEMM tile)."""
    k = ("small", layer_dim, num_layers)
    if k not in _cache:
        _cache[k] = omlp.init_params(seed=23, layer_dim=layer_dim, num_layers=num_layers)
    return without_gate(_cache[k], gated)


# -------------------------------------------------------------- activations ----
_erf = np.vectorize(math.erf, otypes=[np.float64])


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def act_f(act: str, x):
    """f(x), torch's definitions (nn.GELU(): the erf form; nn.Mish: x tanh(softplus(x)))."""
    if act == "relu":
        return np.maximum(x, 0.0)
    if act == "gelu":
        return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))
    if act == "silu":
        return x * _sig(x)
    if act == "mish":
        return x * np.tanh(np.logaddexp(0.0, x))
    if act == "tanh":
        return np.tanh(x)
    if act == "sigmoid":
        return _sig(x)
    assert act == "identity", act
    return x


def act_df(act: str, x):
    if act == "relu":
        return (x > 0).astype(x.dtype)
    if act == "gelu":
        return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if act == "silu":
        s = _sig(x)
        return s * (1.0 + x * (1.0 - s))
    if act == "mish":
        t = np.tanh(np.logaddexp(0.0, x))
        return t + x * (1.0 - t * t) * _sig(x)
    if act == "tanh":
        return 1.0 - np.tanh(x) ** 2
    if act == "sigmoid":
        s = _sig(x)
        return s * (1.0 - s)
    assert act == "identity", act
    return np.ones_like(x)


# -------------------------------------------------------------- restatement ----
def _num_layers(p) -> int:
    return sum(1 for k in p if k.startswith("layers.") and k.endswith(".0.weight"))


def _mlp(p, prefix, x, cache, gated, act):
    h = x @ p[f"{prefix}.hidden.weight"].T + p[f"{prefix}.hidden.bias"]
    g = x @ p[f"{prefix}.gate.weight"].T + p[f"{prefix}.gate.bias"] if gated else None
    u = act_f(act, h) * g if gated else act_f(act, h)
    cache[prefix] = (x, h, g, u)
    return u @ p[f"{prefix}.output.weight"].T + p[f"{prefix}.output.bias"]


def _mlp_back(p, grads, prefix, dout, cache, gated, act):
    x, h, g, u = cache[prefix]
    grads[f"{prefix}.output.weight"] = dout.T @ u
    grads[f"{prefix}.output.bias"] = dout.sum(axis=0)
    du = dout @ p[f"{prefix}.output.weight"]
    dh = du * act_df(act, h) * (g if gated else 1.0)
    grads[f"{prefix}.hidden.weight"] = dh.T @ x
    grads[f"{prefix}.hidden.bias"] = dh.sum(axis=0)
    dx = dh @ p[f"{prefix}.hidden.weight"]
    if gated:
        dg = du * act_f(act, h)
        grads[f"{prefix}.gate.weight"] = dg.T @ x
        grads[f"{prefix}.gate.bias"] = dg.sum(axis=0)
        dx = dx + dg @ p[f"{prefix}.gate.weight"]
    return dx


def forward(params, x, gated: bool, act: str):
    """x [B, 16, 96] (already dropped out, if at all) -> (prob [B], logit [B], cache)."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    assert ("mlp_in.gate.weight" in p) == gated
    L = _num_layers(p)
    x = np.asarray(x, dtype=np.float64).reshape(x.shape[0], -1)
    cache = {"num_layers": L}
    xn, xh, rs = omlp._ln(x, p["norm_in.weight"], p["norm_in.bias"])
    cache["norm_in"] = (xh, rs)
    s = _mlp(p, "mlp_in", xn, cache, gated, act)
    for l in range(L):
        xn, xh, rs = omlp._ln(s, p[f"layers.{l}.0.weight"], p[f"layers.{l}.0.bias"])
        cache[f"layers.{l}.0"] = (xh, rs)
        s = _mlp(p, f"layers.{l}.1", xn, cache, gated, act)
    xn, xh, rs = omlp._ln(s, p["norm_out.weight"], p["norm_out.bias"])
    cache["norm_out"] = (xh, rs)
    z = _mlp(p, "mlp_out", xn, cache, gated, act)[:, 0]
    return 1.0 / (1.0 + np.exp(-z)), z, cache


def backward(params, cache, dz, gated: bool, act: str):
    """Gradients of sum_i dz_i z_i for every parameter, in state-dict order."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    grads = OrderedDict()
    ds = _mlp_back(p, grads, "mlp_out", dz[:, None], cache, gated, act)
    ds = omlp._ln_back(grads, "norm_out", ds, p["norm_out.weight"], cache)
    for l in reversed(range(cache["num_layers"])):
        ds = _mlp_back(p, grads, f"layers.{l}.1", ds, cache, gated, act)
        ds = omlp._ln_back(grads, f"layers.{l}.0", ds, p[f"layers.{l}.0.weight"], cache)
    ds = _mlp_back(p, grads, "mlp_in", ds, cache, gated, act)
    omlp._ln_back(grads, "norm_in", ds, p["norm_in.weight"], cache)
    return OrderedDict((k, grads[k]) for k in params)


def step(params, x, y, gated: bool, act: str, neg_weight=1.0, threshold=1e-4):
    """The trainer's filtered weighted BCE of one batch: (loss, n_sel, gradients, prob)."""
    prob, _, cache = forward(params, x, gated, act)
    loss, n, dz = step_loss_and_dz(prob, y, neg_weight, threshold)
    return loss, n, backward(params, cache, dz, gated, act), prob


def bucket(params, x, y, gated: bool, act: str, neg_weight=1.0, threshold=1e-4):
    """What hbk_mlp_train_fwd_bwd leaves: the UNNORMALISED gradients (sum over the selected rows
    of w dl/dz) by name, n_sel, sum w l and the probabilities."""
    prob, _, cache = forward(params, x, gated, act)
    sel = omlp.select_high_loss(prob, y, threshold)
    dz = np.zeros_like(prob)
    ps, ys = prob[sel], y[sel].astype(np.float64)
    w = np.where(ys == 1, 1.0, neg_weight)
    dz[sel] = w * (ps - ys)
    return backward(params, cache, dz, gated, act), sel.size, float((w * omlp.bce_terms(ps, ys)).sum()), prob


def train_epoch(params, batches, num_steps, warmup_steps, hold_steps, gated: bool, act: str, target=1e-3,
                neg_weight=1.0, threshold=1e-4):
    """oracle.mlp.train_epoch with this module's forward / backward: (params, history)."""
    params = OrderedDict((k, np.asarray(v, dtype=np.float64)) for k, v in params.items())
    opt = Adam(params)
    acc_steps, acc_samples = 1, 0
    hist = {"lr": [], "loss": [], "high_loss_rate": [], "updated": []}
    for i, (x, y) in enumerate(batches):
        if i >= num_steps:
            break
        lr = learning_rate(i, warmup_steps, hold_steps, num_steps, target)
        hist["lr"].append(lr)
        prob, _, cache = forward(params, x, gated, act)
        sel = omlp.select_high_loss(prob, y, threshold)
        hist["high_loss_rate"].append(sel.size / prob.shape[0])
        updated = False
        if sel.size:
            loss, n, dz = step_loss_and_dz(prob, y, neg_weight, threshold, acc_steps)
            acc_samples += n
            if acc_samples < 128:
                acc_steps += 1
                if hist["loss"]:
                    hist["loss"].append(hist["loss"][-1])
            else:
                params = opt.step(params, backward(params, cache, dz, gated, act), lr)
                acc_steps, acc_samples = 1, 0
                hist["loss"].append(loss)
                updated = True
        elif hist["loss"]:
            hist["loss"].append(hist["loss"][-1])
        else:
            hist["loss"].append(0.0)
        hist["updated"].append(updated)
    return params, hist


# ------------------------------------------------------------ ONNX evaluator ----
def onnx_eval(model, x) -> np.ndarray:
    """The graph of a heybuddy.util.onnx_util.OnnxModel on input x [B, 16, 96], node by node in
    float64, for exactly the node types write_wakeword_onnx emits without half layers."""
    val = {k: v.astype(np.float64) if v.dtype.kind == "f" else v for k, v in model.initializers.items()}
    val["input"] = np.asarray(x, dtype=np.float64)
    for n in model.nodes:
        a = [val[i] for i in n.inputs]
        if n.op == "Flatten":
            r = a[0].reshape(a[0].shape[0], -1)
        elif n.op == "LayerNormalization":
            assert n.attrs["axis"] == -1 and abs(n.attrs["epsilon"] - omlp.LN_EPS) < 1e-12
            r = omlp._ln(a[0], a[1], a[2])[0]
        elif n.op == "Gemm":
            assert n.attrs["transB"] == 1 and n.attrs["alpha"] == 1.0 and n.attrs["beta"] == 1.0
            r = a[0] @ a[1].T + a[2]
        elif n.op == "Relu":
            r = np.maximum(a[0], 0.0)
        elif n.op == "Tanh":
            r = np.tanh(a[0])
        elif n.op == "Sigmoid":
            r = _sig(a[0])
        elif n.op == "Softplus":
            r = np.logaddexp(0.0, a[0])
        elif n.op == "Erf":
            r = _erf(a[0])
        elif n.op == "Div":
            r = a[0] / a[1]
        elif n.op == "Add":
            r = a[0] + a[1]
        else:
            assert n.op == "Mul", n.op
            r = a[0] * a[1]
        val[n.outputs[0]] = r
    return val["output"]
