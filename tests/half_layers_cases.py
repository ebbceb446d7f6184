"""Inputs and float64 restatement of the half-layer classifier (use_half_layers,
reference src/python/heybuddy/wakeword.py:211-223, :278-302, :334-348), shared by
tests/test_half_layers.py (CPU), tests/test_half_layers_gpu.py and
tools/make_half_layers_golden.py.

The fixture tests/golden/classifier_half*.npz (load_gold) stores the reference's results only:
every input is regenerated here from seeds. ``params``, ``x``, ``y`` and the epoch's
``batches`` are oracle.golden_classifier.golden_inputs(); the half layers' tensors
come from numpy's default_rng(19), drawn in state-dict order, with LayerNorm weights
1 + 0.2 N(0, 1) and biases 0.1 N(0, 1) (at the default 1 / 0 the bias term of the
input weights' gradient and the weight's scaling would vanish) and every linear
tensor uniform in +-1 / sqrt(fan_in).

The restatement is numpy float64 on top of oracle.mlp's pieces (LayerNorm, gated
MLP and their backward, Adam, schedule, filter): branch h reads rows
HALF_INDICES[h] of the [16, 96] input in the listed order (the last two lists are
not ascending), normalises them with its own LayerNorm(768) and adds its gated MLP
onto mlp_in's output. All branches and norm_in read one dropped-out input.
"""
from __future__ import annotations

import math
import os
import re
from collections import OrderedDict

import numpy as np

from oracle import golden_classifier as gc
from oracle import mlp as omlp

HALF_INDICES = [
    [0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13, 14, 15], [0, 1, 2, 3, 8, 9, 10, 11], [4, 5, 6, 7, 12, 13, 14, 15],
    [4, 5, 6, 7, 8, 9, 10, 11], [0, 1, 2, 3, 12, 13, 14, 15], [0, 1, 4, 5, 8, 9, 12, 13], [2, 3, 6, 7, 10, 11, 14, 15],
    [0, 1, 6, 7, 8, 9, 14, 15], [2, 3, 4, 5, 10, 11, 12, 13], [0, 2, 4, 6, 8, 10, 12, 14], [1, 3, 5, 7, 9, 11, 13, 15],
    [0, 3, 4, 7, 8, 11, 12, 15], [1, 2, 5, 6, 9, 10, 13, 14], [0, 5, 2, 7, 8, 13, 10, 15], [1, 4, 3, 6, 9, 12, 11, 14],
]
N_PARAMS = 1955745  # 256,417 + 16 x 106,208 at the defaults
# tensors of the gradient / epoch records the fixture stores: all of at most 8,192 elements (every
# branch's LayerNorm and bias tensors, which depend on the whole gather order) plus one big matrix
# of a sorted and of an unsorted branch
STORED_MAX = 8192
STORED_BIG = ("half_layers.0.1.hidden.weight", "half_layers.15.1.gate.weight")


def stored(name: str, size: int) -> bool:
    return size <= STORED_MAX or name in STORED_BIG


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def split_gold(record) -> dict:
    """{file: keys}: the fixture travels as three files, each under the 1 MiB a committed file may
    have: the epoch's record, the two big matrices' records, everything else."""
    files = {os.path.join(GOLDEN, f"classifier_half{s}.npz"): [] for s in ("", "_big", "_epoch")}
    main, big, epoch = files
    for k in record:
        if k.split("/", 1)[-1] in STORED_BIG:
            files[big].append(k)
        else:
            files[epoch if k.startswith("epoch") else main].append(k)
    return files


def load_gold() -> dict:
    """The whole fixture as one {key: array}."""
    out = {}
    for s in ("", "_big", "_epoch"):
        with np.load(os.path.join(GOLDEN, f"classifier_half{s}.npz")) as f:
            out.update({k: f[k] for k in f.files})
    return out


def param_shapes(input_shape=(16, 96), layer_dim: int = 96, num_layers: int = 2) -> "OrderedDict[str, tuple]":
    """state_dict names and shapes with half layers, in the reference's order: the
    half layers sit between mlp_in and layers."""
    base = omlp.param_shapes(input_shape, layer_dim, num_layers)
    k = input_shape[0] * input_shape[1] // 2
    hid = omlp.normalized_dim(layer_dim)
    out = OrderedDict()
    for name, shp in base.items():
        if name == "layers.0.0.weight" or (num_layers == 0 and name == "norm_out.weight"):
            for h in range(len(HALF_INDICES)):
                out[f"half_layers.{h}.0.weight"] = (k,)
                out[f"half_layers.{h}.0.bias"] = (k,)
                p = f"half_layers.{h}.1"
                out[f"{p}.hidden.weight"] = (hid, k)
                out[f"{p}.hidden.bias"] = (hid,)
                out[f"{p}.output.weight"] = (layer_dim, hid)
                out[f"{p}.output.bias"] = (layer_dim,)
                out[f"{p}.gate.weight"] = (hid, k)
                out[f"{p}.gate.bias"] = (hid,)
        out[name] = shp
    return out


def with_half_params(base: "OrderedDict[str, np.ndarray]", names, layer_dim: int = 96, num_layers: int = 2,
                     seed: int = 19):
    """``base`` (the tensors without half layers) plus the half layers' tensors drawn from
    default_rng(seed): walk ``names`` (state-dict order), skip what ``base`` supplies."""
    shapes = param_shapes(layer_dim=layer_dim, num_layers=num_layers)
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name in names:
        if name in base:
            out[name] = base[name]
            continue
        shp = shapes[name]
        if re.fullmatch(r"half_layers\.\d+\.0\.(weight|bias)", name):  # a branch's LayerNorm
            v = 1.0 + 0.2 * rng.standard_normal(shp) if name.endswith("weight") else 0.1 * rng.standard_normal(shp)
        else:
            lin = name.rsplit(".", 1)[0]
            b = 1.0 / math.sqrt(shapes[f"{lin}.weight"][1])
            v = rng.uniform(-b, b, shp)
        out[name] = v.astype(np.float32)
    return out


_cache = {}


def golden_inputs():
    """(params with half layers, x [96, 16, 96], y, epoch batches) of the fixture."""
    if "gold" not in _cache:
        params, x, y, batches = gc.golden_inputs()
        _cache["gold"] = (with_half_params(params, list(param_shapes())), x, y, batches)
    return _cache["gold"]


def small_inputs(layer_dim: int = 32, num_layers: int = 1):
    """Parameters of a non-default architecture (layer 32 -> hidden 24: 2 H = 48 is no
    multiple of the 64-wide tile, H no multiple of 16)."""
    key = ("small", layer_dim, num_layers)
    if key not in _cache:
        base = omlp.init_params(seed=23, layer_dim=layer_dim, num_layers=num_layers)
        names = list(param_shapes(layer_dim=layer_dim, num_layers=num_layers))
        _cache[key] = with_half_params(base, names, layer_dim, num_layers, seed=29)
    return _cache[key]


def rows(n: int, seed: int = 41):
    """n seeded input rows [n, 16, 96] and labels, in the fixture's style (x: golden_inputs' 96
    rows are the first 96 of none of these: a separate stream)."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((16, 96))
    u /= np.linalg.norm(u)
    y = (rng.random(n) < 0.4).astype(np.int64)
    x = rng.standard_normal((n, 16, 96)) + np.where(y[:, None, None] == 1, 3.0, -1.0) * u
    return x.astype(np.float32), y


# ------------------------------------------------------------ restatement ----
def _num_layers(p) -> int:
    return sum(1 for k in p if k.startswith("layers.") and k.endswith(".0.weight"))


def forward(params, x, dtype=np.float64):
    """x [B, 16, 96] (already dropped out, if at all) -> (prob [B], logit [B], cache)."""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    L = _num_layers(p)
    x3 = np.asarray(x, dtype=dtype).reshape(x.shape[0], 16, -1)
    cache = {"num_layers": L}
    xn, xh, rs = omlp._ln(x3.reshape(x3.shape[0], -1), p["norm_in.weight"], p["norm_in.bias"])
    cache["norm_in"] = (xh, rs)
    s = omlp._gmlp(p, "mlp_in", xn, cache)
    for h, idx in enumerate(HALF_INDICES):
        xg = x3[:, idx, :].reshape(x3.shape[0], -1)
        xn, xh, rs = omlp._ln(xg, p[f"half_layers.{h}.0.weight"], p[f"half_layers.{h}.0.bias"])
        cache[f"half_layers.{h}.0"] = (xh, rs)
        s = s + omlp._gmlp(p, f"half_layers.{h}.1", xn, cache)
    for l in range(L):
        xn, xh, rs = omlp._ln(s, p[f"layers.{l}.0.weight"], p[f"layers.{l}.0.bias"])
        cache[f"layers.{l}.0"] = (xh, rs)
        s = omlp._gmlp(p, f"layers.{l}.1", xn, cache)
    xn, xh, rs = omlp._ln(s, p["norm_out.weight"], p["norm_out.bias"])
    cache["norm_out"] = (xh, rs)
    z = omlp._gmlp(p, "mlp_out", xn, cache)[:, 0]
    return 1.0 / (1.0 + np.exp(-z)), z, cache


def backward(params, cache, dz, dtype=np.float64):
    """Gradients of sum_i dz_i z_i for every parameter, in state-dict order."""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    grads = OrderedDict()
    ds = omlp._gmlp_back(p, grads, "mlp_out", dz[:, None], cache)
    ds = omlp._ln_back(grads, "norm_out", ds, p["norm_out.weight"], cache)
    for l in reversed(range(cache["num_layers"])):
        ds = omlp._gmlp_back(p, grads, f"layers.{l}.1", ds, cache)
        ds = omlp._ln_back(grads, f"layers.{l}.0", ds, p[f"layers.{l}.0.weight"], cache)
    for h in range(len(HALF_INDICES)):  # ds: the gradient at mlp_in's output, shared by every branch
        d = omlp._gmlp_back(p, grads, f"half_layers.{h}.1", ds, cache)
        omlp._ln_back(grads, f"half_layers.{h}.0", d, p[f"half_layers.{h}.0.weight"], cache)
    ds = omlp._gmlp_back(p, grads, "mlp_in", ds, cache)
    omlp._ln_back(grads, "norm_in", ds, p["norm_in.weight"], cache)
    return OrderedDict((k, grads[k]) for k in params)


def step(params, x, y, neg_weight=1.0, threshold=1e-4):
    """The trainer's filtered weighted BCE of one batch: (loss, n_sel, gradients, prob)."""
    prob, _, cache = forward(params, x)
    loss, n, dz = omlp.step_loss_and_dz(prob, y, neg_weight, threshold)
    return loss, n, backward(params, cache, dz), prob


def train_epoch(params, batches, num_steps, warmup_steps, hold_steps, target=1e-3, neg_weight=1.0,
                threshold=1e-4):
    """oracle.mlp.train_epoch with this module's forward / backward: (params, history)."""
    params = OrderedDict((k, np.asarray(v, dtype=np.float64)) for k, v in params.items())
    opt = omlp.Adam(params)
    acc_steps, acc_samples = 1, 0
    hist = {"lr": [], "loss": [], "high_loss_rate": [], "updated": []}
    for i, (x, y) in enumerate(batches):
        if i >= num_steps:
            break
        lr = omlp.learning_rate(i, warmup_steps, hold_steps, num_steps, target)
        hist["lr"].append(lr)
        prob, _, cache = forward(params, x)
        sel = omlp.select_high_loss(prob, y, threshold)
        hist["high_loss_rate"].append(sel.size / prob.shape[0])
        updated = False
        if sel.size:
            loss, n, dz = omlp.step_loss_and_dz(prob, y, neg_weight, threshold, acc_steps)
            acc_samples += n
            if acc_samples < 128:
                acc_steps += 1
                if hist["loss"]:
                    hist["loss"].append(hist["loss"][-1])
            else:
                params = opt.step(params, backward(params, cache, dz), lr)
                acc_steps, acc_samples = 1, 0
                hist["loss"].append(loss)
                updated = True
        elif hist["loss"]:
            hist["loss"].append(hist["loss"][-1])
        else:
            hist["loss"].append(0.0)
        hist["updated"].append(updated)
    return params, hist


def bucket(params, x, y, neg_weight=1.0, threshold=1e-4):
    """What hbk_mlp_train_fwd_bwd leaves: the UNNORMALISED gradients (sum over the selected rows
    of w dl/dz) by name, n_sel and sum w l."""
    prob, _, cache = forward(params, x)
    sel = omlp.select_high_loss(prob, y, threshold)
    dz = np.zeros_like(prob)
    ps, ys = prob[sel], y[sel].astype(np.float64)
    w = np.where(ys == 1, 1.0, neg_weight)
    dz[sel] = w * (ps - ys)
    return backward(params, cache, dz), sel.size, float((w * omlp.bce_terms(ps, ys)).sum()), prob


def generic_dropout_keep(seed: int, n_rows: int, d: int = 1536, p: float = 0.1) -> np.ndarray:
    """The input-dropout mask of the generic classifier kernels (dropout_elem and
    uniform01 in hbk_mlp_internal.h, which hbk_mlp.hip and the half-layer kernels share): element i = row d + column
    of the UNGATHERED input is dropped iff the top 24 bits of splitmix64(seed + golden (i + 1)),
    as a float32 in [0, 1), are below p. [n_rows, d] bool, True = kept. (oracle.mlp.dropout_keep
    restates the fused kernels' 16-bit hash, which this path does not use.)"""
    with np.errstate(over="ignore"):
        i = np.arange(n_rows * d, dtype=np.uint64)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (i + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return ~(u < np.float32(p)).reshape(n_rows, d)
