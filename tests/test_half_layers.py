"""The half-layer classifier (use_half_layers) without a GPU.

* The float64 restatement (tests/half_layers_cases.py) against the reference's own
  results (tests/golden/classifier_half*.npz, written by tools/make_half_layers_golden.py),
  with the bounds tests/test_classifier_oracle.py uses for the default architecture. The
  reference in float32 differs from itself in float64 by 2.7e-7 in the logits and by 3.3e-6 of
  a tensor's max in the worst gradient, far inside them.
* Layout and model: parameter count, the default plan's offsets inside the half plan,
  state-dict names / shapes / order, strict load, from_file (.pt, .onnx), the ONNX graph.
"""
import ctypes

import numpy as np
import pytest
import torch

import half_layers_cases as hc
from oracle import mlp as omlp


@pytest.fixture(scope="module")
def gold():
    return hc.load_gold()


@pytest.fixture(scope="module")
def inputs():
    return hc.golden_inputs()


@pytest.fixture(scope="module")
def model(inputs):
    from heybuddy.wakeword import WakeWordMLPModel
    m = WakeWordMLPModel(use_half_layers=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in inputs[0].items()}, strict=True)
    return m


# ------------------------------------------------- restatement vs fixture ----
def test_restatement_forward(gold, inputs):
    params, x, _, _ = inputs
    prob, z, _ = hc.forward(params, x)
    np.testing.assert_allclose(z, gold["logit"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(prob, gold["prob"], rtol=1e-5, atol=1e-6)


def test_restatement_loss_and_gradients(gold, inputs):
    params, x, y, _ = inputs
    loss, n, grads, _ = hc.step(params, x, y, neg_weight=2.0)
    assert n == int(gold["n_sel"])
    np.testing.assert_allclose(loss, float(gold["loss"]), rtol=1e-5)
    names = [k for k in params if f"grad/{k}" in gold]
    assert names == [k for k, v in params.items() if hc.stored(k, v.size)] and len(names) >= 6 * 16 + 2
    for k in names:
        ref = gold[f"grad/{k}"]
        scale = np.abs(ref).max() + 1e-12
        np.testing.assert_allclose(grads[k] / scale, ref / scale, rtol=0, atol=2e-5, err_msg=k)


def test_restatement_epoch(gold, inputs):
    params, _, _, batches = inputs
    final, hist = hc.train_epoch(params, batches, 24, 4, 8)
    assert len(hist["loss"]) == len(gold["epoch/loss"])
    np.testing.assert_allclose(hist["high_loss_rate"], gold["epoch/hlr"], rtol=1e-6)
    np.testing.assert_allclose(hist["loss"], gold["epoch/loss"], rtol=2e-4, atol=1e-6)
    assert 0 < sum(hist["updated"]) < 24  # the gate both skipped and fired
    names = [k for k in params if f"epoch_final/{k}" in gold]
    assert len(names) >= 6 * 16 + 2
    for k in names:
        np.testing.assert_allclose(final[k], gold[f"epoch_final/{k}"], rtol=0, atol=2e-4, err_msg=k)


def test_generic_dropout_mask_rate():
    keep = hc.generic_dropout_keep(5, 17)
    assert keep.shape == (17, 1536) and abs(1.0 - keep.mean() - 0.1) < 0.01
    assert not np.array_equal(keep, hc.generic_dropout_keep(6, 17))


# ------------------------------------------------------- layout and model ----
def test_param_count_and_default_offsets_unchanged():
    from heybuddy.kernels import MlpPlan
    half, plain = MlpPlan(half_layers=True), MlpPlan()
    assert plain.n_params == 256417 and half.n_params == hc.N_PARAMS == 256417 + 16 * 106208
    assert half.offsets == plain.offsets
    assert not half.fused and plain.fused
    # the bank follows the default block, branch after branch, every tensor one contiguous run
    assert half.half_offsets[0][0] == 256417
    assert [o[0] for o in half.half_offsets] == [256417 + 106208 * h for h in range(16)]
    flat = torch.arange(half.n_params, dtype=torch.float32)
    views = half.views(flat)
    assert sum(v.numel() for v in views.values()) == half.n_params
    assert all(v.is_contiguous() for v in views.values())
    firsts = sorted(int(v.reshape(-1)[0]) for v in views.values())
    assert firsts[0] == 0 and len(set(firsts)) == len(firsts)
    for k, v in plain.views(flat[:256417]).items():
        assert views[k].data_ptr() == v.data_ptr() and views[k].shape == v.shape, k


def test_plan_rejects_bad_half_geometry():
    from heybuddy import _native
    lib = _native.lib()
    idx = (ctypes.c_int32 * 128)(*[t for r in hc.HALF_INDICES for t in r])
    h = ctypes.c_void_p()
    assert lib.hbk_mlp_plan_create_half(1536, 96, 64, 2, 16, 16, idx, ctypes.byref(h)) == 0
    lib.hbk_mlp_plan_destroy(h)
    assert lib.hbk_mlp_plan_create_half(1540, 96, 64, 2, 16, 16, idx, ctypes.byref(h)) != 0
    assert b"divisible" in lib.hbk_last_error()
    assert lib.hbk_mlp_plan_create_half(1530, 96, 64, 2, 15, 16, idx, ctypes.byref(h)) != 0
    assert b"even" in lib.hbk_last_error()
    bad = (ctypes.c_int32 * 128)(*([16] + [0] * 127))
    assert lib.hbk_mlp_plan_create_half(1536, 96, 64, 2, 16, 16, bad, ctypes.byref(h)) != 0
    assert b"out of range" in lib.hbk_last_error()
    bad[0] = -1
    assert lib.hbk_mlp_plan_create_half(1536, 96, 64, 2, 16, 16, bad, ctypes.byref(h)) != 0


def test_state_dict_matches_the_reference(gold, inputs, model):
    names = [str(n) for n in gold["names"]]
    sd = model.state_dict()
    assert list(sd) == names == [n for n, _ in model.named_parameters()] == list(inputs[0])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(gold[f"shape/{k}"]), k
        np.testing.assert_array_equal(v.numpy(), inputs[0][k])  # the strict load went into the flat buffer
    assert model.flat_parameters.numel() == hc.N_PARAMS
    assert model.half_indices == hc.HALF_INDICES
    assert sorted(model.half_indices[14]) != model.half_indices[14]  # the lists, not the bit masks


def test_initialisation_and_argument_errors():
    from heybuddy.wakeword import WakeWordMLPModel
    m = WakeWordMLPModel(use_half_layers=True)
    sd = m.state_dict()
    assert float(sd["half_layers.3.0.weight"].min()) == 1.0 and float(sd["half_layers.3.0.bias"].abs().max()) == 0.0
    w = sd["half_layers.15.1.hidden.weight"]
    assert float(w.abs().max()) <= 768 ** -0.5 and float(w.std()) > 0.5 * 768 ** -0.5 / 3 ** 0.5
    assert float(sd["half_layers.15.1.output.weight"].abs().max()) <= 64 ** -0.5
    with pytest.raises(ValueError):
        WakeWordMLPModel(input_shape=(8, 96), use_half_layers=True)
    with pytest.raises(NotImplementedError):
        WakeWordMLPModel(use_half_layers=True, use_gating=False)
    with pytest.raises(NotImplementedError):
        WakeWordMLPModel(use_half_layers=True, activation="relu")
    assert WakeWordMLPModel().half_indices == []


def test_from_file_detects_half_layers_and_onnx_round_trips(model, tmp_path):
    from heybuddy.util.onnx_util import read_initializers, read_model, read_nodes
    from heybuddy.wakeword import WakeWordMLPModel
    pt, onnx = str(tmp_path / "h.pt"), str(tmp_path / "h.onnx")
    torch.save(model.state_dict(), pt)
    model.save_onnx(onnx)
    for path in (pt, onnx):
        m = WakeWordMLPModel.from_file(path)
        assert m.use_half_layers and m.num_layers == 2 and m.layer_dim == 96
        for (k, a), (k2, b) in zip(model.state_dict().items(), m.state_dict().items()):
            assert k == k2 and torch.equal(a, b), k
    plain = str(tmp_path / "p.onnx")
    WakeWordMLPModel().save_onnx(plain)
    assert not WakeWordMLPModel.from_file(plain).use_half_layers
    assert not any(op == "Gather" for op, _, _ in read_nodes(plain))
    # the graph: 16 Gather (axis 1) -> Flatten -> LayerNormalization -> gated MLP -> Add
    nodes = read_nodes(onnx)
    inits = read_initializers(onnx)
    gathers = [n for n in nodes if n[0] == "Gather"]
    assert len(gathers) == 16
    assert [inits[ins[1]].tolist() for _, ins, _ in gathers] == hc.HALF_INDICES
    assert all(ins[0] == "input" and inits[ins[1]].dtype == np.int64 for _, ins, _ in gathers)
    g = read_model(onnx)
    assert all(n.attrs["axis"] == 1 for n in g.nodes if n.op == "Gather")
    state = g.producer([n for n in g.nodes if n.op == "LayerNormalization"][17].inputs[0])  # layers.0.0 reads the sum
    assert state.op == "Add"
    for h, (_, _, outs) in enumerate(gathers):
        flat, = g.consumers(outs[0])
        ln, = g.consumers(flat.outputs[0])
        assert (flat.op, ln.op) == ("Flatten", "LayerNormalization") and ln.inputs[1] == f"half_layers.{h}.0.weight"
    assert sum(n.op == "Add" for n in g.nodes) == 16 and sum(n.op == "Gemm" for n in g.nodes) == 3 * (4 + 16)


def test_onnx_graph_computes_the_restatement(model, inputs, tmp_path):
    """The written graph, evaluated node by node in numpy, gives the restatement's probability."""
    from heybuddy.util.onnx_util import read_model
    path = str(tmp_path / "h.onnx")
    model.save_onnx(path)
    g = read_model(path)
    x = inputs[1][:1].astype(np.float64)
    val = {k: v.astype(np.float64) if v.dtype.kind == "f" else v for k, v in g.initializers.items()}
    val["input"] = x
    for n in g.nodes:
        a = [val[i] for i in n.inputs]
        if n.op == "Gather":
            r = np.take(a[0], a[1], axis=n.attrs["axis"])
        elif n.op == "Flatten":
            r = a[0].reshape(a[0].shape[0], -1)
        elif n.op == "LayerNormalization":
            r = omlp._ln(a[0], a[1], a[2])[0]
        elif n.op == "Gemm":
            r = a[0] @ a[1].T + a[2]
        elif n.op == "Sigmoid":
            r = 1.0 / (1.0 + np.exp(-a[0]))
        elif n.op == "Mul":
            r = a[0] * a[1]
        else:
            assert n.op == "Add", n.op
            r = a[0] + a[1]
        val[n.outputs[0]] = r
    prob, _, _ = hc.forward(inputs[0], inputs[1][:1])
    np.testing.assert_allclose(val["output"][:, 0], prob, rtol=1e-12)
