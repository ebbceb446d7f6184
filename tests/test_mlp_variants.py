"""The plain MLP (use_gating=False) and the non-SiLU activations without a GPU.

* The float64 restatement (tests/mlp_variants_cases.py) against the reference's own results
  (tests/golden/classifier_variants_*.npz, written by tools/make_mlp_variants_golden.py) for all
  13 variants, with the bounds tests/test_half_layers.py uses. The reference in float32 differs
  from itself in float64 by at most 1.4e-6 in the logits and 3.0e-6 of a tensor's max in the
  worst gradient over the 13 variants.
* Plans and layouts (host-only): parameter counts, the default plan unchanged, views.
* Model and files: state dict, strict load, from_file (.pt, .onnx), the ONNX graphs.
"""
import ctypes

import numpy as np
import pytest
import torch

import mlp_variants_cases as vc

VARIANTS = pytest.mark.parametrize("gated,act", vc.VARIANTS, ids=[vc.key(g, a) for g, a in vc.VARIANTS])
EPOCH_VARIANTS = pytest.mark.parametrize("gated,act", vc.EPOCH_VARIANTS,
                                         ids=[vc.key(g, a) for g, a in vc.EPOCH_VARIANTS])


@pytest.fixture(scope="module")
def gold():
    return vc.load_gold()


def _model(gated, act, params=None):
    from heybuddy.wakeword import WakeWordMLPModel
    m = WakeWordMLPModel(use_gating=gated, activation=act)
    if params is not None:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m


# ------------------------------------------------- restatement vs fixture ----
def test_the_fixture_holds_the_13_variants(gold):
    assert len(vc.VARIANTS) == 13 and (True, "silu") not in vc.VARIANTS
    assert sorted({k.split("/", 1)[0] for k in gold}) == sorted(vc.key(g, a) for g, a in vc.VARIANTS)
    assert sorted(k.split("/", 1)[0] for k in gold if k.endswith("/epoch/loss")) == \
        sorted(vc.key(g, a) for g, a in vc.EPOCH_VARIANTS)


@VARIANTS
def test_restatement_forward_loss_and_gradients(gold, gated, act):
    g = vc.variant_gold(gold, gated, act)
    params, x, y, _ = vc.golden_inputs(gated)
    loss, n, grads, prob = vc.step(params, x, y, gated, act, neg_weight=2.0)
    _, z, _ = vc.forward(params, x, gated, act)
    np.testing.assert_allclose(z, g["logit"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(prob, g["prob"], rtol=1e-5, atol=1e-6)
    assert n == int(g["n_sel"]) == 96  # (the filter keeps every row at threshold 1e-4)
    np.testing.assert_allclose(loss, float(g["loss"]), rtol=1e-5)
    names = [k for k in params if f"grad/{k}" in g]
    assert names == [k for k, v in params.items() if vc.stored(k, v.size)]
    assert set(vc.STORED_BIG) <= set(names) and len(names) == (23 if gated else 19)
    for k in names:
        ref = g[f"grad/{k}"]
        scale = np.abs(ref).max() + 1e-12
        np.testing.assert_allclose(grads[k] / scale, ref / scale, rtol=0, atol=2e-5, err_msg=k)


@EPOCH_VARIANTS
def test_restatement_epoch(gold, gated, act):
    g = vc.variant_gold(gold, gated, act)
    params, _, _, batches = vc.golden_inputs(gated)
    final, hist = vc.train_epoch(params, batches, 24, 4, 8, gated, act)
    assert len(hist["loss"]) == len(g["epoch/loss"])
    np.testing.assert_allclose(hist["high_loss_rate"], g["epoch/hlr"], rtol=1e-6)
    np.testing.assert_allclose(hist["loss"], g["epoch/loss"], rtol=2e-4, atol=1e-6)
    assert 0 < sum(hist["updated"]) < 24  # the gate both skipped and fired
    names = [k for k in params if f"epoch_final/{k}" in g]
    assert names == [k for k, v in params.items() if vc.stored(k, v.size)]
    for k in names:
        np.testing.assert_allclose(final[k], g[f"epoch_final/{k}"], rtol=0, atol=2e-4, err_msg=k)


# ------------------------------------------------------- plans and layouts ----
def test_param_counts_and_the_default_plan_unchanged():
    from heybuddy.kernels import MlpPlan
    default, plain = MlpPlan(), MlpPlan(gated=False)
    assert default.n_params == 256417 and default.fused is True
    assert plain.n_params == 139425 and plain.fused is False
    # the default plan's offsets, as hbk_mlp_plan_create laid them out before there were variants
    H, D, L = 64, 1536, 96
    want, o = [0, D], 2 * D
    lns = []
    for k, (din, dout) in enumerate([(D, L), (L, L), (L, L), (L, 1)]):
        if k > 0:
            lns += [o, o + L]
            o += 2 * L
        want += [o, o + 2 * H * din, o + 2 * H * din + 2 * H, o + 2 * H * din + 2 * H + dout * H]
        o += 2 * H * din + 2 * H + dout * H + dout
    assert default.offsets == want + lns and o == 256417
    assert MlpPlan(gated=True, activation="swish").offsets == default.offsets
    # a plain plan: the same order without the gate rows
    want, o, lns = [0, D], 2 * D, []
    for k, (din, dout) in enumerate([(D, L), (L, L), (L, L), (L, 1)]):
        if k > 0:
            lns += [o, o + L]
            o += 2 * L
        want += [o, o + H * din, o + H * din + H, o + H * din + H + dout * H]
        o += H * din + H + dout * H + dout
    assert plain.offsets == want + lns and o == 139425


@VARIANTS
def test_non_default_plans_are_not_fused_and_their_views_tile_the_buffer(gold, gated, act):
    from heybuddy.kernels import MlpPlan
    plan = MlpPlan(gated=gated, activation=act)
    assert plan.fused is False and plan.n_params == vc.N_PARAMS[gated]
    flat = torch.arange(plan.n_params, dtype=torch.float32)  # (exact below 2^24)
    views = plan.views(flat)
    assert all(v.is_contiguous() for v in views.values())
    covered = np.zeros(plan.n_params, dtype=np.int64)
    for v in views.values():
        first = int(v.reshape(-1)[0])
        covered[first:first + v.numel()] += 1
    assert (covered == 1).all()  # every float in exactly one view
    g = vc.variant_gold(gold, gated, act)
    assert list(views) == [str(n) for n in g["names"]]
    assert any(".gate." in k for k in views) == gated
    plan.workspace_bytes(1100)  # (host-only: the generic layout covers the plan)


@VARIANTS
def test_state_dict_matches_the_reference(gold, gated, act):
    g = vc.variant_gold(gold, gated, act)
    params = vc.golden_inputs(gated)[0]
    m = _model(gated, act, params)  # strict load
    names = [str(n) for n in g["names"]]
    sd = m.state_dict()
    assert list(sd) == names == [n for n, _ in m.named_parameters()] == list(params)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(g[f"shape/{k}"]), k
        np.testing.assert_array_equal(v.numpy(), params[k])  # the load went into the flat buffer
    assert m.flat_parameters.numel() == vc.N_PARAMS[gated]
    assert m.use_gating == gated and m.activation == act and hasattr(m.mlp_in, "gate") == gated


def test_activation_names_and_initialisation():
    from heybuddy.wakeword import WakeWordMLPModel
    assert WakeWordMLPModel(activation="swish").activation == "silu"
    assert WakeWordMLPModel(activation="swish").plan.fused
    m = WakeWordMLPModel(use_gating=False, activation=None)
    assert m.activation == "identity" and not m.plan.fused
    sd = m.state_dict()
    assert float(sd["layers.0.0.weight"].min()) == 1.0 and float(sd["norm_out.bias"].abs().max()) == 0.0
    w = sd["mlp_in.hidden.weight"]
    assert float(w.abs().max()) <= 1536 ** -0.5 and float(w.std()) > 0.5 * 1536 ** -0.5 / 3 ** 0.5
    assert float(sd["mlp_out.output.weight"].abs().max()) <= 64 ** -0.5


# --------------------------------------------------------- model and files ----
def test_from_file_infers_a_plain_checkpoint(tmp_path):
    from heybuddy.wakeword import WakeWordMLPModel
    m = _model(False, "silu", vc.golden_inputs(False)[0])
    path = str(tmp_path / "plain.pt")
    torch.save(m.state_dict(), path)
    back = WakeWordMLPModel.from_file(path)
    assert back.use_gating is False and back.activation == "silu" and back.num_layers == 2
    assert torch.equal(back.flat_parameters, m.flat_parameters)
    assert WakeWordMLPModel.from_file(path, activation="relu").activation == "relu"
    gated = str(tmp_path / "gated.pt")
    torch.save(WakeWordMLPModel().state_dict(), gated)
    assert WakeWordMLPModel.from_file(gated).use_gating is True


@pytest.mark.parametrize("gated,act", vc.VARIANTS + [(True, "silu")],
                         ids=[vc.key(g, a) for g, a in vc.VARIANTS + [(True, "silu")]])
def test_onnx_round_trip_graph_and_values(gated, act, tmp_path):
    from heybuddy.util.onnx_util import ACTIVATION_OPS, read_model
    from heybuddy.wakeword import WakeWordMLPModel
    params, x, _, _ = vc.golden_inputs(gated)
    m = _model(gated, act, params)
    path = str(tmp_path / "v.onnx")
    m.save_onnx(path)
    back = WakeWordMLPModel.from_file(path)
    assert back.use_gating == gated and back.activation == act and back.num_layers == 2
    for (k, a), (k2, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    g = read_model(path)
    assert g.opset == 19
    block = list(("Gemm",) + ACTIVATION_OPS[act] + (("Gemm", "Mul", "Gemm") if gated else ("Gemm",)))
    want = ["Flatten"] + (["LayerNormalization"] + block) * 4 + ["Sigmoid"]
    assert [n.op for n in g.nodes] == want
    spec = {"relu": ("Relu",), "tanh": ("Tanh",), "sigmoid": ("Sigmoid",), "silu": ("Sigmoid", "Mul"),
            "mish": ("Softplus", "Tanh", "Mul"), "gelu": ("Div", "Erf", "Add", "Mul", "Mul"), "identity": ()}
    assert tuple(n.op for n in g.nodes if n.name.startswith("/layers.1/layers.1.1/activation/")) == spec[act]
    assert len({n.name for n in g.nodes}) == len(g.nodes)
    assert sum(".gate." in i for n in g.nodes for i in n.inputs) == (8 if gated else 0)
    # the written graph computes the restatement
    prob, _, _ = vc.forward(params, x[:5], gated, act)
    np.testing.assert_allclose(vc.onnx_eval(g, x[:5])[:, 0], prob, rtol=0, atol=1e-6)


def test_the_default_onnx_file_is_unchanged(tmp_path):
    """Two writes of the default path give the same bytes, and they are the bytes of the graph as it
    was written before the writer learnt the variants: its nodes, names and initializer order."""
    from heybuddy.util.onnx_util import read_model, write_wakeword_onnx
    from heybuddy.wakeword import WakeWordMLPModel
    params = vc.golden_inputs(True)[0]
    m = _model(True, "silu", params)
    a, b = str(tmp_path / "a.onnx"), str(tmp_path / "b.onnx")
    m.save_onnx(a)
    write_wakeword_onnx(b, params, 2)  # the call as it was before gated / activation existed
    assert open(a, "rb").read() == open(b, "rb").read()
    g = read_model(a)
    assert list(g.initializers) == list(params)  # no constants, no indices
    first = [(n.op, n.name) for n in g.nodes[:8]]
    assert first == [("Flatten", "/flatten/Flatten"), ("LayerNormalization", "/norm_in/LayerNormalization"),
                     ("Gemm", "/mlp_in/hidden/Gemm"), ("Sigmoid", "/mlp_in/activation/Sigmoid"),
                     ("Mul", "/mlp_in/activation/Mul"), ("Gemm", "/mlp_in/gate/Gemm"), ("Mul", "/mlp_in/Mul"),
                     ("Gemm", "/mlp_in/output/Gemm")]
    assert g.nodes[4].inputs == ("/mlp_in/hidden/Gemm_output_0", "/mlp_in/activation/Sigmoid_output_0")
    assert WakeWordMLPModel.from_file(a).plan.fused


# ------------------------------------------------------------------ errors ----
def test_unknown_activation_raises_the_reference_error():
    from heybuddy.kernels import MlpPlan
    from heybuddy.wakeword import WakeWordMLPModel
    for bad in ("leaky", "SiLU", ""):
        with pytest.raises(ValueError, match=f"Activation function '{bad}' not found."):
            WakeWordMLPModel(activation=bad)
    with pytest.raises(ValueError, match="not found"):
        MlpPlan(activation="softmax")


def test_plan_create_ex_argument_errors():
    from heybuddy import _native
    lib = _native.lib()
    h = ctypes.c_void_p()
    for code in range(7):
        assert lib.hbk_mlp_plan_create_ex(1536, 96, 64, 2, 0, code, ctypes.byref(h)) == 0
        n = ctypes.c_int64()
        assert lib.hbk_mlp_layout(h, ctypes.byref(n), None, 0) == 0 and n.value == 139425
        lib.hbk_mlp_plan_destroy(h)
    for code in (-1, 7, 100):
        assert lib.hbk_mlp_plan_create_ex(1536, 96, 64, 2, 1, code, ctypes.byref(h)) == -1  # HBK_ERR_ARG
        assert b"activation" in lib.hbk_last_error() and not h
    assert lib.hbk_mlp_plan_create_ex(1536, 96, 64, 2, 2, 0, ctypes.byref(h)) == -1
    assert b"gated" in lib.hbk_last_error()
    assert lib.hbk_mlp_plan_create_ex(1536, 96, 0, 2, 0, 0, ctypes.byref(h)) == -1
    # the activation entry points check their arguments before any launch
    assert lib.hbk_mlp_act_forward(None, 4, 8, 1, 7, None, None) == -1
    assert b"activation" in lib.hbk_last_error()
    assert lib.hbk_mlp_act_forward(None, 4, 0, 1, 0, None, None) == -1
    assert lib.hbk_mlp_act_forward(None, 4, 8, 1, 0, None, None) == -1
    assert b"NULL" in lib.hbk_last_error()
    assert lib.hbk_mlp_act_backward(None, None, 4, 8, 0, 3, None, None) == -1
    assert lib.hbk_mlp_act_forward(None, 0, 8, 1, 0, None, None) == 0  # no rows: nothing to do


def test_half_layers_stay_gated_silu_only():
    """The ABI has no constructor that combines the bank with a plain block or another activation:
    hbk_mlp_plan_create_half builds gated SiLU, and the Python layers refuse the combination."""
    from heybuddy.kernels import MlpPlan
    from heybuddy.wakeword import WakeWordMLPModel
    half = MlpPlan(half_layers=True)
    assert half.gated and half.activation == "silu" and half.n_params == 256417 + 16 * 106208
    for kw in ({"gated": False}, {"activation": "relu"}):
        with pytest.raises(ValueError, match="half layers"):
            MlpPlan(half_layers=True, **kw)
    with pytest.raises(NotImplementedError):
        WakeWordMLPModel(use_half_layers=True, use_gating=False)
    with pytest.raises(NotImplementedError):
        WakeWordMLPModel(use_half_layers=True, activation="gelu")
