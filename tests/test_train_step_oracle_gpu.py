"""The fused train step against the float64 oracle (oracle/mlp.py), per variant (v1: k1a /
k1b / k3 on the whole GPU; v2: k1s / k1c / k3s on the 64-CU train partition, the library's
own choice from 800 rows; generic: hbk_mlp_train_fwd_bwd on gathered rows), with the
high-loss filter REJECTING rows: every other classifier test selects every row.

Inputs (tests/step_oracle_cases.py; seeded, nothing stored): 6,000 candidates, 1,401
positives in an f32 pool and 4,599 negatives in an f16 pool; the golden parameters P0
(every row selected) and the "wide" parameters Q (output weight x 120, median logit 0).
Under Q the candidates classify as U (filtered, >= 0.25 logits past its threshold) 1,308
= 1,018 negatives + 290 positives, S (kept, 0.05 <= |z| <= 6) 2,199 = 1,680 + 519; rows
of neither class are never used, and every precondition (counts >= 1,000, the margins,
n_sel, the gate's skips and fires) is asserted on the oracle before any GPU call.

Single-step layouts (rows addressed by idx into the two pools):
  dense-1100          P0  rows of any kind, every row selected
  zero-rows-1100      P0  dense, rows 5 / 600 / 1099 with idx = n32, 2^31 - 1, -n16 - 1 (out of
                          range: "reads as a zero row"; the oracle gets zero rows), label 0
  zero-rows-f16-1100  P0  negatives only, pool32 = NULL, out-of-range rows idx = 0, 2^31 - 1,
                          -n16 - 1 (k1a_tile's pool16 fallback)
  sparse-1100         Q   rows 0-127 filtered (a whole k3s split, eight whole tiles), 128-143
                          filtered but row 135, 144-655 a seeded 50/50 mix, 656-1087 kept,
                          1088-1099 filtered (the ragged tail tile); n_sel = 662
  few-801             Q   701 filtered rows, then 100 kept (n_sel = 100 < 128); Bp = 816, the
                          last tile holds one live row, which is selected
  none-800            Q   800 filtered rows: n_sel = 0
  dropout-1100        P0  dense with dropout 0.1: the oracle's input is x * dropout_keep(seed +
                          step + (salt << 24), arange(B)) / 0.9 (step 0, salt 0)
The generic path runs neither the zero-row layouts (it takes gathered rows: no indices,
no pools) nor dropout-1100: by reading, hbk_mlp.hip draws its mask from uniform01
(splitmix64), not from the fused kernels' drop_hash that oracle.mlp.dropout_keep restates.

Bounds (the project's, tests/test_mlp_fused_gpu.py): counts exact, loss sum 1e-5 relative,
prob 1e-6 + 1e-4 relative, every gradient tensor within 1e-4 of its max |g_ref|. Headroom,
a float32 numpy restatement of the step against the float64 one, per layout (worst gradient
tensor as a share of its max |g_ref| / loss sum relative / prob absolute):
  dense-1100 2.0e-6 / 3e-9 / 1.9e-7     zero-rows-1100 1.8e-6 / 9e-9 / 1.9e-7
  zero-rows-f16-1100 1.9e-6 / 8e-8 / 2.1e-7   sparse-1100 3.9e-6 / 4e-7 / 1.1e-5
  few-801 6.5e-6 / 1e-6 / 9.1e-6        none-800 0 / 0 / 6e-8    dropout-1100 1.9e-6 / 9e-10 / 1.5e-7
so the bounds leave 15-50 x for the summation order (prob under Q: 4 x at p = 0.5).

Gated multi-step test: six train_indexed steps from Q at B = 800 (200 f32 positives, then
600 f16 negatives), lr 2e-4, neg_weight 1.5, dropout off, 4 steps per graph. The float64
walk classifies the candidates under its CURRENT parameters before each step and composes
the rows for n_sel = 60, 60, 40, 0, 300, 90: the gate skips, skips, fires (160 samples, 3
accumulation steps), sees no row, fires, skips. History counts, accumulation steps and
fired flags are exact, the loss within 2e-4 (the multi-step bound). Parameters and Adam's m
have no derivable bound (a gradient at the f32 noise floor flips the sign of an lr-sized
step), so a float32 walk of the same oracle over the same rows was measured against the
float64 one on the CPU:
  (a) share of parameters differing by > 1e-5: 2.73e-5 (7 of 256,417)
  (b) |dP - dP_ref|_2 / |dP_ref|_2, dP = P_final - P_init: 2.48e-3
  (c) per tensor max |m - m_ref| / max |m_ref|: GATED_M_F32 below (4.5e-6 .. 8.7e-4)
and the device must stay within 4 x each (its summation order is not numpy's), and within
max |P - P_ref| <= 2 sum(lr of the fired steps) = 8e-4 (the f32 walk: 3.8e-4).
"""
import numpy as np
import pytest
import torch

import step_oracle_cases as sc

pytestmark = pytest.mark.gpu

GATED_SHARE_F32, GATED_DRIFT_F32 = 2.73e-5, 2.49e-3
GATED_M_F32 = {
    "norm_in.weight": 7.1e-4, "norm_in.bias": 8.8e-4, "mlp_in.hidden.weight": 4.3e-4,
    "mlp_in.hidden.bias": 5.0e-4, "mlp_in.output.weight": 3.5e-4, "mlp_in.output.bias": 2.4e-4,
    "mlp_in.gate.weight": 7.0e-4, "mlp_in.gate.bias": 2.5e-4, "layers.0.0.weight": 2.5e-4,
    "layers.0.0.bias": 2.2e-4, "layers.0.1.hidden.weight": 5.5e-4, "layers.0.1.hidden.bias": 3.0e-4,
    "layers.0.1.output.weight": 2.3e-4, "layers.0.1.output.bias": 1.2e-4, "layers.0.1.gate.weight": 2.6e-4,
    "layers.0.1.gate.bias": 2.4e-4, "layers.1.0.weight": 2.6e-4, "layers.1.0.bias": 1.3e-4,
    "layers.1.1.hidden.weight": 1.6e-4, "layers.1.1.hidden.bias": 9.5e-5, "layers.1.1.output.weight": 3.2e-4,
    "layers.1.1.output.bias": 9.4e-5, "layers.1.1.gate.weight": 1.4e-4, "layers.1.1.gate.bias": 9.2e-5,
    "norm_out.weight": 9.3e-5, "norm_out.bias": 1.2e-4, "mlp_out.hidden.weight": 2.0e-4,
    "mlp_out.hidden.bias": 1.4e-4, "mlp_out.output.weight": 1.8e-4, "mlp_out.output.bias": 4.5e-6,
    "mlp_out.gate.weight": 1.5e-4, "mlp_out.gate.bias": 8.2e-5,
}

FUSED_LAYOUTS = ("dense-1100", "zero-rows-1100", "zero-rows-f16-1100", "sparse-1100", "few-801", "none-800",
                 "dropout-1100")
GENERIC_LAYOUTS = ("dense-1100", "sparse-1100", "few-801", "none-800")
CASES = [(v, n) for v in ("v1", "v2") for n in FUSED_LAYOUTS] + [("generic", n) for n in GENERIC_LAYOUTS]


@pytest.fixture(scope="module")
def layouts():
    return sc.layouts()


@pytest.fixture(scope="module")
def dev():
    """The pools on the device, one model per parameter set, the 64-CU train stream."""
    from heybuddy.pipeline import masked_stream, train_cu_set
    from heybuddy.wakeword import WakeWordMLPModel
    w = sc.world()
    models = {}
    for name, params in (("P0", w.P0), ("Q", w.Q)):
        m = WakeWordMLPModel()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        m.dropout.p = 0.0
        models[id(params)] = m.cuda()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ms = masked_stream(torch.device("cuda", 0), train_cu_set(n_cu, 64))
    return {"pool32": torch.from_numpy(w.pool32.copy()).cuda(), "pool16": torch.from_numpy(w.pool16.copy()).cuda(),
            "models": models, "ms": ms}


def _on_variant_stream(dev, variant, fn):
    """fn() on the default stream (v1, generic) or on the 64-CU masked stream (v2)."""
    if variant != "v2":
        out = fn()
    else:
        ms = dev["ms"]
        ms.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(ms.stream):
            out = fn()
    torch.cuda.synchronize()
    return out


def _run_step(dev, variant, lay, stale_workspace=False):
    """One step of ``lay`` through ``variant``: (model, bucket, prob, state) on the device."""
    m = dev["models"][id(lay.params)]
    plan, flat, B = m.plan, m.flat_parameters, lay.B
    bucket = torch.zeros(plan.n_params + plan.N_STATS, device="cuda")
    prob = torch.zeros(B, device="cuda")
    state = plan.new_state("cuda")
    y = torch.from_numpy(lay.y.astype(np.float32)).cuda()
    ws = None
    if stale_workspace:  # NaN bits in f32 and f16: nothing may depend on what the workspace held
        ws = torch.full((plan.workspace_bytes(B),), 0xFF, dtype=torch.uint8, device="cuda")

    def go():
        if variant == "generic":
            x = torch.from_numpy(lay.x).cuda()
            plan.train_fwd_bwd(flat, x, y, bucket, neg_weight=sc.NEG_WEIGHT, prob=prob, workspace=ws)
            return
        assert plan.step_variant(B, "cuda") == (2 if variant == "v2" else 1)
        idx = torch.from_numpy(lay.idx).cuda()
        plan.step_fwd_bwd(flat, bucket, state, 0, y, B, pool32=dev["pool32"] if lay.pool32 else None,
                          pool16=dev["pool16"], idx=idx, idx_stride=B, neg_weight=sc.NEG_WEIGHT,
                          dropout_p=sc.DROP_P if lay.dropout else 0.0, seed=sc.DROP_SEED, prob=prob, workspace=ws)

    _on_variant_stream(dev, variant, go)
    return m, bucket, prob, state


def _check(lay, m, bucket, prob):
    plan = m.plan
    grads = {k: v.cpu().numpy() for k, v in plan.views(bucket[:plan.n_params]).items()}
    sc.check_bucket(lay, grads, bucket[plan.n_params:].cpu().numpy(), prob.cpu().numpy())


@pytest.mark.parametrize("variant,name", CASES, ids=[f"{v}-{n}" for v, n in CASES])
def test_step_matches_oracle(variant, name, layouts, dev):
    """Counts exact, loss 1e-5, prob 1e-6 + 1e-4, every gradient tensor 1e-4 of its max."""
    lay = layouts[name]
    m, bucket, prob, _ = _run_step(dev, variant, lay)
    _check(lay, m, bucket, prob)
    if name == "none-800":
        b = bucket.cpu().numpy()
        assert not b[:m.plan.n_params].any()
        np.testing.assert_array_equal(b[m.plan.n_params:], [0, 0, 0, 0, 0, 0, 800, 0])


@pytest.mark.parametrize("variant", ["v1", "v2", "generic"])
def test_no_selected_row_leaves_the_parameters_alone(variant, layouts, dev):
    """none-800, then the update with nothing accumulated: the gate does not fire, and the
    parameters and Adam's m and v keep their bits."""
    lay = layouts["none-800"]
    m, bucket, _, state = _run_step(dev, variant, lay)
    plan = m.plan
    g = torch.Generator().manual_seed(3)
    flat = m.flat_parameters.clone()
    mm = (1e-3 * torch.randn(plan.n_params, generator=g)).cuda()
    vv = (1e-6 * torch.rand(plan.n_params, generator=g)).cuda()
    before = [t.clone() for t in (flat, mm, vv)]
    hist = torch.zeros((1, 8), device="cuda")
    state[0] = 0.0
    _on_variant_stream(dev, variant, lambda: plan.step_update(flat, bucket, mm, vv, state, 0, lr=1e-3, history=hist))
    for t, b in zip((flat, mm, vv), before):
        assert bool(torch.isfinite(t).all())
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))
    np.testing.assert_array_equal(hist.cpu().numpy()[0], [0, 1, 0, 0, 0, 0, 0, 0])


@pytest.mark.parametrize("name", ["sparse-1100", "few-801"])
@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_step_does_not_depend_on_the_workspace_contents(variant, name, layouts, dev):
    """The same bounds from a workspace of 0xFF bytes and no *_ready flag; all finite. (By
    reading: k1s writes rinfo and mask for all Bp rows in the same call and k1c / k3s clamp
    their row to B - 1, so no address comes from unwritten memory.)"""
    lay = layouts[name]
    m, bucket, prob, _ = _run_step(dev, variant, lay, stale_workspace=True)
    assert bool(torch.isfinite(bucket).all()) and bool(torch.isfinite(prob).all())
    _check(lay, m, bucket, prob)


@pytest.fixture(scope="module")
def gated():
    return sc.gated_walk()


@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_gated_steps_match_oracle(variant, gated, dev, tmp_path):
    from heybuddy.trainer import WakeWordTrainer
    w = sc.world()
    S, B = gated["rows"].shape
    tr = WakeWordTrainer(checkpoint_dir=str(tmp_path), device="cuda")
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.Q.items()}, strict=True)
    tr.model.dropout.p = 0.0
    tr._reset_accumulation()
    plan = tr.model.plan
    idx = torch.from_numpy(w.idx[gated["rows"]].copy()).cuda()
    assert bool((idx[:, :sc.GATED_POS] >= 0).all()) and bool((idx[:, sc.GATED_POS:] < 0).all())
    y = torch.from_numpy(gated["y"].astype(np.float32)).cuda()
    sched = torch.tensor([[sc.GATED_LR, sc.NEG_WEIGHT]] * S, dtype=torch.float32, device="cuda")
    hist = torch.zeros((S, 8), device="cuda")

    def go():
        assert plan.step_variant(B, "cuda") == (2 if variant == "v2" else 1)
        tr.train_indexed(idx, y, sched, pool32=dev["pool32"], pool16=dev["pool16"], history=hist,
                         steps_per_graph=4)

    _on_variant_stream(dev, variant, go)
    h, ref = hist.cpu().numpy().astype(np.float64), gated["hist"]
    print("n_sel", h[:, 0], "acc_steps", h[:, 1], "fired", h[:, 2])
    np.testing.assert_array_equal(h[:, [0, 1, 2, 4, 5, 6, 7]], ref[:, [0, 1, 2, 4, 5, 6, 7]])
    print("loss rel err", np.abs(h[:, 3] - ref[:, 3]) / np.maximum(ref[:, 3], 1e-30))
    np.testing.assert_allclose(h[:, 3], ref[:, 3], rtol=2e-4)
    params = {k: v.detach().cpu().numpy() for k, v in plan.views(tr.model.flat_parameters).items()}
    m = {k: v.cpu().numpy() for k, v in plan.views(tr._m).items()}
    assert all(np.isfinite(v).all() for v in params.values())
    f = sc.gated_figures(params, m, gated)
    print(f"share {f['share']:.3e} (f32 walk {GATED_SHARE_F32:.2e}), drift {f['drift']:.3e} (f32 walk "
          f"{GATED_DRIFT_F32:.2e}), max |P - P_ref| {f['max']:.3e}")
    print("m:", {k: f"{v:.1e}" for k, v in f["m"].items()})
    assert f["max"] <= 2 * sum(gated["fired_lr"])
    assert f["share"] <= 4 * GATED_SHARE_F32
    assert f["drift"] <= 4 * GATED_DRIFT_F32
    for k, v in f["m"].items():
        assert v <= 4 * GATED_M_F32[k], f"{k}: max |m - m_ref| = {v:.2e} of max |m_ref| (f32 walk {GATED_M_F32[k]:.1e})"
