"""The v2 train step's live-tile walk (k3s lists the 16-row tiles that hold a row the high-loss
filter kept, and its splits share only those) against the float64 oracle (oracle/mlp.py).

Yardstick and bounds: those of tests/test_train_step_oracle_gpu.py (its docstring derives
them): counts exact, loss sum 1e-5 relative, prob 1e-6 + 1e-4 relative, every gradient
tensor within 1e-4 of its max |g_ref|; where the oracle's gradient is exactly zero the
device's must be. Everything runs on the 64-CU masked train stream with step_variant
asserted to be 2. Layouts (tests/step_sparse_cases.py; live rows from S, the rest from U,
on the wide parameters Q):

  none-1100                      n_sel = 0: the bucket stays zero, the update does not fire
  one-front-1100                 one live row (3) in tile 0
  one-tail-1100, one-tail-273    one live row in the last, partial tile
  first-32 / first-33            two / three live tiles: the 32-row step boundary
  first-160 / 161, 384 / 385     the compiled split lengths of the two k3s jobs at B = 1,100
                                 (5 and 12 steps of 32 rows) and one row more
  odd-tiles-1100                 live rows only in the odd tiles (every third row of them)
  all-1100                       every row live: the tensors k3s computes have the bits of the
                                 dense path (HBK_STEP_DENSE=1, read once per process: a child)
  ends-17, tail-17, scattered-800   the variant thresholds (B = 17 forced by HBK_STEP=2 in a
                                 child, as one-tail-273; B = 800 is the library's own choice)
  one-tail-1100 and odd-tiles-1100 again from a workspace of 0xFF bytes
and the six gated train_indexed steps of step_oracle_cases.gated_walk (n_sel = 60, 60, 40, 0,
300, 90: live -> none -> live) captured as ONE graph of six steps, with the bounds of
test_gated_steps_match_oracle: a replayed graph has to pick each step's live tiles up from
device memory.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import step_oracle_cases as sc
import step_sparse_cases as sp
from test_train_step_oracle_gpu import (GATED_DRIFT_F32, GATED_M_F32, GATED_SHARE_F32, _check, _on_variant_stream,
                                        _run_step)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "step_sparse_worker.py")
# the tensors k3s computes (plain stores into slabs, summed in a fixed order: the same bits from
# run to run); every other gradient is k2's float atomics
K3S_TENSORS = ("norm_in.weight", "norm_in.bias", ".hidden.weight", ".gate.weight", ".output.weight")

IN_PROCESS = ("none-1100", "one-front-1100", "one-tail-1100", "first-32-1100", "first-33-1100",
              f"first-{sp.K3S_R[0]}-1100", f"first-{sp.K3S_R[0] + 1}-1100", f"first-{sp.K3S_R[1]}-1100",
              f"first-{sp.K3S_R[1] + 1}-1100", "odd-tiles-1100", "all-1100", "scattered-800")
FORCED = ("one-tail-273", "ends-17", "tail-17")


@pytest.fixture(scope="module")
def layouts():
    return sp.layouts()


@pytest.fixture(scope="module")
def dev():
    """The pools on the device, the model on Q, the 64-CU train stream."""
    from heybuddy.pipeline import masked_stream, train_cu_set
    from heybuddy.wakeword import WakeWordMLPModel
    w = sc.world()
    m = WakeWordMLPModel()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.Q.items()}, strict=True)
    m.dropout.p = 0.0
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ms = masked_stream(torch.device("cuda", 0), train_cu_set(n_cu, 64))
    return {"pool32": torch.from_numpy(w.pool32.copy()).cuda(), "pool16": torch.from_numpy(w.pool16.copy()).cuda(),
            "models": {id(w.Q): m.cuda()}, "ms": ms}


def _child(tmp_path_factory, mode, env):
    out = str(tmp_path_factory.mktemp(f"step_sparse_{mode}") / "out.npz")
    base = {k: v for k, v in os.environ.items() if k not in ("HBK_STEP", "HBK_STEP_DENSE")}
    pr = subprocess.Popen([sys.executable, WORKER, mode, out], env=dict(base, **env), cwd=ROOT,
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
def dense_child(tmp_path_factory):
    return _child(tmp_path_factory, "dense", {"HBK_STEP_DENSE": "1"})


@pytest.fixture(scope="module")
def forced_child(tmp_path_factory):
    return _child(tmp_path_factory, "forced", {"HBK_STEP": "2"})


@pytest.fixture(scope="module")
def ran(layouts, dev):
    """Every in-process layout's step, run once: name -> (model, bucket, prob, state)."""
    return {name: _run_step(dev, "v2", layouts[name]) for name in IN_PROCESS}


@pytest.mark.parametrize("name", IN_PROCESS)
def test_step_matches_oracle(name, layouts, ran):
    m, bucket, prob, _ = ran[name]
    _check(layouts[name], m, bucket, prob)


@pytest.mark.parametrize("name", FORCED)
def test_forced_step_matches_oracle(name, forced_child):
    lay = sp.forced_layouts()[name]
    sc.check_bucket(lay, {k: forced_child[f"{name}/g/{k}"] for k in lay.params}, forced_child[f"{name}/stats"],
                    forced_child[f"{name}/prob"])


def test_no_live_row(layouts, ran, dev):
    """n_sel = 0: the whole bucket is zero, and the update with nothing accumulated does not
    fire: parameters and Adam's m and v keep their bits, the history row says so."""
    m, bucket, _, state = ran["none-1100"]
    plan = m.plan
    b = bucket.cpu().numpy()
    assert not b[:plan.n_params].any()
    np.testing.assert_array_equal(b[plan.n_params:], [0, 0, 0, 0, 0, 0, 1100, 0])
    g = torch.Generator().manual_seed(3)
    flat = m.flat_parameters.clone()
    mm = (1e-3 * torch.randn(plan.n_params, generator=g)).cuda()
    vv = (1e-6 * torch.rand(plan.n_params, generator=g)).cuda()
    before = [t.clone() for t in (flat, mm, vv)]
    hist = torch.zeros((1, 8), device="cuda")
    state = state.clone()
    state[0] = 0.0
    _on_variant_stream(dev, "v2", lambda: plan.step_update(flat, bucket.clone(), mm, vv, state, 0, lr=1e-3, history=hist))
    for t, b0 in zip((flat, mm, vv), before):
        assert torch.equal(t.view(torch.int32), b0.view(torch.int32))
    np.testing.assert_array_equal(hist.cpu().numpy()[0], [0, 1, 0, 0, 0, 0, 0, 0])


def test_all_live_has_the_dense_path_bits(layouts, ran, dense_child):
    """Every tile live: the listed tiles are all tiles and the splits' boundaries those of the
    dense path, so what k3s computes is bit-identical to HBK_STEP_DENSE=1; the dense child
    itself meets the oracle's bounds."""
    lay = layouts["all-1100"]
    m, bucket, _, _ = ran["all-1100"]
    plan = m.plan
    sc.check_bucket(lay, {k: dense_child[f"all-1100/g/{k}"] for k in lay.params}, dense_child["all-1100/stats"],
                    dense_child["all-1100/prob"])
    n = 0
    for k, v in plan.views(bucket[:plan.n_params]).items():
        if k.startswith("norm_in.") or k.endswith(K3S_TENSORS[2:]):
            np.testing.assert_array_equal(v.cpu().numpy().view(np.int32), dense_child[f"all-1100/g/{k}"].view(np.int32),
                                          err_msg=k)
            n += 1
    assert n == 14, n  # norm_in's two, and the hidden / gate / output weights of the four gated MLPs


@pytest.mark.parametrize("name", ["one-tail-1100", "odd-tiles-1100"])
def test_stale_workspace(name, layouts, dev):
    """From a workspace of 0xFF bytes: no stale slab, tile maximum or list entry leaks."""
    lay = layouts[name]
    m, bucket, prob, _ = _run_step(dev, "v2", lay, stale_workspace=True)
    assert bool(torch.isfinite(bucket).all()) and bool(torch.isfinite(prob).all())
    _check(lay, m, bucket, prob)


def test_gated_steps_in_one_graph(dev, tmp_path):
    from heybuddy.trainer import WakeWordTrainer
    gated = sc.gated_walk()
    w = sc.world()
    S, B = gated["rows"].shape
    assert list(gated["hist"][:, 0]) == [60, 60, 40, 0, 300, 90]
    tr = WakeWordTrainer(checkpoint_dir=str(tmp_path), device="cuda")
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.Q.items()}, strict=True)
    tr.model.dropout.p = 0.0
    tr._reset_accumulation()
    plan = tr.model.plan
    idx = torch.from_numpy(w.idx[gated["rows"]].copy()).cuda()
    y = torch.from_numpy(gated["y"].astype(np.float32)).cuda()
    sched = torch.tensor([[sc.GATED_LR, sc.NEG_WEIGHT]] * S, dtype=torch.float32, device="cuda")
    hist = torch.zeros((S, 8), device="cuda")

    def go():
        assert plan.step_variant(B, "cuda") == 2
        tr.train_indexed(idx, y, sched, pool32=dev["pool32"], pool16=dev["pool16"], history=hist, steps_per_graph=S)

    _on_variant_stream(dev, "v2", go)
    h, ref = hist.cpu().numpy().astype(np.float64), gated["hist"]
    print("n_sel", h[:, 0], "acc_steps", h[:, 1], "fired", h[:, 2])
    np.testing.assert_array_equal(h[:, [0, 1, 2, 4, 5, 6, 7]], ref[:, [0, 1, 2, 4, 5, 6, 7]])
    print("loss rel err", np.abs(h[:, 3] - ref[:, 3]) / np.maximum(ref[:, 3], 1e-30))
    np.testing.assert_allclose(h[:, 3], ref[:, 3], rtol=2e-4)
    params = {k: v.detach().cpu().numpy() for k, v in plan.views(tr.model.flat_parameters).items()}
    mom = {k: v.cpu().numpy() for k, v in plan.views(tr._m).items()}
    assert all(np.isfinite(v).all() for v in params.values())
    f = sc.gated_figures(params, mom, gated)
    print(f"share {f['share']:.3e}, drift {f['drift']:.3e}, max |P - P_ref| {f['max']:.3e}")
    print("m:", {k: f"{v:.1e}" for k, v in f["m"].items()})
    assert f["max"] <= 2 * sum(gated["fired_lr"])
    assert f["share"] <= 4 * GATED_SHARE_F32
    assert f["drift"] <= 4 * GATED_DRIFT_F32
    for k, v in f["m"].items():
        assert v <= 4 * GATED_M_F32[k], f"{k}: max |m - m_ref| = {v:.2e} of max |m_ref| (f32 walk {GATED_M_F32[k]:.1e})"
