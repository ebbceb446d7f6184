"""Every kernel instantiation and network depth a train-step plan can pick, against the float64
oracle (oracle/mlp.py). The cases are data (tests/step_route_cases.py); tests/test_step_routes.py
proves on the CPU that they reach all 14 k3s pairs with full-length, short, half-filled and
zero-slab splits (all 93 k3s_body<> instantiations), k1c's four K chunks at their RT extremes,
k1b's six K splits (the inference batches of test_mlp_fused_gpu.py), depths 0 / 1 / 2 under v1
and v2 and HBK_PRE_TILES 1 to 4. Every
case here first asserts, through hbk_mlp_step_plan_info, that the plan it is about to run is the
one the CPU checker (tests/step_routes_check.cpp) printed for it, and prints it: a forced knob
the planner silently replaced fails before the step runs.

Where: cases that need HBK_STEP=2 latched run in ONE fresh child (tests/step_routes_worker.py, on
the 64-CU stream, 114 single steps of at most 1,100 rows); the rest (the library's own plans on
32 / 48 / 64 / 128-CU streams and the whole GPU, the gated walks) run here.

Bounds: the project's, through step_oracle_cases.check_bucket, unchanged: counts exact, loss sum
1e-5, prob 1e-6 + 1e-4 relative, every gradient tensor within 1e-4 of its max |g_ref|. Headroom,
the float32 numpy restatement of each new layout against the float64 one (worst gradient tensor
as a share of its max |g_ref| / loss sum relative / worst prob error as a share of its bound):
  dense-1 3.2e-6 / 2e-9 / 0.00      dense-32 .. dense-961 (17 sizes) <= 3.7e-6 / <= 1e-7 / <= 0.01
  sparse-32 4.7e-6 / 5e-8 / 0.15    sparse-64 6.5e-6 / 2e-7 / 0.19   sparse-273 3.4e-6 / 6e-7 / 0.19
  one-273 7.2e-6 / 6e-7 / 0.15      one-545 6.0e-6 / 2e-7 / 0.09     sparse-545 5.3e-6 / 3e-7 / 0.39
  none-32, none-64, L0 / L1 none-800 0 / 0 / 0.00                    k1c-273 2.0e-6 / 4e-8 / 0.00
  d0-1 .. d0-273, d1-1 .. d1-273 <= 1.3e-6 / <= 7e-8 / 0.00
  L0/dense-1100 1.4e-6 / 2e-8 / 0.00   L0/sparse-1100 2.7e-6 / 8e-8 / 0.27   L0/few-801 2.6e-6 / 4e-8 / 0.23
  L1/dense-1100 1.7e-6 / 9e-8 / 0.00   L1/sparse-1100 3.4e-6 / 4e-7 / 0.32   L1/few-801 6.1e-6 / 2e-7 / 0.18
Gradients and loss leave >= 10 x everywhere. sparse-32, one-273, one-545 and sparse-273 carry the
row seed (of 5 to 8 tried) that leaves 4 x on every bound; a first version of the one-live-tile
layouts with a SINGLE selected row was dropped, because one row's loss under the wide parameters
carries its f32 logit error whole (up to 3.8e-5 relative, past the 1e-5 bound in the f32
restatement itself). The prob figure of the mixed layouts on wide parameters (sparse-545, L0 / L1
sparse-1100: 0.27 to 0.39 of the bound, i.e. 2.6 to 3.7 x) is that of the existing sparse-1100
(0.38) and does not move with the seed (8 seeds each: 0.19 to 0.58): it is the f32 logit error
through the x 120 output weight at the few hundred selected rows with small p, where the bound
is 1e-6 + 1e-4 p.

Gated walks (six train_indexed steps at B = 800, n_sel = 60, 60, 40, 0, 300, 90; see
tests/test_train_step_oracle_gpu.py) from the wide parameters W0 / W1 of depth 0 / 1: history
counts, accumulation steps and fired flags exact, loss within 2e-4. The float32 walk of the oracle
over the float64 walk's rows, measured on the CPU against the float64 walk:
  depth 0: share of parameters differing by > 1e-5: 4.57e-6 (1 of 218,721); drift 1.40e-3;
           max |P - P_ref| 1.96e-4; per tensor max |m - m_ref| / max |m_ref|: GATED_M_F32[0]
  depth 1: share 1.26e-5 (3 of 237,569); drift 2.14e-3; max |P - P_ref| 3.15e-4; GATED_M_F32[1]
and the device must stay within 4 x each and within max |P - P_ref| <= 2 sum(lr of the fired
steps) = 8e-4, as at depth 2.

HBK_PRE_TILES 1, 2, 4: the depth-2 walk on v2 with the bounds of test_gated_steps_match_oracle.
By reading (k1a_tile<true, true> in hbk_mlp_fused.hip) the grouping decides only which workgroup
and loop iteration computes a row tile's statistics and mask; each row's mean and variance are
summed by one wave over that row alone, in the same lane order, so no sum can change with it. The
final parameters are still NOT asserted bit-equal to the default run's: the chain kernel adds the
bias and LayerNorm gradients with float atomics, whose order differs from run to run whatever the
grouping. Whether they came out bit-equal is printed.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import step_oracle_cases as sc
import step_route_cases as rc
from step_routes_worker import StepRunner, check_against_oracle, per_call_knobs
from test_step_routes import checker, run_checker  # noqa: F401  (the CPU checker, built the same way)
from test_train_step_oracle_gpu import GATED_DRIFT_F32, GATED_M_F32 as GATED_M_F32_L2, GATED_SHARE_F32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "step_routes_worker.py")

# the f32 walk's figures per depth (see above); depth 2: tests/test_train_step_oracle_gpu.py's
GATED_SHARE = {0: 4.58e-6, 1: 1.27e-5, 2: GATED_SHARE_F32}
GATED_DRIFT = {0: 1.41e-3, 1: 2.14e-3, 2: GATED_DRIFT_F32}
GATED_M_F32 = {
    0: {"norm_in.weight": 1.6e-04, "norm_in.bias": 1.3e-04, "mlp_in.hidden.weight": 1.2e-04,
        "mlp_in.hidden.bias": 5.5e-05, "mlp_in.output.weight": 7.5e-05, "mlp_in.output.bias": 1.6e-05,
        "mlp_in.gate.weight": 1.6e-04, "mlp_in.gate.bias": 1.5e-04, "norm_out.weight": 2.6e-05,
        "norm_out.bias": 2.0e-05, "mlp_out.hidden.weight": 2.5e-05, "mlp_out.hidden.bias": 1.5e-05,
        "mlp_out.output.weight": 9.1e-05, "mlp_out.output.bias": 8.7e-06, "mlp_out.gate.weight": 3.1e-05,
        "mlp_out.gate.bias": 1.9e-05},
    1: {"norm_in.weight": 2.4e-04, "norm_in.bias": 1.7e-04, "mlp_in.hidden.weight": 4.5e-04,
        "mlp_in.hidden.bias": 2.9e-04, "mlp_in.output.weight": 2.1e-04, "mlp_in.output.bias": 1.1e-04,
        "mlp_in.gate.weight": 3.5e-04, "mlp_in.gate.bias": 2.4e-04, "layers.0.0.weight": 1.1e-04,
        "layers.0.0.bias": 8.4e-05, "layers.0.1.hidden.weight": 1.5e-04, "layers.0.1.hidden.bias": 7.5e-05,
        "layers.0.1.output.weight": 6.8e-05, "layers.0.1.output.bias": 4.4e-05, "layers.0.1.gate.weight": 9.4e-05,
        "layers.0.1.gate.bias": 6.3e-05, "norm_out.weight": 5.3e-05, "norm_out.bias": 4.3e-05,
        "mlp_out.hidden.weight": 6.3e-05, "mlp_out.hidden.bias": 4.6e-05, "mlp_out.output.weight": 4.5e-05,
        "mlp_out.output.bias": 4.3e-05, "mlp_out.gate.weight": 5.1e-05, "mlp_out.gate.bias": 3.6e-05},
    2: GATED_M_F32_L2,
}

CASES = {c.name: c for c in rc.cases()}
WORKER_CASES = [c.name for c in CASES.values() if c.where == "worker"]
MAIN_STEPS = [c.name for c in CASES.values() if c.where == "main" and rc.is_step(c)]
GATED = [c.name for c in CASES.values() if c.layout == "gated" and "HBK_PRE_TILES" not in c.knobs]
GENERIC = [f"L{L}/{kind}" for L in (0, 1) for kind in rc.DEPTH_KINDS]


@pytest.fixture(scope="module")
def plans(checker):  # noqa: F811
    return run_checker(checker, list(CASES.values()))


@pytest.fixture(scope="module")
def worker(plans, tmp_path_factory):
    """The child's verdict per case (one run for the module), and its output."""
    d = tmp_path_factory.mktemp("step_routes")
    plans_json, out = str(d / "plans.json"), str(d / "out.json")
    json.dump(plans, open(plans_json, "w"))
    env = {k: v for k, v in os.environ.items() if k not in rc.PER_CALL_KNOBS}
    pr = subprocess.Popen([sys.executable, WORKER, plans_json, out], env=dict(env, HBK_STEP="2"), cwd=ROOT,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        log, _ = pr.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        pr.kill()
        pr.communicate()
        raise
    print(log)
    assert pr.returncode == 0, log[-4000:]
    return json.load(open(out))


@pytest.fixture(scope="module")
def runner():
    return StepRunner()


def test_the_worker_ran_every_case(worker):
    assert sorted(worker) == sorted(WORKER_CASES) and len(WORKER_CASES) >= 110


@pytest.mark.parametrize("name", WORKER_CASES)
def test_forced_route_matches_oracle(name, worker):
    """A worker case: the plan the checker printed, then check_bucket's bounds."""
    assert worker[name] == "ok", worker[name]


@pytest.mark.parametrize("name", MAIN_STEPS)
def test_own_plan_matches_oracle(name, runner, plans):
    """The library's own plan on a 32 / 48 / 128-CU stream, and at depths 0 / 1 / 2 on the whole GPU (v1) and
    on 64 CUs (v2): the plan the checker printed, then check_bucket's bounds."""
    runner.run_case(CASES[name], plans[name])


@pytest.mark.parametrize("key", GENERIC)
def test_generic_path_matches_oracle_at_depth(key, runner):
    """hbk_mlp_train_fwd_bwd on gathered rows at depths 0 and 1."""
    lay = rc.layout(key)
    m = runner.model(lay.params)
    plan = m.plan
    bucket = torch.zeros(plan.n_params + plan.N_STATS, device="cuda")
    prob = torch.zeros(lay.B, device="cuda")
    plan.train_fwd_bwd(m.flat_parameters, torch.from_numpy(lay.x).cuda(),
                       torch.from_numpy(lay.y.astype(np.float32)).cuda(), bucket, neg_weight=sc.NEG_WEIGHT, prob=prob)
    torch.cuda.synchronize()
    check_against_oracle(lay, plan, bucket, prob)


@pytest.mark.parametrize("variant", ["v1", "v2", "generic"])
@pytest.mark.parametrize("L", [0, 1])
def test_no_selected_row_leaves_the_parameters_alone_at_depth(L, variant, runner, plans):
    """none-800 at depth L, then the update with nothing accumulated: the gate does not fire, and the
    parameters and Adam's m and v keep their bits."""
    lay = rc.layout(f"L{L}/none-800")
    m = runner.model(lay.params)
    plan, cus = m.plan, 64 if variant == "v2" else runner.n_cu
    bucket = torch.zeros(plan.n_params + plan.N_STATS, device="cuda")
    state = plan.new_state("cuda")
    y = torch.from_numpy(lay.y.astype(np.float32)).cuda()
    g = torch.Generator().manual_seed(3)
    flat = m.flat_parameters.clone()
    mm = (1e-3 * torch.randn(plan.n_params, generator=g)).cuda()
    vv = (1e-6 * torch.rand(plan.n_params, generator=g)).cuda()
    before = [t.clone() for t in (flat, mm, vv)]
    hist = torch.zeros((1, 8), device="cuda")

    def go():
        if variant == "generic":
            plan.train_fwd_bwd(flat, torch.from_numpy(lay.x).cuda(), y, bucket, neg_weight=sc.NEG_WEIGHT)
        else:
            case = CASES[f"L{L}-{variant}-none-800"]
            runner.assert_plan(case, plans[case.name], plan)
            plan.step_fwd_bwd(flat, bucket, state, 0, y, lay.B, pool32=runner.pool32, pool16=runner.pool16,
                              idx=torch.from_numpy(lay.idx).cuda(), idx_stride=lay.B, neg_weight=sc.NEG_WEIGHT)
        state[0] = 0.0
        plan.step_update(flat, bucket, mm, vv, state, 0, lr=1e-3, history=hist)

    runner.on_stream(cus, go)
    for t, b in zip((flat, mm, vv), before):
        assert bool(torch.isfinite(t).all())
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))
    np.testing.assert_array_equal(hist.cpu().numpy()[0], [0, 1, 0, 0, 0, 0, 0, 0])


def _gated_run(runner, case, want, start, walk, tmp_path):
    """The six-step walk through train_indexed on the case's stream with its knobs: (history, parameters, m)."""
    from heybuddy.trainer import WakeWordTrainer
    w = sc.world()
    S, B = walk["rows"].shape
    tr = WakeWordTrainer(checkpoint_dir=str(tmp_path), device="cuda", num_layers=case.NG - 2)
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in start.items()}, strict=True)
    tr.model.dropout.p = 0.0
    tr._reset_accumulation()
    plan = tr.model.plan
    idx = torch.from_numpy(w.idx[walk["rows"]].copy()).cuda()
    y = torch.from_numpy(walk["y"].astype(np.float32)).cuda()
    sched = torch.tensor([[sc.GATED_LR, sc.NEG_WEIGHT]] * S, dtype=torch.float32, device="cuda")
    hist = torch.zeros((S, 8), device="cuda")

    def go():
        with per_call_knobs(case.knobs):
            runner.assert_plan(case, want, plan)
            tr.train_indexed(idx, y, sched, pool32=runner.pool32, pool16=runner.pool16, history=hist,
                             steps_per_graph=4)
            torch.cuda.synchronize()

    runner.on_stream(case.cus, go)
    params = {k: v.detach().cpu().numpy() for k, v in plan.views(tr.model.flat_parameters).items()}
    m = {k: v.cpu().numpy() for k, v in plan.views(tr._m).items()}
    return hist.cpu().numpy().astype(np.float64), params, m


def _check_gated(h, params, m, walk, start, depth):
    """The assertions of test_gated_steps_match_oracle with the figures of ``depth``."""
    ref = walk["hist"]
    print("n_sel", h[:, 0], "acc_steps", h[:, 1], "fired", h[:, 2])
    np.testing.assert_array_equal(h[:, [0, 1, 2, 4, 5, 6, 7]], ref[:, [0, 1, 2, 4, 5, 6, 7]])
    print("loss rel err", np.abs(h[:, 3] - ref[:, 3]) / np.maximum(ref[:, 3], 1e-30))
    np.testing.assert_allclose(h[:, 3], ref[:, 3], rtol=2e-4)
    assert all(np.isfinite(v).all() for v in params.values())
    f = sc.gated_figures(params, m, walk, start=start)
    print(f"share {f['share']:.3e} (f32 walk {GATED_SHARE[depth]:.2e}), drift {f['drift']:.3e} (f32 walk "
          f"{GATED_DRIFT[depth]:.2e}), max |P - P_ref| {f['max']:.3e}")
    print("m:", {k: f"{v:.1e}" for k, v in f["m"].items()})
    assert f["max"] <= 2 * sum(walk["fired_lr"])
    assert f["share"] <= 4 * GATED_SHARE[depth]
    assert f["drift"] <= 4 * GATED_DRIFT[depth]
    for k, v in f["m"].items():
        assert v <= 4 * GATED_M_F32[depth][k], (
            f"{k}: max |m - m_ref| = {v:.2e} of max |m_ref| (f32 walk {GATED_M_F32[depth][k]:.1e})")


@pytest.mark.parametrize("name", GATED)
def test_gated_steps_match_oracle_at_depth(name, runner, plans, tmp_path):
    case = CASES[name]
    L = case.NG - 2
    start, walk = rc.depth_params(L)[1], rc.gated_walk(L)
    h, params, m = _gated_run(runner, case, plans[name], start, walk, tmp_path)
    _check_gated(h, params, m, walk, start, L)


@pytest.fixture(scope="module")
def walk2():
    return sc.gated_walk()


@pytest.fixture(scope="module")
def default_pre_tiles_run(runner, plans, walk2, tmp_path_factory):
    """The depth-2 walk on v2 with HBK_PRE_TILES = 3, the default."""
    case = CASES["pre3-gated"]
    return _gated_run(runner, case, plans[case.name], sc.world().Q, walk2, tmp_path_factory.mktemp("pre3"))


@pytest.mark.parametrize("n", rc.PRE_TILES)
def test_gated_steps_match_oracle_at_every_pre_tiles(n, runner, plans, walk2, default_pre_tiles_run, tmp_path):
    case = CASES[f"pre{n}-gated"]
    if n == 3:
        h, params, m = default_pre_tiles_run
    else:
        h, params, m = _gated_run(runner, case, plans[case.name], sc.world().Q, walk2, tmp_path)
    _check_gated(h, params, m, walk2, sc.world().Q, 2)
    same = all(np.array_equal(params[k].view(np.int32), default_pre_tiles_run[1][k].view(np.int32)) for k in params)
    print(f"HBK_PRE_TILES={n}: final parameters bit-equal to the default run's: {same}")
