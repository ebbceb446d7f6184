"""Child process of tests/test_step_routes_gpu.py: the "worker" cases of tests/step_route_cases.py,
single train steps with the v2 kernels (k1s / k1c / k2 / k3s) FORCED on the 64-CU train stream at
batch sizes the library would give to v1. HBK_STEP is read once per process, hence the fresh
process; HBK_K3_PAIR, HBK_K3_R, HBK_K1_KC and HBK_K1_RT are read per call and set here between
calls (``per_call_knobs``).

usage: HBK_STEP=2 python tests/step_routes_worker.py PLANS.json OUT.json

PLANS.json: case name -> the plan tests/step_routes_check.cpp printed for it. Every case first
asserts that hbk_mlp_step_plan_info reports exactly that plan, prints it, runs the step and
compares the bucket with the float64 oracle (step_oracle_cases.check_bucket). OUT.json: case name
-> "ok" or the assertion's message. Anything but a failed assertion (a HIP error) ends the
process at once with a non-zero status: nothing more runs on the GPU.

``StepRunner`` is also what the parent's own (main-process) cases run through.
"""
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "hey-buddy_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import step_oracle_cases as sc  # noqa: E402
import step_route_cases as rc  # noqa: E402


@contextlib.contextmanager
def per_call_knobs(knobs):
    """The per-call knobs of a case in os.environ for the calls inside, then as they were."""
    mine = {k: str(v) for k, v in knobs.items() if k in rc.PER_CALL_KNOBS}
    before = {k: os.environ.get(k) for k in mine}
    os.environ.update(mine)
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class StepRunner:
    """The pools on the device, one model per parameter set, one masked stream per width."""

    def __init__(self):
        w = sc.world()
        self.pool32 = torch.from_numpy(w.pool32.copy()).cuda()
        self.pool16 = torch.from_numpy(w.pool16.copy()).cuda()
        self.n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        self._models, self._streams = {}, {}

    def model(self, params):
        from heybuddy.wakeword import WakeWordMLPModel
        if id(params) not in self._models:
            L = sum(1 for k in params if k.startswith("layers.") and k.endswith(".0.weight"))
            m = WakeWordMLPModel(num_layers=L)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
            m.dropout.p = 0.0
            assert m.plan.fused
            self._models[id(params)] = m.cuda()
        return self._models[id(params)]

    def on_stream(self, cus, fn):
        """fn() on the default stream (the whole GPU) or on a stream masked to ``cus`` CUs."""
        from heybuddy.pipeline import masked_stream, train_cu_set
        if cus >= self.n_cu:
            out = fn()
        else:
            if cus not in self._streams:
                self._streams[cus] = masked_stream(torch.device("cuda", 0), train_cu_set(self.n_cu, cus))
            ms = self._streams[cus]
            ms.stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(ms.stream):
                out = fn()
        torch.cuda.synchronize()
        return out

    def assert_plan(self, case, want, plan):
        """hbk_mlp_step_plan_info (current stream, knobs as set now) against the checker's plan."""
        got = plan.step_plan_info(case.B, "cuda")
        print(f"{case.name}: plan {got}")
        assert got == {k: want[k] for k in got}, f"{case.name}: the library plans {got}, the checker {want}"
        return got

    def run_case(self, case, want):
        """One single-step case: plan asserted, step run, bucket against the oracle."""
        lay = rc.layout(case.layout)
        m = self.model(lay.params)
        plan, B = m.plan, lay.B
        bucket = torch.zeros(plan.n_params + plan.N_STATS, device="cuda")
        prob = torch.zeros(B, device="cuda")
        y = torch.from_numpy(lay.y.astype(np.float32)).cuda()
        idx = torch.from_numpy(lay.idx).cuda()
        ws = None
        if case.stale:  # NaN bits in f32 and f16: nothing may depend on what the workspace held
            ws = torch.full((plan.workspace_bytes(B),), 0xFF, dtype=torch.uint8, device="cuda")

        def go():
            with per_call_knobs(case.knobs):
                self.assert_plan(case, want, plan)
                plan.step_fwd_bwd(m.flat_parameters, bucket, plan.new_state("cuda"), 0, y, B, pool32=self.pool32,
                                  pool16=self.pool16, idx=idx, idx_stride=B, neg_weight=sc.NEG_WEIGHT,
                                  dropout_p=sc.DROP_P if lay.dropout else 0.0, seed=sc.DROP_SEED, prob=prob,
                                  workspace=ws)
                torch.cuda.synchronize()

        self.on_stream(case.cus, go)
        check_against_oracle(lay, plan, bucket, prob)


def check_against_oracle(lay, plan, bucket, prob):
    """The bounds of tests/test_train_step_oracle_gpu.py, unchanged (check_bucket); all finite; with no
    selected row the gradients are exact zeros."""
    assert bool(torch.isfinite(bucket).all()) and bool(torch.isfinite(prob).all()), f"{lay.name}: not finite"
    grads = {k: v.cpu().numpy() for k, v in plan.views(bucket[:plan.n_params]).items()}
    stats = bucket[plan.n_params:].cpu().numpy()
    sc.check_bucket(lay, grads, stats, prob.cpu().numpy())
    if lay.reference()[1][0] == 0:
        assert not bucket[:plan.n_params].cpu().numpy().any(), f"{lay.name}: a gradient without a selected row"
        np.testing.assert_array_equal(stats, [0, 0, 0, 0, 0, 0, lay.B, 0])


def main():
    assert os.environ.get("HBK_STEP") == "2"
    plans = json.load(open(sys.argv[1]))
    runner, results = StepRunner(), {}
    for case in rc.cases():
        if case.where != "worker":
            continue
        try:
            runner.run_case(case, plans[case.name])
            results[case.name] = "ok"
        except AssertionError as e:  # a wrong result: reported per case; the next case still runs
            results[case.name] = f"{e}"[:3000] or "assertion failed"
            print(f"{case.name}: FAILED {results[case.name]}")
        with open(sys.argv[2], "w") as f:  # (after every case: what ran before a HIP error is kept)
            json.dump(results, f)
    print(f"{len(results)} cases, {sum(v == 'ok' for v in results.values())} ok")


if __name__ == "__main__":
    main()
