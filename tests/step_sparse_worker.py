"""Child process of tests/test_step_sparse_gpu.py (never imported by pytest): single v2 train
steps on the 64-CU train stream under an environment the library reads once per process.

usage: HBK_STEP_DENSE=1 python tests/step_sparse_worker.py dense OUT.npz
           the all-live layout of step_sparse_cases.layouts() on the dense path
       HBK_STEP=2 python tests/step_sparse_worker.py forced OUT.npz
           step_sparse_cases.forced_layouts() (batches below the library's v2 threshold)

Asserts step_variant == 2 at every batch and writes <layout>/{stats, prob, g/<name>}.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hey-buddy_amd"), os.path.join(ROOT, "tests")]


def main():
    import numpy as np
    import torch
    import step_oracle_cases as sc
    import step_sparse_cases as sp
    from heybuddy.pipeline import masked_stream, train_cu_set
    from heybuddy.wakeword import WakeWordMLPModel

    mode, path = sys.argv[1], sys.argv[2]
    if mode == "dense":
        assert os.environ.get("HBK_STEP_DENSE") == "1" and "HBK_STEP" not in os.environ
        lays = {"all-1100": sp.layouts()["all-1100"]}
    else:
        assert mode == "forced" and os.environ.get("HBK_STEP") == "2" and "HBK_STEP_DENSE" not in os.environ
        lays = sp.forced_layouts()
    w = sc.world()
    dev = torch.device("cuda", 0)
    ms = masked_stream(dev, train_cu_set(torch.cuda.get_device_properties(0).multi_processor_count, 64))
    pool32, pool16 = torch.from_numpy(w.pool32.copy()).cuda(), torch.from_numpy(w.pool16.copy()).cuda()
    m = WakeWordMLPModel()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.Q.items()}, strict=True)
    m.dropout.p = 0.0
    m = m.cuda()
    plan, out = m.plan, {}
    ms.stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(ms.stream):
        for name, lay in lays.items():
            assert plan.step_variant(lay.B, dev) == 2, name
            bucket = torch.zeros(plan.n_params + plan.N_STATS, device=dev)
            prob = torch.zeros(lay.B, device=dev)
            plan.step_fwd_bwd(m.flat_parameters, bucket, plan.new_state(dev), 0,
                              torch.from_numpy(lay.y.astype(np.float32)).cuda(), lay.B, pool32=pool32, pool16=pool16,
                              idx=torch.from_numpy(lay.idx).cuda(), idx_stride=lay.B, neg_weight=sc.NEG_WEIGHT,
                              prob=prob)
            torch.cuda.synchronize()
            out[f"{name}/stats"] = bucket[plan.n_params:].cpu().numpy()
            out[f"{name}/prob"] = prob.cpu().numpy()
            for k, v in plan.views(bucket[:plan.n_params]).items():
                out[f"{name}/g/{k}"] = v.cpu().numpy()
    np.savez(path, **out)
    print(f"{mode}: {list(lays)}")


if __name__ == "__main__":
    main()
