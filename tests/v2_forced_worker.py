"""Child process of tests/test_v2_forced_gpu.py (never imported by pytest): the v2 train step
(k1s / k1c / k2 / k3s) FORCED at the batch sizes the library would give to v1, on the 64-CU
train stream. HBK_STEP is read once per process, hence the fresh process.

usage: HBK_STEP=2 python tests/v2_forced_worker.py OUT.npz

Asserts step_variant == 2 at every batch it runs and writes one .npz:
  step/<layout>/{stats, prob, g/<name>}  single steps of step_oracle_cases.forced_layouts()
  b96/{stats, prob, g/<name>}            the tests/golden/classifier.npz step (neg_weight 2)
  epoch/{lr, hlr, loss, rec, fp, final/<name>}   the fixture's 24-step train_epoch
  stages/{<history>, sizes, final/<name>}        the fixture's 3-stage WakeWordTrainer.__call__
  batches                                every batch size whose variant was queried
"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hey-buddy_amd"), os.path.join(ROOT, "tests")]


def main():
    import numpy as np
    import torch
    import step_oracle_cases as sc
    from heybuddy.pipeline import masked_stream, train_cu_set
    from heybuddy.trainer import WakeWordTrainer
    from heybuddy.wakeword import WakeWordMLPModel
    from oracle import golden_classifier as gc
    from test_stages_gpu import STAGE_HISTORIES, StageIterator

    assert os.environ.get("HBK_STEP") == "2"
    out, batches = {}, []
    w = sc.world()
    dev = torch.device("cuda", 0)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ms = masked_stream(dev, train_cu_set(n_cu, 64))
    pool32, pool16 = torch.from_numpy(w.pool32.copy()).cuda(), torch.from_numpy(w.pool16.copy()).cuda()

    def model(params):
        m = WakeWordMLPModel()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        m.dropout.p = 0.0
        return m.cuda()

    def is_v2(plan, B):
        batches.append(B)
        assert plan.step_variant(B, dev) == 2, B

    def step(tag, m, B, y, neg_weight, **rows):
        plan = m.plan
        is_v2(plan, B)
        bucket = torch.zeros(plan.n_params + plan.N_STATS, device=dev)
        prob = torch.zeros(B, device=dev)
        plan.step_fwd_bwd(m.flat_parameters, bucket, plan.new_state(dev), 0,
                          torch.from_numpy(np.asarray(y, np.float32)).cuda(), B, neg_weight=neg_weight, prob=prob,
                          **rows)
        torch.cuda.synchronize()
        out[f"{tag}/stats"] = bucket[plan.n_params:].cpu().numpy()
        out[f"{tag}/prob"] = prob.cpu().numpy()
        for k, v in plan.views(bucket[:plan.n_params]).items():
            out[f"{tag}/g/{k}"] = v.cpu().numpy()

    def trainer(ck):
        tr = WakeWordTrainer(checkpoint_dir=ck, device="cuda")
        tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.P0.items()}, strict=True)
        tr.model.dropout.p = 0.0
        return tr

    ms.stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(ms.stream), tempfile.TemporaryDirectory() as ck:
        models = {id(w.P0): model(w.P0), id(w.Q): model(w.Q)}
        for name, lay in sc.forced_layouts().items():
            step(f"step/{name}", models[id(lay.params)], lay.B, lay.y, sc.NEG_WEIGHT, pool32=pool32, pool16=pool16,
                 idx=torch.from_numpy(lay.idx).cuda(), idx_stride=lay.B)
        params, x, y, np_batches = gc.golden_inputs()
        step("b96", models[id(w.P0)], len(x), y, 2.0,
             pool32=torch.from_numpy(x).cuda().reshape(len(x), -1).contiguous())

        tr = trainer(os.path.join(ck, "epoch"))
        for xb, _ in np_batches:
            is_v2(tr.model.plan, len(xb))
        data = [(torch.from_numpy(xb), torch.from_numpy(yb)) for xb, yb in np_batches]
        h = tr.train_epoch(data, num_steps=24, warmup_steps=4, hold_steps=8, validation_steps=1000,
                           checkpoint_steps=100000)
        torch.cuda.synchronize()
        for name, t in zip(("lr", "nw", "loss", "hlr", "rec", "fp"), h[:6]):
            out[f"epoch/{name}"] = t.numpy()
        for k, v in tr.model.state_dict().items():
            out[f"epoch/final/{k}"] = v.cpu().numpy()

        pools, val, test = gc.stage_inputs()
        it = StageIterator(pools)
        tr = trainer(os.path.join(ck, "stages"))
        hs = tr(it, validation=[(torch.from_numpy(a), torch.from_numpy(b)) for a, b in val],
                testing=[(torch.from_numpy(a), torch.from_numpy(b)) for a, b in test], num_steps=gc.STAGE_STEPS,
                validation_steps=gc.STAGE_VAL_STEPS, checkpoint_steps=100000, name="stages")
        torch.cuda.synchronize()
        for B in sorted(set(it.sizes)):
            is_v2(tr.model.plan, B)
        for k in STAGE_HISTORIES:
            out[f"stages/{k}"] = hs[k].numpy()
        out["stages/sizes"] = np.array(it.sizes)
        for k, v in tr.model.state_dict().items():
            out[f"stages/final/{k}"] = v.cpu().numpy()
    out["batches"] = np.array(batches)
    np.savez(sys.argv[1], **out)
    print(f"v2 forced at {len(batches)} batch sizes: {sorted(set(batches))}")


if __name__ == "__main__":
    main()
