"""Time of one generic train step (hbk_mlp_train_fwd_bwd + hbk_mlp_gate_adam) of a classifier
variant: plain or gated blocks, any activation.

    python tools/probe_mlp_variant.py [ITERS] [--batch=1100] [--gated] [--activation=silu]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python tools/probe_mlp_variant.py 50
    python tools/probe_mlp_variant.py --summarise DIR 55      # kernel time per step from that trace

Without a profiler it prints the event-timed time per step; the summary adds up the trace's
kernel times (memsets are not kernels and stay out) and divides by the number of steps
(warm-up included: 5 + ITERS).
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hey-buddy_amd"))


def summarise(directory: str, steps: int) -> None:
    path, = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    rows = list(csv.DictReader(open(path)))
    total = 0.0
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns = float(r["TotalDurationNs"])
        total += ns
        print(f"{ns / steps / 1e3:8.2f} us per step  {int(r['Calls']) / steps:5.1f} launches  {r['Name'][:90]}")
    print(f"{total / steps / 1e3:8.2f} us of kernel time per step over {steps} steps")


def main() -> None:
    if "--summarise" in sys.argv:
        i = sys.argv.index("--summarise")
        return summarise(sys.argv[i + 1], int(sys.argv[i + 2]))
    import torch
    from heybuddy.wakeword import WakeWordMLPModel
    batch = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--batch=")), 1100)
    act = next((a.split("=")[1] for a in sys.argv if a.startswith("--activation=")), "silu")
    iters = next((int(a) for a in sys.argv[1:] if a.isdigit()), 50)
    torch.manual_seed(0)
    m = WakeWordMLPModel(use_gating="--gated" in sys.argv, activation=act).cuda()
    plan = m.plan
    flat = m.flat_parameters
    x = torch.randn(batch, 1536, device="cuda")
    y = (torch.rand(batch, device="cuda") < 0.3).float()
    bucket = torch.zeros(plan.n_params + plan.N_STATS, device="cuda")
    mom, var = torch.zeros_like(flat), torch.zeros_like(flat)
    state = torch.tensor([0.0, 1.0, 0.0, 0.0], device="cuda")
    ctrl = torch.zeros(4, device="cuda")

    def step(i):
        plan.train_fwd_bwd(flat, x, y, bucket, neg_weight=1.0, dropout_p=0.1, seed=i)
        plan.gate_adam(flat, bucket, mom, var, state, ctrl, None, 1e-4)

    for i in range(5):
        step(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        step(5 + i)
    t1.record()
    torch.cuda.synchronize()
    print(f"generic step, {'gated' if m.use_gating else 'plain'} {m.activation}, B = {batch}: "
          f"{t0.elapsed_time(t1) / iters * 1e3:.1f} us per step ({iters} steps, event-timed)")


if __name__ == "__main__":
    main()
