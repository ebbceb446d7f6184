"""Time of the half-layer bank (hbk_mlp_half.hip) inside hbk_mlp_train_fwd_bwd.

    python tools/probe_half.py [ITERS] [--batch=1100]        # event-timed whole call
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python tools/probe_half.py 50
    python tools/probe_half.py --summarise DIR               # the bank's kernels from that trace

The summary adds the average time of the bank's forward kernels and of its backward kernels
per call and states each as a share of the f32 MFMA peak (157.3 TFLOP/s) for the
2 * 16 * B * 768 * 2H FLOP each side's big product needs. The bank's gate is a launch of the generic
path's gate_fwd_kernel (one of that kernel's 1 + n_blocks launches per call; 5.7 us at B = 1,100),
which the statistics do not tell apart from the others: the forward sum leaves it out.
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hey-buddy_amd"))

FWD = ("half_stats_kernel", "half_hg_kernel", "half_out_kernel", "half_sum_kernel")
BWD = ("half_colsum_kernel", "half_dwo_kernel", "half_du_kernel", "half_dwhg_kernel")
PEAK_F32_MFMA = 157.3e12


def summarise(directory: str, batch: int) -> None:
    path, = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    rows = list(csv.DictReader(open(path)))
    per_call = {}
    calls = None
    for r in rows:
        for k in FWD + BWD:
            if k in r["Name"]:
                n = int(r["Calls"])
                total = float(r["AverageNs"]) * n
                if k == "half_hg_kernel":
                    calls = n
                per_call[k] = (n, total)
    flop = 2.0 * 16 * batch * 768 * 128
    for side, names in (("forward", FWD), ("backward", BWD)):
        ns = sum(per_call[k][1] for k in names) / calls
        parts = ", ".join(f"{k[5:-7]} {per_call[k][1] / calls / 1e3:.1f}" for k in names)
        print(f"{side} bank: {ns / 1e3:.1f} us per call over {calls} calls ({parts}); "
              f"{flop / 1e9:.2f} GFLOP -> {flop / ns / 1e3:.2f} TFLOP/s = {100 * flop / (ns * 1e-9) / PEAK_F32_MFMA:.1f} % "
              f"of the f32 MFMA peak")


def main() -> None:
    batch = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--batch=")), 1100)
    if "--summarise" in sys.argv:
        return summarise(sys.argv[sys.argv.index("--summarise") + 1], batch)
    import torch
    from heybuddy.wakeword import WakeWordMLPModel
    iters = next((int(a) for a in sys.argv[1:] if a.isdigit()), 50)
    torch.manual_seed(0)
    m = WakeWordMLPModel(use_half_layers=True).cuda()
    plan = m.plan
    x = torch.randn(batch, 1536, device="cuda")
    y = (torch.rand(batch, device="cuda") < 0.3).float()
    bucket = torch.zeros(plan.n_params + plan.N_STATS, device="cuda")
    for _ in range(5):
        plan.train_fwd_bwd(m.flat_parameters, x, y, bucket, neg_weight=1.0, dropout_p=0.1, seed=1)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        plan.train_fwd_bwd(m.flat_parameters, x, y, bucket, neg_weight=1.0, dropout_p=0.1, seed=i)
    t1.record()
    torch.cuda.synchronize()
    print(f"hbk_mlp_train_fwd_bwd with half layers, B = {batch}: {t0.elapsed_time(t1) / iters * 1e3:.1f} us per call "
          f"({iters} calls)")


if __name__ == "__main__":
    main()
