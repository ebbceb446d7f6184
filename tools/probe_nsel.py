"""How many rows the high-loss filter keeps in the headline's train steps.

Runs bench.py's main() with the arguments given after ``--`` (default: the
headline, config 5, 5 + 2 steps) and keeps every history buffer the timed
path hands to train_indexed; after the run it reads column 0 (n_sel) of the
last chunk's rows and column 2 (fired: the share of steps whose update ran,
and how firing and non-firing steps follow each other) and prints n_sel's
distribution, with ceil(n_sel / 16) (the
fewest 16-row tiles that hold them) and ceil(n_sel / 32) (the 32-row steps
of a row-compacted walk) per train step. The history has no per-row data, so
the live tiles themselves are counted by classifying the chunk's last 200
batches again with the final weights.

usage: python tools/probe_nsel.py [--out FILE] [-- bench.py arguments]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hey-buddy_amd"))


def main() -> None:
    argv = sys.argv[1:]
    bench_args = ["--gpus", "1", "--steps", "5", "--warmup", "2", "--config", "5", "--no-cpu"]
    if "--" in argv:
        bench_args = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None

    import numpy as np
    import torch
    from heybuddy.trainer import WakeWordTrainer

    seen = {}
    inner = WakeWordTrainer.train_indexed

    def train_indexed(self, idx, y, sched, *a, history=None, **kw):
        if history is not None and history.shape[0] > 8:  # not bench.py's 8-step train_probe
            seen[history.data_ptr()] = (history, int(idx.shape[1]), self, idx, y, kw.get("pool32"), kw.get("pool16"))
        return inner(self, idx, y, sched, *a, history=history, **kw)

    WakeWordTrainer.train_indexed = train_indexed
    import bench
    sys.argv = ["bench.py", *bench_args]
    rc = bench.main()
    torch.cuda.synchronize()
    res = {"bench_args": bench_args, "buffers": []}
    def reforward(tr, idx, y, pool32, pool16, steps):
        """The live 16-row tiles themselves (the history has no per-row data): the chunk's last
        ``steps`` batches classified again with the FINAL weights (dropout on, another mask),
        filtered as the step filters, counted per tile. -> (n_sel, live tiles) per batch."""
        plan, params = tr.model.plan, tr.model.flat_parameters.detach().contiguous()
        p32, p16 = pool32.reshape(pool32.shape[0], -1), pool16.reshape(pool16.shape[0], -1)
        out = []
        for s in range(idx.shape[0] - steps, idx.shape[0]):
            i = idx[s].long()
            x = torch.where((i >= 0)[:, None], p32[i.clamp(min=0)], p16[(-i - 1).clamp(min=0)].float())
            p = plan.forward(params, x, dropout_p=float(tr.model.dropout.p), seed=s)
            sel = torch.where(y == 1, p < 1 - 1e-4, p >= 1e-4)
            pad = torch.zeros(-(-len(sel) // 16) * 16, dtype=torch.bool, device=sel.device)
            pad[:len(sel)] = sel
            out.append((int(sel.sum()), int(pad.view(-1, 16).any(1).sum())))
        return np.array(out, np.float64)

    for hist, B, tr, idx, y, pool32, pool16 in seen.values():
        h = hist.cpu().numpy().astype(np.float64)
        h = h[h[:, 1] > 0] if (h[:, 1] > 0).any() else h  # rows a step wrote (accumulation steps >= 1)
        n = h[:, 0]
        tiles_lo = np.ceil(n / 16)  # (the tiles themselves: reforward below)
        steps32 = np.ceil(n / 32)

        def dist(v):
            return {"mean": round(float(v.mean()), 2), "median": float(np.median(v)),
                    "p95": float(np.percentile(v, 95)), "max": float(v.max()), "min": float(v.min())}
        res["buffers"].append({
            "batch_rows": B, "train_steps": int(len(n)), "n_sel": dist(n), "share_of_batch_median": round(float(np.median(n)) / B, 4),
            "n_neg_sel": dist(h[:, 4]), "n_pos_sel": dist(h[:, 6]),
            "live_16row_tiles_lower_bound": dist(tiles_lo), "dense_16row_tiles": -(-B // 16),
            "compacted_32row_steps": dist(steps32), "dense_32row_steps": -(-B // 32),
            # column 2 (fired): the steps whose update ran; the others' gradients are dropped
            # (the < 128-sample gate). pairs: (this step, the next) fired -> count
            "fired_share": round(float((h[:, 2] > 0).mean()), 3), "fired_steps": int((h[:, 2] > 0).sum()),
            "n_sel_below_128_share": round(float((n < 128).mean()), 3),
            "fired_pairs": {f"{int(a)}{int(b)}": int(((h[:-1, 2] > 0) == a).__and__((h[1:, 2] > 0) == b).sum())
                            for a in (0, 1) for b in (0, 1)}})
        if pool32 is not None and pool16 is not None:
            rf = reforward(tr, idx, y, pool32, pool16, min(200, idx.shape[0]))
            res["buffers"][-1]["reforward_last_200_batches_final_weights"] = {
                "n_sel": dist(rf[:, 0]), "live_16row_tiles": dist(rf[:, 1]),
                "live_32row_steps": dist(np.ceil(rf[:, 1] / 2))}
    line = json.dumps(res)
    print("NSEL " + line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    sys.exit(rc or 0)


if __name__ == "__main__":
    main()
