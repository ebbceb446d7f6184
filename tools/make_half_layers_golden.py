"""tests/golden/classifier_half*.npz: the reference's half-layer classifier
(WakeWordMLPModel(use_half_layers=True), WakeWordTrainer(use_half_layers=True)) on the
seeded inputs of tests/half_layers_cases.py. Development machines only: it imports
the reference package through oracle.make_golden.import_reference().

    python tools/make_half_layers_golden.py [--check]

Stored (dropout p = 0, as in oracle/golden_classifier.py):
  names, shapes      the reference's state dict, in order ("shape/<name>")
  prob, logit        forward of the 96-row batch
  loss, n_sel, grad/ the trainer's filtered weighted BCE at neg_weight 2 and its autograd
                     gradients, on the stored subset (half_layers_cases.stored)
  epoch/, epoch_final/   the 24-step train_epoch (warmup 4, hold 8): six histories and
                     the final parameters on the stored subset
--check also runs the reference's forward and gradients in float64 and prints how far
its own float32 results are from that (the floor under the tests' bounds).
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import half_layers_cases as hc  # noqa: E402
from oracle import golden_classifier as gc  # noqa: E402
from oracle.make_golden import import_reference  # noqa: E402


def _load(model, params, dtype):
    import torch
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    model.dropout.p = 0.0
    return model.to(dtype)


def run(hb, dtype, epoch=True):
    import torch
    torch.manual_seed(0)
    base, x, y, np_batches = gc.golden_inputs()
    model = hb.wakeword.WakeWordMLPModel(use_half_layers=True)
    names = list(model.state_dict())
    params = hc.with_half_params(base, names)
    assert list(params) == list(hc.golden_inputs()[0]) and list(model.half_indices) == hc.HALF_INDICES
    _load(model, params, dtype)
    out = {"names": np.array(names)}
    for k, v in model.state_dict().items():
        out[f"shape/{k}"] = np.array(v.shape)
    logits = {}
    hook = model.mlp_out.register_forward_hook(lambda m, i, o: logits.__setitem__("z", o.detach()))
    xt, yt = torch.from_numpy(x).to(dtype), torch.from_numpy(y)
    p = model(xt)
    hook.remove()
    out["prob"] = p.detach().numpy()[:, 0]
    out["logit"] = logits["z"].numpy()[:, 0]
    # one step of the trainer's loss (trainer.py:407-445), neg weight 2, accumulation steps 1
    thr, nw = 1e-4, 2.0
    sel_neg = (yt == 0) & (p.squeeze() >= thr)
    sel_pos = (yt == 1) & (p.squeeze() < 1 - thr)
    ys = torch.cat([yt[sel_neg], yt[sel_pos]]).to(dtype)
    ps = torch.cat([p[sel_neg], p[sel_pos]])
    w = torch.ones(ys.shape[0], dtype=dtype) * nw
    w[ys == 1] = 1.0
    loss = torch.nn.functional.binary_cross_entropy(ps, ys.unsqueeze(1), w.unsqueeze(1))
    model.zero_grad()
    loss.backward()
    out["loss"] = np.array(loss.item())
    out["n_sel"] = np.array(ps.shape[0])
    for k, prm in model.named_parameters():
        if hc.stored(k, prm.numel()):
            out[f"grad/{k}"] = prm.grad.numpy().copy()
    if not epoch:
        return out
    batches = [(torch.from_numpy(xb).to(dtype), torch.from_numpy(yb)) for xb, yb in np_batches]
    with tempfile.TemporaryDirectory() as ck:
        trainer = hb.trainer.WakeWordTrainer(checkpoint_dir=ck, use_half_layers=True)
        _load(trainer.model, params, dtype)
        hist = trainer.train_epoch(batches, num_steps=len(batches), warmup_steps=4, hold_steps=8,
                                   validation_steps=1000, checkpoint_steps=100000)
        for n, h in zip(["lr", "nw", "loss", "hlr", "recall", "fp"], hist[:6]):
            out[f"epoch/{n}"] = h.numpy()
        moved = []
        for k, prm in trainer.model.named_parameters():
            moved.append(np.abs(prm.detach().numpy().astype(np.float64) - params[k]).ravel())
            if hc.stored(k, prm.numel()):
                out[f"epoch_final/{k}"] = prm.detach().numpy().copy()
        print(f"the epoch moved parameters by {np.concatenate(moved).mean():.3e} on average")
    return out


def main() -> None:
    import torch
    hb = import_reference()
    out = run(hb, torch.float32)
    if "--check" in sys.argv:
        ref = run(hb, torch.float64, epoch=False)  # (the reference's train_epoch casts to float32)
        print("logit   f32 vs f64:", np.abs(out["logit"] - ref["logit"]).max())
        worst = max(((np.abs(out[k] - ref[k]).max() / (np.abs(ref[k]).max() + 1e-12), k)
                     for k in out if k.startswith("grad/")))
        print("grad    f32 vs f64 (of the tensor's max):", worst)
    # three files, so that each stays under the repository's 1 MiB limit for a committed file
    # (half_layers_cases.load_gold reads them back as one record)
    for path, keys in hc.split_gold(out).items():
        np.savez_compressed(path, **{k: out[k] for k in keys})
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20), path


if __name__ == "__main__":
    main()
