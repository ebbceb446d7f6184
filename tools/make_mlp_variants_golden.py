"""tests/golden/classifier_variants_*.npz: the reference's classifier with plain MLP blocks
(WakeWordMLPModel(use_gating=False)) and with every activation get_activation names, on the
seeded inputs of oracle.golden_classifier.golden_inputs(). Development machines only: it
imports the reference package through oracle.make_golden.import_reference().

    python tools/make_mlp_variants_golden.py [--check]

Stored per variant ({gated, plain} x 7 activations without gated SiLU: 13), under
"<variant>/" (mlp_variants_cases.key), at dropout p = 0 as in oracle/golden_classifier.py:
  names, shape/      the reference's state dict, in order
  prob, logit        forward of the 96-row batch
  loss, n_sel, grad/ the trainer's filtered weighted BCE at neg_weight 2 and its autograd
                     gradients, on the stored subset (mlp_variants_cases.stored)
  epoch/, epoch_final/   for mlp_variants_cases.EPOCH_VARIANTS: the 24-step train_epoch (warmup 4,
                     hold 8): six histories and the final parameters on the stored subset
--check also runs the reference's forward and gradients in float64 and prints how far its own
float32 results are from that (the floor under the tests' bounds).
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mlp_variants_cases as vc  # noqa: E402
from oracle.make_golden import import_reference  # noqa: E402


def _load(model, params, dtype):
    import torch
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    model.dropout.p = 0.0
    return model.to(dtype)


def run(hb, gated, act, dtype, epoch):
    import torch
    torch.manual_seed(0)
    params, x, y, np_batches = vc.golden_inputs(gated)
    model = hb.wakeword.WakeWordMLPModel(use_gating=gated, activation=act)
    names = list(model.state_dict())
    assert names == list(params), (names, list(params))
    assert sum(p.numel() for p in model.parameters()) == vc.N_PARAMS[gated]
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
        if vc.stored(k, prm.numel()):
            out[f"grad/{k}"] = prm.grad.numpy().copy()
    if not epoch:
        return out
    batches = [(torch.from_numpy(xb).to(dtype), torch.from_numpy(yb)) for xb, yb in np_batches]
    with tempfile.TemporaryDirectory() as ck:
        trainer = hb.trainer.WakeWordTrainer(checkpoint_dir=ck, use_gating=gated, activation=act)
        _load(trainer.model, params, dtype)
        hist = trainer.train_epoch(batches, num_steps=len(batches), warmup_steps=4, hold_steps=8,
                                   validation_steps=1000, checkpoint_steps=100000)
        for n, h in zip(["lr", "nw", "loss", "hlr", "recall", "fp"], hist[:6]):
            out[f"epoch/{n}"] = h.numpy()
        for k, prm in trainer.model.named_parameters():
            if vc.stored(k, prm.numel()):
                out[f"epoch_final/{k}"] = prm.detach().numpy().copy()
    return out


def main() -> None:
    import torch
    hb = import_reference()
    files = {True: {}, False: {}}
    floor_z, floor_g = (0.0, ""), (0.0, "")
    for gated, act in vc.VARIANTS:
        v = vc.key(gated, act)
        out = run(hb, gated, act, torch.float32, (gated, act) in vc.EPOCH_VARIANTS)
        print(v, "n_sel", int(out["n_sel"]), "of", len(out["prob"]), "loss", float(out["loss"]))
        if "--check" in sys.argv:
            ref = run(hb, gated, act, torch.float64, False)  # (the reference's train_epoch casts to float32)
            floor_z = max(floor_z, (float(np.abs(out["logit"] - ref["logit"]).max()), v))
            floor_g = max(floor_g, max((float(np.abs(out[k] - ref[k]).max() / (np.abs(ref[k]).max() + 1e-12)),
                                        f"{v}/{k}") for k in out if k.startswith("grad/")))
        files[gated].update({f"{v}/{k}": a for k, a in out.items()})
    if "--check" in sys.argv:
        print("logit   f32 vs f64, worst variant:", floor_z)
        print("grad    f32 vs f64 (of the tensor's max), worst tensor:", floor_g)
    for gated, record in files.items():
        path = vc.gold_path(gated)
        np.savez_compressed(path, **record)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20), path


if __name__ == "__main__":
    main()
