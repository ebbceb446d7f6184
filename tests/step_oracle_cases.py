"""Seeded inputs, float64 references and the shared comparisons of the train-step
tests (never collected by pytest; imported by tests/test_train_step_oracle_gpu.py,
tests/v2_forced_worker.py and the fixture-pinned classifier tests). numpy only.

Candidates: default_rng(2025), 6,000 rows, y ~ Bernoulli(0.25), x = N(0, 1) +
(0.8 if y else -0.2) in f32; the negative rows are rounded through f16 and live in
``pool16``, the positives in ``pool32`` (the oracle sees the rounded values).
"Wide" parameters Q: the golden parameters P0 with mlp_out.output.weight x 120 and
the output bias set so that the median candidate logit is 0: under Q the high-loss
filter (negatives with p >= 1e-4, positives with p < 1 - 1e-4) rejects rows.
Under a parameter set the candidates are classified by their float64 logit z, with
T = logit(1e-4) = -9.21:
  U (filtered with margin): negatives with z < T - 0.25, positives with z > -T + 0.25
  S (kept with margin):     0.05 <= |z| <= 6
and nothing else is ever used: 0.25 logits is ~2,000 x the f32 logit error, and with
|z| <= 6 log(1 - p) in f32 stays inside the 1e-5 loss bound.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np

from oracle import golden_classifier as gc
from oracle import mlp as omlp

D = 1536
N_CAND = 6000
T = math.log(1e-4 / (1.0 - 1e-4))
MARGIN = 0.25
NEG_WEIGHT = 1.5
DROP_P, DROP_SEED = 0.1, 0x5EED1234ABC


class World:
    """The candidates, their pools and the two parameter sets (built once)."""

    def __init__(self):
        self.P0 = gc.golden_inputs()[0]
        rng = np.random.default_rng(2025)
        y = (rng.random(N_CAND) < 0.25).astype(np.int64)
        x = (rng.standard_normal((N_CAND, D)) + np.where(y[:, None] == 1, 0.8, -0.2)).astype(np.float32)
        neg = y == 0
        x[neg] = x[neg].astype(np.float16).astype(np.float32)
        self.x, self.y = x, y
        self.pool32 = np.ascontiguousarray(x[~neg])
        self.pool16 = np.ascontiguousarray(x[neg].astype(np.float16))
        self.n32, self.n16 = len(self.pool32), len(self.pool16)
        # candidate c is row idx[c] of the step ABI: >= 0 -> pool32, < 0 -> pool16 row -i - 1
        idx = np.empty(N_CAND, np.int64)
        idx[~neg] = np.arange(self.n32)
        idx[neg] = -np.arange(self.n16) - 1
        self.idx = idx.astype(np.int32)
        Q = OrderedDict((k, v.copy()) for k, v in self.P0.items())
        Q["mlp_out.output.weight"] = (Q["mlp_out.output.weight"] * np.float32(120.0)).astype(np.float32)
        Q["mlp_out.output.bias"] = np.zeros_like(Q["mlp_out.output.bias"])
        z = omlp.forward(Q, x)[1]
        Q["mlp_out.output.bias"] = np.array([-np.median(z)], np.float32)
        self.Q = Q
        for a in (self.x, self.y, self.pool32, self.pool16, self.idx):
            a.setflags(write=False)

    def classify(self, params):
        """(U, S) candidate index arrays under ``params`` (float64 logits)."""
        z = omlp.forward(params, self.x)[1]
        U = np.where(self.y == 0, z < T - MARGIN, z > -T + MARGIN)
        S = (np.abs(z) >= 0.05) & (np.abs(z) <= 6.0)
        return np.flatnonzero(U), np.flatnonzero(S)


_world = None


def world() -> World:
    global _world
    if _world is None:
        _world = World()
    return _world


def margins_ok(z, y) -> bool:
    """Every row at least MARGIN logits from the threshold the filter compares it with."""
    thr = np.where(np.asarray(y) == 0, T, -T)
    return bool((np.abs(z - thr) >= MARGIN).all())


class Layout:
    """One single-step case: ``rows`` index the candidates (-1: an out-of-range idx,
    a zero row labelled 0); ``idx`` / ``y`` are what the device gets, ``x`` what the
    oracle gets."""

    def __init__(self, name, params, rows, bad_idx=(), pool32=True, dropout=False):
        w = world()
        self.name, self.params, self.pool32, self.dropout = name, params, pool32, dropout
        rows = np.asarray(rows, np.int64)
        self.B = len(rows)
        live = rows >= 0
        self.y = np.where(live, w.y[np.maximum(rows, 0)], 0).astype(np.int64)
        self.idx = np.where(live, w.idx[np.maximum(rows, 0)], 0).astype(np.int64)
        assert (~live).sum() == len(bad_idx)
        self.idx[~live] = bad_idx
        self.idx = self.idx.astype(np.int32)
        x = np.where(live[:, None], w.x[np.maximum(rows, 0)], np.float32(0.0)).astype(np.float32)
        if dropout:  # the kernels' mask of step 0, salt 0: rows arange(B); kept elements scaled in f32
            keep = omlp.dropout_keep(DROP_SEED, np.arange(self.B), D, DROP_P)
            scale = np.float32(1.0) / (np.float32(1.0) - np.float32(DROP_P))
            x = np.where(keep, x * scale, np.float32(0.0)).astype(np.float32)
        self.x = x
        self._ref = None

    def reference(self):
        """(gradients by name, stats [8], prob [B], logits [B]) in float64, computed once."""
        if self._ref is None:
            flat, stats = omlp.flat_bucket(self.params, self.x, self.y, neg_weight=NEG_WEIGHT)
            prob, z, _ = omlp.forward(self.params, self.x)
            grads, o = OrderedDict(), 0
            for k, v in self.params.items():
                grads[k] = flat[o:o + v.size].reshape(v.shape)
                o += v.size
            for a in (stats, prob, z, *grads.values()):
                a.setflags(write=False)
            self._ref = (grads, stats, prob, z)
        return self._ref


def _take(rng, pool, n):
    return rng.choice(pool, n, replace=False)


_layouts = None


def layouts() -> "OrderedDict[str, Layout]":
    """The single-step layouts (see tests/test_train_step_oracle_gpu.py); every
    precondition is asserted here, on the oracle alone."""
    global _layouts
    if _layouts is not None:
        return _layouts
    w = world()
    U, S = w.classify(w.Q)
    assert len(U) >= 1000 and len(S) >= 1000, (len(U), len(S))
    out = OrderedDict()
    rng = np.random.default_rng(41)
    dense = _take(rng, N_CAND, 1100)
    out["dense-1100"] = Layout("dense-1100", w.P0, dense)
    zr = dense.copy()
    zr[[5, 600, 1099]] = -1  # a first-tile row, a middle row and the last row of the ragged tail tile
    out["zero-rows-1100"] = Layout("zero-rows-1100", w.P0, zr, bad_idx=(w.n32, 2 ** 31 - 1, -w.n16 - 1))
    neg = np.flatnonzero(w.y == 0)
    zr16 = _take(rng, neg, 1100)
    zr16[[5, 600, 1099]] = -1  # without pool32 every idx >= 0 is out of range
    out["zero-rows-f16-1100"] = Layout("zero-rows-f16-1100", w.P0, zr16, bad_idx=(0, 2 ** 31 - 1, -w.n16 - 1),
                                       pool32=False)
    # sparse: rows 0-127 filtered (a whole k3s split, eight whole tiles), 128-143 filtered but row 135,
    # 144-655 a seeded 50/50 mix, 656-1087 kept, 1088-1099 filtered (the ragged tail tile)
    u, s = rng.permutation(U), rng.permutation(S)
    mix = rng.random(512) < 0.5
    rows = np.empty(1100, np.int64)
    from_u = np.ones(1100, bool)
    from_u[135] = False
    from_u[144:656] = mix
    from_u[656:1088] = False
    rows[from_u] = u[:from_u.sum()]
    rows[~from_u] = s[:(~from_u).sum()]
    out["sparse-1100"] = Layout("sparse-1100", w.Q, rows)
    # few: 701 filtered rows, then 100 kept ones (n_sel = 100 < 128); Bp = 816, one live row in the last tile
    out["few-801"] = Layout("few-801", w.Q, np.concatenate([_take(rng, U, 701), _take(rng, S, 100)]))
    out["none-800"] = Layout("none-800", w.Q, _take(rng, U, 800))
    out["dropout-1100"] = Layout("dropout-1100", w.P0, dense, dropout=True)
    for lay in out.values():
        _, stats, _, z = lay.reference()
        assert margins_ok(z, lay.y), lay.name
        if lay.params is w.P0:
            assert stats[0] == lay.B, lay.name  # every row selected
        else:
            sel = np.abs(z) < -T  # the selected rows' loss stays inside the f32 bound
            assert (np.abs(z[sel]) <= 6.0).all() and stats[0] == sel.sum(), lay.name
    st = out["sparse-1100"].reference()[1]
    assert st[0] == (~from_u).sum() and 0 < st[2] < st[0]
    assert out["few-801"].reference()[1][0] == 100 and out["none-800"].reference()[1][0] == 0
    _layouts = out
    return out


def forced_layouts() -> "OrderedDict[str, Layout]":
    """The forced-v2 child's single-step cases: dense rows on P0 at small batches, and at
    B = 273 a sparse layout on Q (the first 128 rows filtered, the rest mixed)."""
    w = world()
    U, S = w.classify(w.Q)
    out = OrderedDict()
    rng = np.random.default_rng(43)
    for B in (1, 15, 16, 17, 33, 129, 273, 550):
        out[f"dense-{B}"] = Layout(f"dense-{B}", w.P0, _take(rng, N_CAND, B))
    u, s = rng.permutation(U), rng.permutation(S)
    from_u = np.ones(273, bool)
    from_u[128:] = rng.random(145) < 0.5
    rows = np.empty(273, np.int64)
    rows[from_u] = u[:from_u.sum()]
    rows[~from_u] = s[:(~from_u).sum()]
    out["sparse-273"] = Layout("sparse-273", w.Q, rows)
    for lay in out.values():
        _, stats, _, z = lay.reference()
        assert margins_ok(z, lay.y), lay.name
    assert out["sparse-273"].reference()[1][0] == (~from_u).sum()
    return out


# ------------------------------------------------------------ comparisons ----
def check_bucket(lay: Layout, grads, stats, prob) -> None:
    """A step's bucket against the float64 oracle: counts exact, loss sum 1e-5, prob
    1e-6 + 1e-4 relative, every gradient tensor within 1e-4 of that tensor's max |g_ref|
    (the bound of test_fused_grads_match_reference). grads: {name: array}."""
    g_ref, s_ref, p_ref, _ = lay.reference()
    stats = np.asarray(stats, np.float64)
    print(f"{lay.name}: n_sel {stats[0]:.0f}, loss sum rel err "
          f"{abs(stats[1] - s_ref[1]) / max(abs(s_ref[1]), 1e-30):.2e}, "
          f"prob max err {np.abs(np.asarray(prob) - p_ref).max():.2e}")
    np.testing.assert_array_equal(stats[[0, 2, 3, 4, 5, 6]], s_ref[[0, 2, 3, 4, 5, 6]], err_msg=lay.name)
    np.testing.assert_allclose(stats[1], s_ref[1], rtol=1e-5, err_msg=lay.name)
    assert stats[7] == 0.0
    np.testing.assert_allclose(prob, p_ref, rtol=1e-4, atol=1e-6, err_msg=lay.name)
    worst = 0.0
    for k, ref in g_ref.items():
        g = np.asarray(grads[k], np.float64)
        assert np.isfinite(g).all(), f"{lay.name} {k}: non-finite gradient"
        scale = np.abs(ref).max()
        if scale == 0.0:
            assert not g.any(), f"{lay.name} {k}: the oracle's gradient is exactly zero"
            continue
        err = np.abs(g - ref).max() / scale
        worst = max(worst, err)
        assert err <= 1e-4, f"{lay.name} {k}: max |g - g_ref| = {err:.2e} of max |g_ref|"
    print(f"{lay.name}: worst gradient tensor {worst:.2e} of its max |g_ref|")


def check_step_against_gold(gold, params, stats, prob, grads_over_n) -> None:
    """The B = 96 fixture step (tests/golden/classifier.npz): n_sel exact, loss 1e-5, prob
    1e-4 / 1e-6, gradients (already divided by n_sel) 1e-4 of each tensor's max |g|."""
    n_sel = int(gold["n_sel"])
    assert int(stats[0]) == n_sel
    np.testing.assert_allclose(stats[1] / n_sel, float(gold["loss"]), rtol=1e-5)
    np.testing.assert_allclose(prob, gold["prob"], rtol=1e-4, atol=1e-6)
    for k in params:
        ref = gold[f"grad/{k}"]
        scale = np.abs(ref).max() + 1e-12
        np.testing.assert_allclose(np.asarray(grads_over_n[k]) / scale, ref / scale, rtol=0, atol=1e-4, err_msg=k)


def check_epoch_against_gold(gold, params, lr, hlr, loss, rec, fp, final) -> None:
    """The 24-step train_epoch against the reference's run. The oracle's bounds
    (test_classifier_oracle.py): loss 2e-4; final parameters within 2e-4 except Adam's
    sign flips where a gradient sits at the fp32 noise floor (each flip moves a weight by
    up to 2 lr): at most 0.5 % of the 256,417 parameters, as in test_stages_gpu.py."""
    np.testing.assert_allclose(lr, gold["epoch/lr"], rtol=1e-6)
    np.testing.assert_allclose(hlr, gold["epoch/hlr"], rtol=1e-6)
    assert loss.shape == gold["epoch/loss"].shape
    np.testing.assert_allclose(loss, gold["epoch/loss"], rtol=2e-4, atol=1e-7)
    np.testing.assert_allclose(rec, gold["epoch/recall"], atol=1e-6)
    np.testing.assert_allclose(fp, gold["epoch/fp"], atol=1e-6)
    diffs = np.concatenate([np.abs(np.asarray(final[k]) - gold[f"epoch_final/{k}"]).ravel() for k in params])
    assert (diffs > 2e-4).mean() <= 5e-3, (diffs > 2e-4).mean()
    assert diffs.max() <= 5e-3, diffs.max()  # a flipped element: a few lr-sized steps at most


def check_stages_against_gold(gold, params, h, fetched_sizes, final) -> None:
    """The 3-stage WakeWordTrainer.__call__ against the reference's run (bounds: the
    docstring of tests/test_stages_gpu.py). h: {name: array}; fetched_sizes: the size of
    every batch the iterator yielded."""
    lens = list(gold["stage_lengths"])
    assert lens == [8, 16, 32]
    sizes, o = [], 0
    for n in lens:  # one batch per stage is fetched past the last step, as in the reference
        sizes += list(fetched_sizes[o:o + n])
        o += n + 1
    np.testing.assert_array_equal(sizes, gold["batch_sizes"])
    np.testing.assert_allclose(h["lr"], gold["hist/learning_rate"], rtol=1e-6)
    np.testing.assert_allclose(h["nw"], gold["hist/negative_weight"], rtol=1e-6)
    np.testing.assert_allclose(h["hlr"], gold["hist/high_loss_rate"], rtol=1e-6)
    np.testing.assert_allclose(h["vfp"], gold["hist/validation_false_positive_rate_per_hour"], rtol=1e-6)
    np.testing.assert_allclose(h["vrecall"], gold["hist/validation_recall"], atol=1e-6)
    np.testing.assert_allclose(h["recall"], gold["hist/recall"], atol=1e-6)
    np.testing.assert_allclose(h["fp"], gold["hist/false_positive_rate"], atol=1e-6)
    np.testing.assert_allclose(h["loss"], gold["hist/loss"], rtol=2e-4, atol=1e-7)
    d = np.concatenate([np.abs(np.asarray(final[k]) - gold[f"final/{k}"]).ravel() for k in params])
    bound = 2 * float(np.sum(gold["hist/learning_rate"]))
    assert float(np.mean(d <= 2e-4)) >= 0.995, float(np.mean(d <= 2e-4))
    assert float(d.max()) <= bound, (float(d.max()), bound)


# -------------------------------------------------- gated multi-step walk ----
GATED_B, GATED_POS = 800, 200
GATED_LR = 2e-4
GATED_NSEL = (60, 60, 40, 0, 300, 90)


def gated_walk(dtype=np.float64, plan=None, start=None):
    """Six steps from ``start`` (default Q) at B = 800 (200 positives, then 600 negatives) through the oracle
    (forward, step_loss_and_dz, backward, Adam and the < 128-sample gate of
    omlp.train_epoch). Before each step the candidates are classified under the float64
    walk's CURRENT parameters and the step's rows composed from U and S, the filtered rows
    first inside each label block, for GATED_NSEL selected rows. ``plan``: the rows of an
    earlier (float64) walk, replayed in another dtype. Returns a dict: rows [6, 800]
    (candidates), hist [6, 8] (the device history's columns), params, m, fired lrs."""
    w = world()
    start = w.Q if start is None else start
    params = OrderedDict((k, np.asarray(v, dtype=dtype)) for k, v in start.items())
    opt = omlp.Adam(params)
    opt.m = OrderedDict((k, v.astype(dtype)) for k, v in opt.m.items())
    opt.v = OrderedDict((k, v.astype(dtype)) for k, v in opt.v.items())
    y = np.concatenate([np.ones(GATED_POS), np.zeros(GATED_B - GATED_POS)]).astype(np.int64)
    acc_steps, acc_samples = 1, 0
    rows_all, hist, fired_lr = [], np.zeros((len(GATED_NSEL), 8)), []
    for step, n in enumerate(GATED_NSEL):
        if plan is None:
            rng = np.random.default_rng(100 + step)
            U, S = w.classify(params)
            # a quarter of the selected rows positive, more where too few positives are filtered
            n_pos = min(n, max(n // 4, GATED_POS - int((w.y[U] == 1).sum())))
            parts = []
            for label, total, k in ((1, GATED_POS, n_pos), (0, GATED_B - GATED_POS, n - n_pos)):
                u, s = U[w.y[U] == label], S[w.y[S] == label]
                assert len(u) >= total - k and len(s) >= k, (step, label, len(u), len(s))
                parts += [_take(rng, u, total - k), _take(rng, s, k)]
            rows = np.concatenate(parts)
        else:
            rows = plan[step]
        rows_all.append(rows)
        x = w.x[rows]
        prob, z, cache = omlp.forward(params, x, dtype=dtype)
        if plan is None:
            assert margins_ok(z, y), step
        sel = omlp.select_high_loss(prob, y)
        h = hist[step]
        h[0], h[1] = sel.size, acc_steps
        if sel.size:
            loss, ns, dz = omlp.step_loss_and_dz(prob, y, NEG_WEIGHT, 1e-4, acc_steps)
            ps, ys = prob[sel], y[sel]
            h[3] = loss
            h[4], h[5] = (ys == 0).sum(), ((ys == 0) & (ps >= 0.5)).sum()
            h[6], h[7] = (ys == 1).sum(), ((ys == 1) & (ps > 0.5)).sum()
            acc_samples += ns
            if acc_samples < 128:
                acc_steps += 1
            else:
                grads = omlp.backward(params, cache, dz.astype(dtype), dtype)
                params = opt.step(params, grads, GATED_LR)
                acc_steps, acc_samples = 1, 0
                h[2] = 1.0
                fired_lr.append(GATED_LR)
    if plan is None:
        assert list(hist[:, 0]) == list(GATED_NSEL)
        assert (hist[:, 2] == 0).sum() >= 2 and (hist[:, 2] == 1).sum() >= 2 and (hist[:, 0] == 0).any()
    return {"rows": np.stack(rows_all), "y": y, "hist": hist, "params": params, "m": opt.m, "fired_lr": fired_lr}


def gated_figures(params, m, ref, start=None) -> dict:
    """The three multi-step figures of a run against the float64 walk ``ref``: the share of
    parameters differing by > 1e-5, |dP - dP_ref|_2 / |dP_ref|_2 (dP = P_final - P_init)
    and, per tensor, max |m - m_ref| / max |m_ref|; and max |P - P_ref|."""
    start = world().Q if start is None else start  # the walk's initial parameters
    cat = lambda d: np.concatenate([np.asarray(d[k], np.float64).ravel() for k in start])  # noqa: E731
    p, pr, p0 = cat(params), cat(ref["params"]), cat(start)
    return {
        "share": float((np.abs(p - pr) > 1e-5).mean()),
        "drift": float(np.linalg.norm((p - p0) - (pr - p0)) / np.linalg.norm(pr - p0)),
        "m": {k: float(np.abs(np.asarray(m[k], np.float64) - ref["m"][k]).max() / np.abs(ref["m"][k]).max())
              for k in start},
        "max": float(np.abs(p - pr).max()),
    }
