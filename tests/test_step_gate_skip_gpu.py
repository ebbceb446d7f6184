"""HBK_STEP_GATE_SKIP: a train step whose accumulation gate will not fire computes no weight
gradient (k3s / k3_wgrad leave in their prologue) and its update touches neither parameters,
moments nor weight cache, and reads no slab (k4 resolves the gate first). train_indexed sets the
flag whenever it defers the slabs; HBK_STEP_GATE_SKIP=0 in the environment (read by every
step call) makes the library ignore it.

Walks (tests/step_oracle_cases.py, the float64 oracle; B = 800: 200 f32 positives, then 600 f16
negatives, lr 2e-4, dropout off):
  walk6  gated_walk as it stands: n_sel = 60, 60, 40, 0, 300, 90 -> no, no, fire, no, fire, no
  walk8  the same function over n_sel = 60, 0, 30, 60, 100, 20, 300, 90 -> fires at steps 3 and 6;
         with steps_per_graph = 2 the first step runs eagerly and ONE captured two-step graph
         is replayed over steps (1, 2), (3, 4), (5, 6) = (no, no), (fire, no), (no, fire)
Variants: v2 (k3s) on the 64-CU masked stream, where B = 800 is the smallest batch the library
gives v2; v1 (k3_wgrad_kernel) on the whole device. The whole device takes v1 at every batch,
so v1 runs the same B = 800 walks: the float64 references exist there, and three 16-row tiles
would exercise nothing the 50 tiles do not (the exit is uniform, taken in every workgroup's
prologue). step_variant is asserted in both.

1  stale slabs: from a workspace of 0xFF bytes (NaN in f32 and f16), step by step through walk6.
   After every step that does not fire (the first two, the n_sel = 0 one, the last) parameters,
   m, v and the weight-cache planes keep their bits; after the first fire everything is finite;
   after the walk the figures of test_gated_steps_match_oracle hold (4 x the f32 walk's).
2  the decision is read on every replay: walk8, history columns 0, 1, 2, 4-7 exact, loss 2e-4.
3  skip on against HBK_STEP_GATE_SKIP=0, twice off and once on, walk6. History columns 0, 1, 2,
   4-7 and both state halves equal; the loss column within the 2e-4 of the other gated tests,
   not bit for bit: it is k2's float-atomic sum over the tiles, whose order changes from run
   to run on the parent too. At the first fire (step 2; until then the parameters have the
   same bits in every run) the tensors whose gradients come from the slabs (norm_in, every
   hidden / gate / output weight: plain stores, summed in a fixed order) have the same bits of
   parameters, m and v in all three runs. The other tensors (biases, LayerNorm(96): k2's float
   atomics) are compared on Adam's m there, m = 0.1 g / (n_sel steps): linear in the gradient,
   where the parameter itself moves by lr sign(g) and flips on a gradient at the noise floor.
   Figure: max over those tensors of max |m_a - m_b| / max |m_a|. Off against off, measured on
   one MI355X: 1.207e-7 (v2) and 1.576e-7 (v1), RUN_TO_RUN below (one f32 rounding of a tile's
   atomic sum); on against off must stay within 4 x that, the margin the gated tests give the
   f32 walk: 4.8e-7 and 6.3e-7. Measured on against off in the same run: 1.207e-7 and 1.576e-7.
4  v1: cases 1 and 3 with variant = v1.
5  the flag without HBK_STEP_DEFER_PARTIALS is refused (HBK_ERR_ARG).
"""
import numpy as np
import pytest
import torch

import step_oracle_cases as sc
from test_train_step_oracle_gpu import GATED_DRIFT_F32, GATED_M_F32, GATED_SHARE_F32, _on_variant_stream

pytestmark = pytest.mark.gpu

NSEL8 = (60, 0, 30, 60, 100, 20, 300, 90)
K3S_TENSORS = ("norm_in.weight", "norm_in.bias", ".hidden.weight", ".gate.weight", ".output.weight")
# the skip-off configuration against itself (two runs, the figure of case 3): v2 / v1
RUN_TO_RUN = {"v2": 1.207e-7, "v1": 1.576e-7}


def _from_slabs(name):
    return name.startswith("norm_in.") or name.endswith(K3S_TENSORS[2:])


@pytest.fixture(scope="module")
def walk6():
    g = sc.gated_walk()
    assert list(g["hist"][:, 2]) == [0, 0, 1, 0, 1, 0]
    return g


@pytest.fixture(scope="module")
def walk8():
    keep = sc.GATED_NSEL
    sc.GATED_NSEL = NSEL8  # (gated_walk reads the module's tuple; its own preconditions are asserted inside)
    try:
        g = sc.gated_walk()
    finally:
        sc.GATED_NSEL = keep
    f = list(g["hist"][:, 2])
    assert list(g["hist"][:, 0]) == list(NSEL8)
    assert [(f[1], f[2]), (f[3], f[4]), (f[5], f[6])] == [(0, 0), (1, 0), (0, 1)]
    return g


@pytest.fixture(scope="module")
def dev():
    from heybuddy.pipeline import masked_stream, train_cu_set
    w = sc.world()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ms = masked_stream(torch.device("cuda", 0), train_cu_set(n_cu, 64))
    return {"pool32": torch.from_numpy(w.pool32.copy()).cuda(), "pool16": torch.from_numpy(w.pool16.copy()).cuda(),
            "ms": ms}


class Run:
    """One trainer on Q over a walk's rows; step(n) runs the next n steps on the variant's stream."""

    def __init__(self, dev, variant, walk, tmp_path, stale=False, steps_per_graph=2):
        from heybuddy.trainer import WakeWordTrainer
        w = sc.world()
        self.dev, self.variant, self.spg = dev, variant, steps_per_graph
        self.S, self.B = walk["rows"].shape
        tr = self.tr = WakeWordTrainer(checkpoint_dir=str(tmp_path), device="cuda")
        tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.Q.items()}, strict=True)
        tr.model.dropout.p = 0.0
        tr._reset_accumulation()
        self.plan = tr.model.plan
        if stale:
            tr._indexed_ws = torch.full((self.plan.workspace_bytes(self.B),), 0xFF, dtype=torch.uint8, device="cuda")
        self.idx = torch.from_numpy(w.idx[walk["rows"]].copy()).cuda()
        self.y = torch.from_numpy(walk["y"].astype(np.float32)).cuda()
        self.sched = torch.tensor([[sc.GATED_LR, sc.NEG_WEIGHT]] * self.S, dtype=torch.float32, device="cuda")
        self.hist = torch.zeros((self.S, 8), device="cuda")
        self.done = 0
        n_g = sum(k.endswith(".hidden.weight") for k in w.Q)  # gated MLPs
        self.cache_bytes = (n_g - 1) * 4 * (96 * 64 + 128 * 96) * 2  # hbk_mlp_plan.h: wsplit_halves, f16

    def step(self, n):
        def go():
            assert self.plan.step_variant(self.B, "cuda") == (2 if self.variant == "v2" else 1)
            self.tr.train_indexed(self.idx, self.y, self.sched, pool32=self.dev["pool32"], pool16=self.dev["pool16"],
                                  history=self.hist, steps_per_graph=self.spg, n_steps=n, continued=self.done > 0)

        _on_variant_stream(self.dev, self.variant, go)
        self.done += n

    def bits(self):
        """(parameters, m, v, weight-cache planes) as integer copies."""
        tr = self.tr
        return [tr.model.flat_parameters.detach().view(torch.int32).clone(), tr._m.view(torch.int32).clone(),
                tr._v.view(torch.int32).clone(), tr._indexed_ws[:self.cache_bytes].clone()]

    def named(self, flat):
        return {k: v.detach().cpu().numpy().copy() for k, v in self.plan.views(flat).items()}


def _check_hist(h, ref):
    h = h.cpu().numpy().astype(np.float64)
    print("n_sel", h[:, 0], "acc_steps", h[:, 1], "fired", h[:, 2])
    np.testing.assert_array_equal(h[:, [0, 1, 2, 4, 5, 6, 7]], ref[:, [0, 1, 2, 4, 5, 6, 7]])
    np.testing.assert_allclose(h[:, 3], ref[:, 3], rtol=2e-4)


@pytest.mark.parametrize("variant", ["v2", "v1"])
def test_stale_slabs_are_never_consumed(variant, walk6, dev, tmp_path, monkeypatch):
    monkeypatch.delenv("HBK_STEP_GATE_SKIP", raising=False)
    r = Run(dev, variant, walk6, tmp_path, stale=True)
    fired = walk6["hist"][:, 2]
    before = None
    for s in range(r.S):
        if s == 0:  # (the first step fills the weight cache from the parameters: planes compared from step 1)
            before = r.bits()[:3]
        r.step(1)
        after = r.bits()
        if not fired[s]:
            for name, a, b in zip(("params", "m", "v", "weight cache"), after, before):
                assert torch.equal(a, b), f"step {s} (n_sel {walk6['hist'][s, 0]:.0f}, no fire) changed {name}"
        else:
            assert all(bool(torch.isfinite(t.view(torch.float32)).all()) for t in after[:3]), s
            assert bool(torch.isfinite(after[3].view(torch.float16).float()).all()), s
            assert not all(torch.equal(a, b) for a, b in zip(after[:3], before[:3])), s  # (it did step)
        before = after
    _check_hist(r.hist, walk6["hist"])
    params, m = r.named(r.tr.model.flat_parameters), r.named(r.tr._m)
    assert all(np.isfinite(v).all() for v in params.values())
    f = sc.gated_figures(params, m, walk6)
    print(f"share {f['share']:.3e}, drift {f['drift']:.3e}, max |P - P_ref| {f['max']:.3e}")
    assert f["max"] <= 2 * sum(walk6["fired_lr"])
    assert f["share"] <= 4 * GATED_SHARE_F32
    assert f["drift"] <= 4 * GATED_DRIFT_F32
    for k, v in f["m"].items():
        assert v <= 4 * GATED_M_F32[k], f"{k}: max |m - m_ref| = {v:.2e} of max |m_ref| (f32 walk {GATED_M_F32[k]:.1e})"


def test_the_decision_is_read_on_every_replay(walk8, dev, tmp_path, monkeypatch):
    monkeypatch.delenv("HBK_STEP_GATE_SKIP", raising=False)
    r = Run(dev, "v2", walk8, tmp_path, steps_per_graph=2)
    r.step(r.S)  # one eager step, the two-step graph three times, one eager step
    assert sum(k[0] == "indexed" for k in r.tr._graphs) == 1
    _check_hist(r.hist, walk8["hist"])
    assert bool(torch.isfinite(r.tr.model.flat_parameters).all())


def _first_fire_and_rest(dev, variant, walk, tmp_path):
    """-> ({name: (P, m, v) int32 bits} after the first fire (step 2), history, state) of one run."""
    r = Run(dev, variant, walk, tmp_path)
    for _ in range(3):
        r.step(1)
    tr = r.tr
    snap = {k: tuple(d[k].view(np.int32) for d in (r.named(tr.model.flat_parameters), r.named(tr._m), r.named(tr._v)))
            for k in sc.world().Q}
    r.step(r.S - 3)
    return snap, r.hist.clone(), tr._fstate.cpu().numpy().copy()


def _m_figure(a, b):
    worst = 0.0
    for k in a:
        if not _from_slabs(k):
            ma, mb = a[k][1].view(np.float32).astype(np.float64), b[k][1].view(np.float32).astype(np.float64)
            worst = max(worst, float(np.abs(ma - mb).max() / np.abs(ma).max()))
    return worst


@pytest.mark.parametrize("variant", ["v2", "v1"])
def test_skip_on_equals_skip_off(variant, walk6, dev, tmp_path, monkeypatch):
    runs = {}
    for name, knob in (("off_a", "0"), ("off_b", "0"), ("on", "1")):
        monkeypatch.setenv("HBK_STEP_GATE_SKIP", knob)
        runs[name] = _first_fire_and_rest(dev, variant, walk6, tmp_path / name)
    monkeypatch.delenv("HBK_STEP_GATE_SKIP")
    for name in ("off_a", "on"):
        _check_hist(runs[name][1], walk6["hist"])
    np.testing.assert_array_equal(runs["on"][2], runs["off_a"][2])  # both state halves
    n = 0
    for k in sc.world().Q:
        if _from_slabs(k):
            for which, a, b, c in zip("Pmv", runs["on"][0][k], runs["off_a"][0][k], runs["off_b"][0][k]):
                np.testing.assert_array_equal(a, b, err_msg=f"{which} of {k}: skip on against off")
                np.testing.assert_array_equal(b, c, err_msg=f"{which} of {k}: skip off, two runs")
            n += 1
    assert n == 14, n
    parent = _m_figure(runs["off_a"][0], runs["off_b"][0])
    ours = max(_m_figure(runs["on"][0], runs["off_a"][0]), _m_figure(runs["on"][0], runs["off_b"][0]))
    print(f"GATE-SKIP {variant}: atomically summed tensors, max |m_a - m_b| / max |m|: off against off "
          f"{parent:.3e}, on against off {ours:.3e} (recorded off against off {RUN_TO_RUN[variant]})")
    assert RUN_TO_RUN[variant] is not None, "the off-against-off figure has not been recorded"
    assert ours <= 4 * RUN_TO_RUN[variant]


def test_flag_needs_deferred_partials(dev):
    from heybuddy._native import HBKError
    from heybuddy.wakeword import WakeWordMLPModel
    m = WakeWordMLPModel().cuda()
    plan, B = m.plan, 48
    bucket = torch.zeros(plan.n_params + plan.N_STATS, device="cuda")
    y = torch.zeros(B, device="cuda")
    idx = torch.zeros(B, dtype=torch.int32, device="cuda")
    with pytest.raises(HBKError, match=r"status -1: .*HBK_STEP_DEFER_PARTIALS"):  # (-1: HBK_ERR_ARG)
        plan.step_fwd_bwd(m.flat_parameters, bucket, plan.new_state("cuda"), 0, y, B, pool32=dev["pool32"],
                          pool16=dev["pool16"], idx=idx, idx_stride=B, gate_skip=True)
    torch.cuda.synchronize()
    assert not bucket.any()  # refused before any launch
