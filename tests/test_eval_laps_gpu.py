"""The lap form of the evaluation pass (kv_gemm_kernel<.., kLap>): a pass that
covers an f16 pool read in order several times over evaluates the laps of a
pool row two at a time. Every row evaluation keeps its values, its
chunk order and its MFMA sequence, so against the plain form (HBK_EVAL_LAPS=0,
read per call) prob is bit-identical and the counts are equal.

Pools of 16, 48, 130 and 257 rows (under one tile of 128 pool rows, one that is
no multiple of 16, two and three tiles with a ragged last one); rows = k laps
for k = 1, 2, 3, 4, 5, 9, and the same + 7; the pass starting at pool row 0, 5
and n_pool - 3 (a lap boundary inside a tile); dropout 0.1 and 0.
hbk_mlp_eval_laps reports which rows of a pass take the lap form. (Four laps per
wave were built and measured slower than the plain form: DESIGN.md section 8.)
"""
import os

import numpy as np
import pytest
import torch

from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

POOLS = (16, 48, 130, 257)
LAPS = (1, 2, 3, 4, 5, 9)


class _Env:
    """HBK_EVAL_LAPS for the calls inside (the library reads it per call)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("HBK_EVAL_LAPS")
        if self.value is None:
            os.environ.pop("HBK_EVAL_LAPS", None)
        else:
            os.environ["HBK_EVAL_LAPS"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("HBK_EVAL_LAPS", None)
        else:
            os.environ["HBK_EVAL_LAPS"] = self.old


@pytest.fixture(scope="module")
def setup():
    from heybuddy.wakeword import WakeWordMLPModel
    params = omlp.init_params(seed=15)
    rng = np.random.default_rng(16)
    host = {n: (rng.standard_normal((n, 16, 96)) - 0.2).astype(np.float16) for n in POOLS}
    # centre the output bias so that the predictions straddle the threshold (non-trivial counts)
    _, z, _ = omlp.forward(params, host[257].astype(np.float32))
    params["mlp_out.output.bias"] = (params["mlp_out.output.bias"] - np.median(z) + 1e-3).astype(np.float32)
    m = WakeWordMLPModel()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m = m.cuda()
    ws = torch.empty(m.plan.eval_workspace_bytes(4096), dtype=torch.uint8, device="cuda")
    m.plan.eval_prepare(m.flat_parameters, ws)
    pools = {n: torch.from_numpy(h).cuda() for n, h in host.items()}
    return params, m, ws, host, pools


def _count(m, ws, pool, rows, laps, p=0.0, seed=0, row_offset=0, idx=None, label=0):
    counts = torch.zeros(4, device="cuda")
    prob = torch.full((rows,), -1.0, device="cuda")
    with _Env(laps):
        m.plan.eval_count(m.flat_parameters, pool, rows, label, counts, ws, idx=idx, row_offset=row_offset,
                          dropout_p=p, seed=seed, prob=prob)
    return counts.cpu().numpy(), prob.cpu().numpy()


def _plan(rows, n_pool):
    two = rows // (2 * n_pool) * 2 * n_pool
    return two, rows - two


@pytest.mark.parametrize("n_pool", POOLS)
def test_lap_form_is_bit_identical_to_the_plain_form(n_pool, setup):
    from heybuddy.kernels import MlpPlan
    _, m, ws, _, pools = setup
    seen = set()
    for k in LAPS:
        for extra in (0, 7):
            rows = n_pool * k + extra
            with _Env(None):
                plan = MlpPlan.eval_laps(rows, n_pool)
            assert plan == _plan(rows, n_pool), (rows, n_pool, plan)
            with _Env("0"):
                assert MlpPlan.eval_laps(rows, n_pool) == (0, rows)
            seen.add((plan[0] > 0, plan[1] > 0))
            for off in (0, 5, n_pool - 3):
                for p in (0.1, 0.0):
                    seed = 0x5EED_0000 + 131 * rows + off
                    c1, p1 = _count(m, ws, pools[n_pool], rows, None, p=p, seed=seed, row_offset=off)
                    c0, p0 = _count(m, ws, pools[n_pool], rows, "0", p=p, seed=seed, row_offset=off)
                    what = f"n_pool {n_pool}, rows {rows}, offset {off}, dropout {p}: launched as {plan}"
                    assert np.array_equal(p1.view(np.int32), p0.view(np.int32)), what
                    assert (p0 >= 0).all(), what  # every row evaluation was written
                    np.testing.assert_array_equal(c1, c0, err_msg=what)
                    np.testing.assert_array_equal(c1, omlp.eval_counts(p1, 0), err_msg=what)
    # the lap form alone, lap sets + a plain remainder, and the plain form alone all ran
    assert seen == {(True, False), (True, True), (False, True)}


def test_lap_form_matches_the_float64_oracle(setup):
    params, m, ws, host, pools = setup
    n, rows, off, seed = 130, 130 * 5 + 7, 5, 0x1234_5678_9ABC
    c, pr = _count(m, ws, pools[n], rows, None, p=0.1, seed=seed, row_offset=off)
    keep = omlp.dropout_keep(seed, off + np.arange(rows), p=0.1)
    x = host[n][(off + np.arange(rows)) % n].astype(np.float32).reshape(rows, -1) * keep / np.float32(0.9)
    ref, _, _ = omlp.forward(params, x.reshape(rows, 16, 96))
    np.testing.assert_allclose(pr, ref, atol=2e-5, rtol=0)
    np.testing.assert_array_equal(c, omlp.eval_counts(pr, 0))
    assert 0 < c[0] < rows


def test_indexed_rows_take_the_plain_form(setup):
    from heybuddy.kernels import MlpPlan
    _, m, ws, _, pools = setup
    n, rows, off, seed = 257, 257 * 4 + 7, 5, 99
    assert MlpPlan.eval_laps(rows, n, True, has_idx=True) == (0, rows)
    assert MlpPlan.eval_laps(rows, n, False) == (0, rows)  # f32 pools stay on the plain form
    idx = torch.from_numpy(((off + np.arange(rows)) % n).astype(np.int32)).cuda()
    ci, pi = _count(m, ws, pools[n], rows, None, p=0.1, seed=seed, row_offset=off, idx=idx)
    cl, pl = _count(m, ws, pools[n], rows, None, p=0.1, seed=seed, row_offset=off)
    assert np.array_equal(pi.view(np.int32), pl.view(np.int32))
    np.testing.assert_array_equal(ci, cl)


def test_multi_launch_of_f16_pools_is_unchanged(setup):
    """hbk_mlp_eval_count_multi has no lap form: its counts equal the separate launches',
    which take the lap form."""
    from heybuddy.kernels import MlpPlan
    _, m, ws, _, pools = setup
    parts = [(pools[130], 130 * 4 + 7, 5, 0, 0, 0x61), (pools[257], 257 * 2, 254, 1, 1, 0x62)]
    assert MlpPlan.eval_laps(parts[0][1], 130) == (520, 7) and MlpPlan.eval_laps(parts[1][1], 257) == (514, 0)
    multi = torch.zeros((2, 4), device="cuda")
    m.plan.eval_count_multi(m.flat_parameters, parts, multi, ws, dropout_p=0.1)
    sep = torch.zeros((2, 4), device="cuda")
    for pool, rows, off, label, which, seed in parts:
        m.plan.eval_count(m.flat_parameters, pool, rows, label, sep[which], ws, row_offset=off, dropout_p=0.1,
                          seed=seed)
    torch.testing.assert_close(multi, sep, rtol=0, atol=0)
    assert 0 < float(multi.sum())


def test_two_contiguous_shares_sum_to_one_pass(setup):
    """A pass split as the data-parallel ranks split it, into two contiguous shares with their
    own row offsets (one dropout stream here, so that the row evaluations are the same)."""
    _, m, ws, _, pools = setup
    n, rows, off, seed = 130, 130 * 9 + 7, 5, 0x77
    c, pr = _count(m, ws, pools[n], rows, None, p=0.1, seed=seed, row_offset=off)
    half = rows // 2
    ca, pa = _count(m, ws, pools[n], half, None, p=0.1, seed=seed, row_offset=off)
    cb, pb = _count(m, ws, pools[n], rows - half, None, p=0.1, seed=seed, row_offset=off + half)
    np.testing.assert_array_equal(ca + cb, c)
    assert np.array_equal(np.concatenate([pa, pb]).view(np.int32), pr.view(np.int32))
