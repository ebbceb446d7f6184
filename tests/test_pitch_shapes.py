"""hbk_pitch_shift's host side at every ratio and clip length of
tests/pitch_shape_cases.py, on the CPU.

* The geometry csrc/hbk_augment_plan.h computes (tests/augment_plan_check.cpp
  with `L rate num den` arguments, built with AddressSanitizer + UBSan as in
  tests/test_augment_plan.py) equals oracle.augment.pitch_shift_geometry, and
  the loaded library's workspace size equals the header's layout total.
* Rates above 2 (ratios below 1/2), which ps_vocoder_kernel cannot step through
  and torch_pitch_shift never draws, are refused; 1/2 is accepted.
* The argument checks of hbk_pitch_shift that need no device.
* The preconditions of tests/test_pitch_shapes_gpu.py: every listed clip but the
  silent one has a non-silent oracle output, the silent one an all-zero one, and
  the reference's float32 formulation agrees with the float64 oracle.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import pitch_shape_cases as psc
from test_augment_plan import checker  # noqa: F401  (the sanitizer-built tests/augment_plan_check.cpp)

from oracle import augment as oaug

GEOMETRY_FIELDS = ("f_in", "f_out", "l1", "orig", "nw", "width", "target")


def _run(exe, cases):
    args = [str(v) for L, (num, den) in cases for v in (L, psc.SAMPLE_RATE, num, den)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("HBK_")}
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]  # no invariant message, no sanitizer report
    out = json.loads(r.stdout)["pitch"]
    assert [(c["L"], (c["num"], c["den"])) for c in out] == list(cases)
    return out


def test_the_ratios_are_the_accepted_fast_shifts():
    from fractions import Fraction
    fast = oaug.pitch_fast_shifts(psc.SAMPLE_RATE, 12)
    assert len(fast) == 14
    want = sorted(set(fast) - {Fraction(*psc.REFUSED_FAST_SHIFT)})
    assert [Fraction(*r) for r in psc.FAST_SHIFTS] == want
    assert [(f.numerator, f.denominator) for f in want] == list(psc.FAST_SHIFTS)  # in lowest terms
    assert psc.RATIOS == psc.FAST_SHIFTS + ((5, 2),)
    assert all(Fraction(*r) < Fraction(1, 2) for r in psc.RATE_ABOVE_2)


def test_geometry_equals_the_oracle(checker):  # noqa: F811
    from heybuddy._native import lib
    h = lib()
    cases = [(L, r) for r in psc.RATIOS for L in psc.LENGTHS]
    for c in _run(checker, cases):
        L, num, den = c["L"], c["num"], c["den"]
        assert c["rc"] == 0 and c["error"] == "", (L, num, den, c["error"])
        want = oaug.pitch_shift_geometry(L, num, den)
        want["nw"] = want["new"]
        got = c["geometry"]
        assert {k: got[k] for k in GEOMETRY_FIELDS} == {k: want[k] for k in GEOMETRY_FIELDS}, (L, num, den)
        assert got["L"] == L and got["rate"] == want["rate"]
        totals = {k["n"]: k["total"] for k in c["calls"]}
        for n in (1, 3, 65535):
            assert h.hbk_pitch_shift_workspace_size(n, L, psc.SAMPLE_RATE, num, den) == totals[n] > 0, (L, num, den, n)
    # the fast shift the geometry refuses: its resampler's taps
    (c,) = _run(checker, [(23040, psc.REFUSED_FAST_SHIFT)])
    assert c["rc"] == -3 and "(149 taps)" in c["error"]


def test_rates_above_2_are_refused(checker):  # noqa: F811
    """The vocoder advances the source frame by at most two per output frame, and
    torch_pitch_shift.get_fast_shifts keeps ratios in [0.5, 2]."""
    from heybuddy._native import lib
    h = lib()
    cases = [(L, r) for r in psc.RATE_ABOVE_2 for L in (126, 3001, 23040)]
    for c in _run(checker, cases):
        L, num, den = c["L"], c["num"], c["den"]
        assert c["rc"] == -3 and "geometry" not in c, (L, num, den)
        assert f"{num}/{den} has rate {den / num:g} > 2" in c["error"], c["error"]
        assert "at most two source frames per output frame" in c["error"] and "[0.5, 2]" in c["error"]
        for n in (1, 3, 65535):
            assert h.hbk_pitch_shift_workspace_size(n, L, psc.SAMPLE_RATE, num, den) == 0
    for c in _run(checker, [(L, (1, 2)) for L in (126, 3001, 23040)]):  # rate exactly 2.0
        assert c["rc"] == 0 and c["geometry"]["rate"] == 2.0
        assert h.hbk_pitch_shift_workspace_size(1, c["L"], psc.SAMPLE_RATE, 1, 2) > 0


def test_argument_checks_that_need_no_device():
    from heybuddy._native import lib
    h = lib()
    HBK_OK, HBK_ERR_ARG = 0, -1
    # n > 65535 is refused before the pointers are looked at; n = 0 is a call with nothing to do
    rc = h.hbk_pitch_shift(None, 23040, 65536, None, 23040, psc.SAMPLE_RATE, 128, 125, None, 23040, None, 0, None)
    assert rc == HBK_ERR_ARG and "n > 65535" in h.hbk_last_error().decode()
    assert h.hbk_pitch_shift(None, 23040, 0, None, 23040, psc.SAMPLE_RATE, 128, 125, None, 23040, None, 0,
                             None) == HBK_OK


@pytest.mark.parametrize("L", psc.LENGTHS)
def test_oracle_preconditions(L):
    """What the GPU tests rely on, so that they cannot skip their way to green."""
    x, idx = psc.clips(L)
    assert len(idx) % 2 == 1 and sorted(idx.tolist() + [len(idx) // 2]) == list(range(x.shape[0]))
    assert list(idx) != sorted(idx)
    assert (x[idx[0]] != 0).all() and x[idx[2], -1] != 0 and not x[idx[psc.SILENT]].any()
    if L == 9000:
        assert np.flatnonzero(x[idx[5]])[[0, -1]].tolist() == [7600, 8599]
    ratios = [r for r, l in psc.ALL_CASES if l == L]
    assert ratios
    for r in ratios:
        ref, f32 = psc.oracle(r, L), psc.oracle_f32(r, L)
        assert ref.shape == (len(idx), L) and np.isfinite(ref).all()
        for p in range(len(idx)):
            if p == psc.SILENT:
                assert not ref[p].any() and not f32[p].any()
                continue
            assert np.abs(ref[p]).max() > 1e-2, f"{r} clip {p}: silent oracle output"
            l2, mx = psc.errors(f32[p], ref[p])
            print(f"L {L} ratio {r[0]}/{r[1]} clip {p}: float32 formulation rel L2 {l2:.2e}, max {mx:.2e} of peak")
            assert l2 <= 1e-3, f"{r} clip {p}: float32 against float64 rel L2 {l2:.2e}"
