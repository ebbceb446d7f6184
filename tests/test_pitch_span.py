"""hbk_pitch_shift over each clip's non-silent span (HBK_PS_SPAN, on by default).

The vocoder starts at the first frame group whose source frames can be
non-zero, stops 36 frames after the last one, and the resampler reads zeros
outside the clip's own computed range. 13 listed clips of 23,040 samples, both
fast shifts, paired in workgroups of two as listed below (idx order):

  0 | 1   burst of 3,000 at 9,000          | the burst at 40 (front reflect padding)
  2 | 3   the burst ending at L - 30       | one non-zero sample at 11,520
  4 | 5   100 samples (under one window)   | a burst with an exact-zero gap of 4,000 inside
  6 | 7   all zero                         | a burst at 12,000
  8 | 9   early burst at 500               | late burst at 18,000 (disjoint spans, long union)
 10 | 11  burst + 0.97**k tail to underflow| full length, no zeros
 12       burst alone (odd count: the padding slot repeats it)
and row 9 of the buffer unlisted (comes back untouched). idx is a permutation
of the rows.

Bounds against oracle.augment.pitch_shift (float64) are the project's: per clip
relative L2 <= 1e-4 and max error <= 1e-3 of the oracle's peak.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 23040
SHIFTS = ((128, 125), (125, 128))
UNLISTED = 9
# row of the clip at idx position p (a permutation that skips row UNLISTED)
ROWS = np.array([3, 0, 7, 1, 12, 5, 2, 13, 8, 4, 11, 6, 10], np.int32)
N_ROWS = 14


def _clips():
    rng = np.random.default_rng(20240611)
    t = np.arange(T)

    def burst(n):  # speech-like: noise under a syllable-rate envelope, hard edges
        env = 0.15 + 0.85 * np.sin(np.pi * np.arange(n) / max(n, 1) * 6.0) ** 2
        return 0.3 * rng.standard_normal(n) * env

    c = np.zeros((len(ROWS), T))
    b = burst(3000)
    c[0, 9000:12000] = b
    c[1, 40:3040] = b
    c[2, T - 30 - 3000:T - 30] = b
    c[3, 11520] = 0.4
    c[4, 15000:15100] = burst(100)
    c[5, 6000:16000] = burst(10000)
    c[5, 9000:13000] = 0.0
    # 6: all zero
    c[7, 12000:15000] = burst(3000)
    c[8, 500:3500] = burst(3000)
    c[9, 18000:21000] = burst(3000)
    c[10, 4000:7000] = burst(3000)
    k = np.arange(T - 7000)
    c[10, 7000:] = 0.2 * 0.97 ** k * np.where(k % 2, -1.0, 1.0)  # float32 underflows to 0 near k = 3,400
    c[11] = burst(T)
    c[11][c[11] == 0] = 1e-3
    c[12, 9000:12000] = burst(3000)
    x = np.zeros((N_ROWS, T), np.float32)
    x[ROWS] = c.astype(np.float32)
    x[UNLISTED] = (0.1 * np.sin(2 * np.pi * 300.0 * t / 16000.0)).astype(np.float32)
    assert (x[ROWS[10], 7000 + 3600:] == 0).all() and x[ROWS[10], 7000 + 3000] != 0  # the tail does underflow
    assert (x[ROWS[11]] != 0).all()
    return x


def _run_device(x, num, den):
    import torch
    from heybuddy.kernels import pitch_shift
    xd = torch.from_numpy(x).cuda()
    return pitch_shift(xd, torch.from_numpy(ROWS), num, den, out=xd).cpu().numpy()


if __name__ == "__main__":  # child of test_span_path_against_full_path: python test_pitch_span.py OUT.npz
    for p in (ROOT, os.path.join(ROOT, "hey-buddy_amd")):
        sys.path.insert(0, p)
    x = _clips()
    np.savez(sys.argv[1], **{f"s{num}_{den}": _run_device(x, num, den) for num, den in SHIFTS})
    sys.exit(0)

from oracle import augment as oaug  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clips():
    x = _clips()
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def oracle(clips):
    ref = {s: oaug.pitch_shift(clips[ROWS], *s) for s in SHIFTS}
    for r in ref.values():
        r.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def device(clips):
    return {s: _run_device(clips, *s) for s in SHIFTS}


def _far_from(nz, reach):
    """samples more than `reach` samples from every True of nz"""
    k = np.ones(2 * reach + 1)
    return np.convolve(nz.astype(np.float64), k, mode="same") < 0.5


@pytest.mark.parametrize("shift", SHIFTS, ids=lambda s: f"{s[0]}_{s[1]}")
def test_span_path_matches_oracle(shift, clips, oracle, device):
    """Every clip within the project's bounds; exactly 0.0 at every sample more
    than 512 samples from the nearest non-zero oracle sample (the oracle's
    support is the input's +- 255); a silent clip stays silent; the unlisted
    row is untouched."""
    ref, out = oracle[shift], device[shift]
    for p, row in enumerate(ROWS):
        r, o = ref[p], out[row]
        if not r.any():
            assert not o.any(), f"clip {p}: silent oracle output, non-zero device output"
            continue
        l2 = np.sqrt(((o - r) ** 2).sum()) / np.sqrt((r ** 2).sum())
        mx = np.abs(o - r).max() / np.abs(r).max()
        far = _far_from(r != 0, 512)
        stray = int(np.count_nonzero(o[far]))
        print(f"shift {shift} clip {p}: rel L2 {l2:.2e}, rel max {mx:.2e}, {int(far.sum())} far samples, "
              f"{stray} of them non-zero")
        assert l2 <= 1e-4 and mx <= 1e-3, f"clip {p}: rel L2 {l2:.2e}, rel max {mx:.2e}"
        assert stray == 0, f"clip {p}: {stray} non-zero samples in silence"
    assert not out[ROWS[6]].any()
    np.testing.assert_array_equal(out[UNLISTED], clips[UNLISTED])


def test_span_path_against_full_path(clips, tmp_path):
    """HBK_PS_SPAN=0 against the default, each in a fresh process (which sees
    only its own environment; the switch is read on every call, see
    test_span_switch_is_read_per_call): bit-identical before (the clip's last non-zero input sample
    - 256), |a - b| <= 1e-3 of the clip's peak everywhere else."""
    me = os.path.abspath(__file__)
    env = {k: v for k, v in os.environ.items() if k != "HBK_PS_SPAN"}
    runs = {"span": env, "full": dict(env, HBK_PS_SPAN="0")}
    procs = {k: subprocess.Popen([sys.executable, me, str(tmp_path / f"{k}.npz")], env=e, stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, text=True) for k, e in runs.items()}
    for k, pr in procs.items():
        try:
            log, _ = pr.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            raise
        assert pr.returncode == 0, f"{k}: {log[-3000:]}"
    span, full = np.load(tmp_path / "span.npz"), np.load(tmp_path / "full.npz")
    for num, den in SHIFTS:
        a, b = span[f"s{num}_{den}"], full[f"s{num}_{den}"]
        np.testing.assert_array_equal(a[UNLISTED], b[UNLISTED])
        for p, row in enumerate(ROWS):
            nz = np.flatnonzero(clips[row])
            cut = max(int(nz[-1]) - 256, 0) if nz.size else 0
            same = np.array_equal(a[row, :cut].view(np.int32), b[row, :cut].view(np.int32))
            peak = max(float(np.abs(a[row]).max()), float(np.abs(b[row]).max()))
            d = float(np.abs(a[row].astype(np.float64) - b[row]).max())
            print(f"shift {num}/{den} clip {p}: bits equal before {cut}: {same}; max |a - b| {d:.2e}, peak {peak:.2e}")
            assert same, f"shift {num}/{den} clip {p}: the span path differs from the full path before sample {cut}"
            assert d <= 1e-3 * peak, f"shift {num}/{den} clip {p}: |a - b| {d:.2e} > 1e-3 of peak {peak:.2e}"


def test_span_switch_is_read_per_call(clips):
    """HBK_PS_SPAN toggled between calls of ONE process: five clips (a silent one,
    a full-length one, three placed bursts; the odd count leaves one vocoder
    workgroup with a lone clip), both shifts. The HBK_PS_SPAN=0 call against the
    default call holds what test_span_path_against_full_path accepts across two
    processes; the HBK_PS_SPAN=1 call equals the default call bit for bit."""
    import torch
    from heybuddy.kernels import pitch_shift
    rows = ROWS[[6, 11, 0, 2, 9]]  # silent, full length, bursts at 9,000, at the end, at 18,000
    x = np.ascontiguousarray(clips[rows])
    idx = torch.arange(len(rows), dtype=torch.int32)

    def run(num, den, span):
        if span is None:
            os.environ.pop("HBK_PS_SPAN", None)
        else:
            os.environ["HBK_PS_SPAN"] = span
        xd = torch.from_numpy(x).cuda()
        return pitch_shift(xd, idx, num, den, out=xd).cpu()

    before = os.environ.get("HBK_PS_SPAN")
    try:
        for num, den in SHIFTS:
            default, full, on = run(num, den, None), run(num, den, "0"), run(num, den, "1")
            assert torch.equal(on, default), f"shift {num}/{den}: HBK_PS_SPAN=1 differs from the default call"
            a, b = default.numpy(), full.numpy()
            assert not a[0].any() and not b[0].any()
            for p in range(len(rows)):
                nz = np.flatnonzero(x[p])
                cut = max(int(nz[-1]) - 256, 0) if nz.size else 0
                same = np.array_equal(a[p, :cut].view(np.int32), b[p, :cut].view(np.int32))
                peak = max(float(np.abs(a[p]).max()), float(np.abs(b[p]).max()))
                d = float(np.abs(a[p].astype(np.float64) - b[p]).max())
                print(f"shift {num}/{den} clip {p}: bits equal before {cut}: {same}; max |a - b| {d:.2e}, peak {peak:.2e}")
                assert same, f"shift {num}/{den} clip {p}: the span call differs from the full call before sample {cut}"
                assert d <= 1e-3 * peak, f"shift {num}/{den} clip {p}: |a - b| {d:.2e} > 1e-3 of peak {peak:.2e}"
    finally:
        if before is None:
            os.environ.pop("HBK_PS_SPAN", None)
        else:
            os.environ["HBK_PS_SPAN"] = before


@pytest.mark.parametrize("shift", SHIFTS, ids=lambda s: f"{s[0]}_{s[1]}")
def test_in_place_and_out_of_place_are_identical(shift, clips, device):
    """hbk_pitch_shift through the C ABI with out a separate buffer pre-filled
    with a sentinel: the listed rows carry the in-place call's bits, every
    other row keeps the sentinel (nothing depends on out's previous contents)."""
    import torch
    from heybuddy._native import check, lib, ptr, stream_ptr
    num, den = shift
    xd = torch.from_numpy(np.array(clips)).cuda()
    idx = torch.from_numpy(ROWS).cuda()
    out = torch.full((N_ROWS, T), 12345.0, dtype=torch.float32, device="cuda")
    need = int(lib().hbk_pitch_shift_workspace_size(len(ROWS), T, 16000, num, den))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")  # NaN bits: stale workspace must not be read
    check(lib().hbk_pitch_shift(ptr(xd), xd.stride(0), len(ROWS), ptr(idx), T, 16000, num, den, ptr(out),
                                out.stride(0), ptr(ws), need, stream_ptr(xd.device)), "hbk_pitch_shift")
    o = out.cpu().numpy()
    np.testing.assert_array_equal(xd.cpu().numpy(), clips)  # x is read only
    assert (o[UNLISTED] == 12345.0).all()
    np.testing.assert_array_equal(o[ROWS].view(np.int32), device[shift][ROWS].view(np.int32))
