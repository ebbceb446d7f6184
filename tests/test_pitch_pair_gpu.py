"""hbk_pitch_shift with its clips paired by span (the default) against list-order
pairs (HBK_PS_PAIR=0, read per call): the same bits.

A vocoder workgroup runs the union of its two clips' spans; which clip shares
the workgroup, and which workgroup starts first, changes only which frames
outside a clip's own range are computed, and those are never read. Clips of
23,040 samples, in the order they are listed:

  0  burst of 3,000 at 9,000
  1  all zero
  2  signal only at the start (samples 0 .. 2,999)
  3  signal running to the last sample
  4  full length, no zeros
  5  a span within 250 samples of each end (200 .. T - 201)
  6  the burst of clip 0 again (identical spans)
  7+ every fourth: clip 0's burst again; else a burst of random length and place

n = 1, 2, 3, 7 and 64 of them; idx is a permutation of the buffer's rows with
every third row left out, and the rows left out come back untouched.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 23040
SHIFTS = ((128, 125), (125, 128))
COUNTS = (1, 2, 3, 7, 64)


def _case(n):
    rng = np.random.default_rng(977 + n)

    def burst(m):
        env = 0.15 + 0.85 * np.sin(np.pi * np.arange(m) / max(m, 1) * 6.0) ** 2
        return (0.3 * rng.standard_normal(m) * env).astype(np.float32)

    b0 = burst(3000)
    b0[[0, -1]] = 0.25  # the span's ends are non-zero
    c = np.zeros((n, T), np.float32)
    for p in range(n):
        if p == 0 or p == 6 or (p >= 7 and p % 4 == 0):
            c[p, 9000:12000] = b0
        elif p == 1:
            pass
        elif p == 2:
            c[p, :3000] = b0
        elif p == 3:
            c[p, T - 3000:] = b0
        elif p == 4:
            c[p] = burst(T)
            c[p][c[p] == 0] = 1e-3
        elif p == 5:
            c[p, 200:T - 200] = burst(T - 400)
            c[p, [200, T - 201]] = 0.25
        else:
            m = int(rng.integers(500, 12000))
            s = int(rng.integers(0, T - m))
            c[p, s:s + m] = burst(m)
    rows = n + (n + 1) // 2 + 1  # every third row is not listed
    listed = np.array([r for r in range(rows) if r % 3 != 2][:n], np.int32)
    idx = rng.permutation(listed).astype(np.int32)
    x = np.empty((rows, T), np.float32)
    x[:] = (0.1 * np.sin(2 * np.pi * 300.0 * np.arange(T) / 16000.0)).astype(np.float32)
    x[idx] = c
    return x, idx


def _shift(x, idx, num, den, pair):
    import torch
    from heybuddy.kernels import pitch_shift
    old = os.environ.get("HBK_PS_PAIR")
    try:
        if pair:
            os.environ.pop("HBK_PS_PAIR", None)
        else:
            os.environ["HBK_PS_PAIR"] = "0"
        xd = torch.from_numpy(x).cuda()
        out = pitch_shift(xd, torch.from_numpy(idx), num, den, out=xd).cpu().numpy()
    finally:
        if old is None:
            os.environ.pop("HBK_PS_PAIR", None)
        else:
            os.environ["HBK_PS_PAIR"] = old
    return out


@pytest.mark.parametrize("shift", SHIFTS, ids=lambda s: f"{s[0]}_{s[1]}")
@pytest.mark.parametrize("n", COUNTS)
def test_paired_by_span_is_bit_identical_to_list_order(n, shift):
    x, idx = _case(n)
    a = _shift(x, idx, *shift, pair=True)
    b = _shift(x, idx, *shift, pair=False)
    unlisted = np.setdiff1d(np.arange(x.shape[0]), idx)
    assert unlisted.size > 0
    np.testing.assert_array_equal(a[unlisted].view(np.int32), x[unlisted].view(np.int32))
    np.testing.assert_array_equal(b[unlisted].view(np.int32), x[unlisted].view(np.int32))
    for p, row in enumerate(idx):
        assert np.array_equal(a[row].view(np.int32), b[row].view(np.int32)), f"clip {p} (row {row}) differs"
    if n > 1:
        assert not a[idx[1]].any()  # the silent clip stays silent
    assert np.abs(a[idx[0]]).max() > 0.05  # and the shifted clips are not


@pytest.mark.parametrize("shift", SHIFTS, ids=lambda s: f"{s[0]}_{s[1]}")
def test_pairing_reads_no_stale_workspace(shift):
    """Through the C ABI with a workspace of NaN bits and out a separate buffer
    holding a sentinel: the listed rows carry the in-place call's bits, every
    other row keeps the sentinel."""
    import torch
    from heybuddy._native import check, lib, ptr, stream_ptr
    num, den = shift
    x, idx = _case(7)
    ref = _shift(x, idx, num, den, pair=True)
    assert os.environ.get("HBK_PS_PAIR", "1") != "0"
    xd = torch.from_numpy(x).cuda()
    idxd = torch.from_numpy(idx).cuda()
    out = torch.full(x.shape, 12345.0, dtype=torch.float32, device="cuda")
    need = int(lib().hbk_pitch_shift_workspace_size(len(idx), T, 16000, num, den))
    for fill in (0xFF, 0x00):
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        check(lib().hbk_pitch_shift(ptr(xd), xd.stride(0), len(idx), ptr(idxd), T, 16000, num, den, ptr(out),
                                    out.stride(0), ptr(ws), need, stream_ptr(xd.device)), "hbk_pitch_shift")
        o = out.cpu().numpy()
        unlisted = np.setdiff1d(np.arange(x.shape[0]), idx)
        assert (o[unlisted] == 12345.0).all()
        np.testing.assert_array_equal(o[idx].view(np.int32), ref[idx].view(np.int32))
