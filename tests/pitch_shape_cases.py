"""The ratios, clip lengths and clips of tests/test_pitch_shapes.py (CPU) and
tests/test_pitch_shapes_gpu.py: everything hbk_pitch_shift accepts beyond the
two product ratios at 23,040 samples. Data and the float64 oracle's answers,
computed once per (ratio, length) and shared read-only: no device, no library.
"""
import functools

import numpy as np

SAMPLE_RATE = 16000

# torch_pitch_shift's fast shifts within an octave at 16 kHz that pitch_geometry accepts
# (oracle.augment.pitch_fast_shifts(16000, 12) minus 125/64, whose resampler needs 149 > 144 taps), as
# (num, den), rate = den / num:
#   1/2      rate 2.0: a double step on every frame; 2 phases
#   64/125   rate 1.95: 125 phases, target about L / 2
#   5/8, 16/25, 25/32, 4/5   rates 1.6 .. 1.25: double steps in most groups (never FULL); 8, 25, 64, 5 phases
#   125/128, 128/125   the product's two ratios: 128 / 125 phases
#   5/4, 32/25, 25/16, 8/5   rates 0.8 .. 0.625: repeats in every group; 4, 25, 16, 5 phases
#   2/1      rate 0.5: a repeat on every other frame; 1 phase, l1 = 2 L
FAST_SHIFTS = ((1, 2), (64, 125), (5, 8), (16, 25), (25, 32), (4, 5), (125, 128), (128, 125), (5, 4), (32, 25),
               (25, 16), (8, 5), (2, 1))
REFUSED_FAST_SHIFT = (125, 64)
# 5/2 (rate 0.4: a source frame repeated two or three times, l1 about 2.5 L) stands for the ratios above 2, which
# torch_pitch_shift never draws and the geometry accepts
RATIOS = FAST_SHIFTS + ((5, 2),)
PRODUCT = ((128, 125), (125, 128))
# rate above 2: the vocoder would need more than two source frames per output frame; refused
RATE_ABOVE_2 = ((2, 5), (1, 3), (1, 4), (8, 25), (1, 7))

LENGTHS = (
    126,    # the shortest accepted; f_in = 19 < the 64 d rows held in LDS
    250,    # n_fft: every sample lies within the reflect padding's reach, no span can be skipped
    251,    # n_fft + 1
    455,    # 7 * 65: f_in = 66, the first d-row refill; a multiple of 7 and odd
    3001,   # a multiple of neither 4 nor 7; spans can be skipped at both ends
    9000,   # f_in = 1286: crosses the sliding DFT's 1,024-frame restart
    23040,  # the product's clip length
)

SILENT = 4  # the list position of the all-zero clip


def ratio_id(r):
    return f"{r[0]}_{r[1]}"


@functools.lru_cache(maxsize=None)
def clips(L):
    """(x [rows, L] float32, idx int32): the listed clips, by list position,
      0  full length, no zeros
      1  a burst in the middle third
      2  a burst over the last two thirds, to the last sample (a shorter one that only the reflect padding's
         frames hold comes out as exact silence at rate 2 and L = 126)
      3  two tones (440 Hz and 3,100 Hz), full length
      4  all zero
    and for L >= 9000 two late bursts with nearly the same span, [L - 1400, L - 400) and [L - 1300, L - 500)
    (at 9,000: 7,600 .. 8,600), which the span pairing puts into one workgroup: its first frame group lies
    beyond source frame 1,024, so the skipped restart anchors are replayed. One further row of the buffer is
    not listed. idx is a permutation of the listed rows; the count is odd, so one vocoder workgroup holds a
    lone clip."""
    rng = np.random.default_rng(1000003 + L)
    t = np.arange(L)

    def burst(n):  # speech-like: noise under a syllable-rate envelope, hard edges (tests/test_pitch_span.py)
        env = 0.15 + 0.85 * np.sin(np.pi * np.arange(n) / max(n, 1) * 6.0) ** 2
        return 0.3 * rng.standard_normal(n) * env

    third = L // 3
    c = [np.zeros(L) for _ in range(5)]
    c[0] = burst(L)
    c[1][third:2 * third] = burst(third)
    c[2][third:] = burst(L - third)
    c[3] = 0.2 * np.sin(2 * np.pi * 440.0 * t / SAMPLE_RATE) + 0.1 * np.sin(2 * np.pi * 3100.0 * t / SAMPLE_RATE + 0.5)
    if L == 9000:
        for a, b in ((L - 1400, L - 400), (L - 1300, L - 500)):
            late = np.zeros(L)
            late[a:b] = burst(b - a)
            c.append(late)
    c = np.stack(c).astype(np.float32)
    c[0][c[0] == 0] = 1e-3
    c[2, -1] = 0.25
    n = len(c)
    assert n % 2 == 1 and (c[0] != 0).all() and not c[SILENT].any()
    unlisted = n // 2
    listed = np.array([r for r in range(n + 1) if r != unlisted], np.int32)
    idx = rng.permutation(listed).astype(np.int32)
    x = np.empty((n + 1, L), np.float32)
    x[unlisted] = (0.1 * np.sin(2 * np.pi * 300.0 * t / SAMPLE_RATE) + 0.05).astype(np.float32)
    x[idx] = c
    x.setflags(write=False)
    idx.setflags(write=False)
    return x, idx


@functools.lru_cache(maxsize=None)
def oracle(ratio, L):
    """oracle.augment.pitch_shift (float64) of the listed clips of clips(L), by list position."""
    from oracle import augment as oaug
    x, idx = clips(L)
    ref = oaug.pitch_shift(x[idx], *ratio)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def oracle_f32(ratio, L):
    """oracle.augment.pitch_shift_torch (the reference's float32 formulation) of the same clips."""
    from oracle import augment as oaug
    x, idx = clips(L)
    ref = oaug.pitch_shift_torch(x[idx], *ratio)
    ref.setflags(write=False)
    return ref


def errors(got, ref):
    """(relative L2, max error / the reference's peak) of one clip"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return (float(np.sqrt(((got - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum())),
            float(np.abs(got - ref).max() / np.abs(ref).max()))


# the (ratio, length) pairs of test_pitch_shapes_gpu.py's tests
RATIO_CASES = [(r, L) for r in RATIOS for L in (3001, 23040)] + \
              [(r, L) for r in PRODUCT + ((1, 2), (2, 1)) for L in LENGTHS if L not in (3001, 23040)]
# the ratios with 1, 2, 5, 25, 125 and 128 resampler phases
VALU_CASES = [(r, L) for r in ((2, 1), (1, 2), (8, 5), (16, 25), (64, 125), (125, 128)) for L in (455, 3001)] + \
             [(r, 23040) for r in PRODUCT]
KNOB_CASES = [(r, L) for r in ((128, 125), (1, 2), (2, 1)) for L in (251, 455, 9000)]
ALL_CASES = sorted(set(RATIO_CASES + VALU_CASES + KNOB_CASES + [(r, 126) for r in PRODUCT]))
