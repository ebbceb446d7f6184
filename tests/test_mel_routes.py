"""Mel kernel routes: the cases, the checker and a proof that it is sharp (CPU).

``hbk_mel_plan_create`` picks one of four kernels from the window, the
filterbank and the environment (include/hbk.h, hbk_mel_plan_info).
tests/test_mel_routes_gpu.py runs every route against ``oracle.mel.mel_frames``
in fp64; this file holds what that comparison is made of, and checks it
without a GPU:

- the windows W0-W2, the filterbanks B0-B5 and the 2-mel bank, the input
  clips, the bound of each case and the checker;
- ``route_on_host``: the routing rules of hbk_mel_plan_create restated, and
  what each bank must route to;
- ``mel_frames_f32``: the operation restated in f32 (window multiply, FFT,
  power, filter sums and log10 all in f32). Unfaulted it meets every case's
  bound, so the bounds are attainable in f32; with any one of FAULTS injected
  it fails the checker, so the comparison would notice that kernel fault.

Bounds (none is new): bank B0 on the speech-like clips takes the flat 1e-4 of
tests/test_mel.py, every other case ``oracle.mel.fp32_noise_tolerance`` per
bin. Both are in units of the default output scale (out_div 10) and scale by
10 / out_div. A bin that the oracle puts on the log floor is held to the
bound of a bin AT the floor (mel power max(P, log_floor)): fp32 noise can
lift it no further than that.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import mel as omel

N_CLIPS, CLIP_LEN, N_FRAMES = 13, 23040, 141   # 1,833 frames: ragged for 16-, 24-, 32- and 64-frame groups
HBK_ERR_ARG, HBK_ERR_UNSUPPORTED = -1, -3
SLACK_BOUND, SLACK_SHARE = 2e-4, 0.10


# ------------------------------------------------------------- windows ----

@functools.lru_cache(maxsize=None)
def window(name: str) -> np.ndarray:
    if name == "W0":   # H0: Hann 400 centred in 512, zero on its first and last 56 samples
        w = omel.hann_window()
    elif name == "W1":  # full-length periodic Hann: zero at sample 0 only
        w = omel.hann_window(512, 512)
    elif name == "W2":  # Hamming: nowhere zero, every sample of a frame counts
        w = (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(512) / 512.0)).astype(np.float32)
    else:
        raise KeyError(name)
    w.setflags(write=False)
    return w


def window_edge0(w: np.ndarray) -> bool:
    return bool(np.all(w[:32] == 0) and np.all(w[-32:] == 0))


# --------------------------------------------------------- filterbanks ----

def _runs_bank(runs, seed: int) -> np.ndarray:
    """[257, len(runs)] f32: uniform(0.1, 1) weights on bins [lo, hi] of each
    run, zero elsewhere; a run of None is an all-zero column."""
    rng = np.random.default_rng(seed)
    fb = np.zeros((257, len(runs)), dtype=np.float32)
    for m, r in enumerate(runs):
        if r is not None:
            lo, hi = r
            fb[lo:hi + 1, m] = rng.uniform(0.1, 1.0, hi - lo + 1).astype(np.float32)
    return fb


def linear_bank(n_mels: int) -> np.ndarray:
    """Triangular filters with centres linear in Hz over 0-8000, [257, n_mels] f32."""
    freqs = np.linspace(0.0, 8000.0, 257)
    pts = np.linspace(0.0, 8000.0, n_mels + 2)
    d = pts[1] - pts[0]
    down = (freqs[:, None] - pts[None, :-2]) / d
    up = (pts[None, 2:] - freqs[:, None]) / d
    return np.maximum(0.0, np.minimum(down, up)).astype(np.float32)


B3_ZERO_COLUMN = 5
_B3_RUNS = [
    (0, 15), (241, 256),      # DC and Nyquist weights non-zero; also the 2-mel bank
    (256, 256), (0, 0),       # one tap each: the read window is clamped to [241, 256] / starts at 0
    (127, 128), None,
    # 1 to 16 taps, odd and even starts, over the whole spectrum
    (7, 7), (10, 11), (33, 35), (60, 63), (81, 85), (100, 105), (129, 135), (150, 157),
    (171, 179), (200, 209), (15, 25), (46, 57), (91, 103), (120, 133), (141, 155), (222, 237),
    (240, 255), (255, 256), (1, 16), (64, 64), (113, 128), (250, 256), (2, 3), (187, 199),
]
_B4_RUNS = (
    # mels 0-15: at most 8 taps from the even start bin
    [(0, 7), (3, 8), (8, 15), (11, 16), (16, 16), (21, 25), (30, 37), (41, 44),
     (52, 59), (65, 70), (76, 83), (89, 89), (96, 103), (107, 112), (118, 125),
     (122, 127)]              # mel 15: 8-tap window from 122 clamped to 120
    # mels 16-31: at most 16 taps from the even start bin; not in frequency order
    + [(100, 115), (5, 19), (32, 47), (57, 70), (64, 64), (13, 27), (80, 95), (111, 125),
       (2, 17), (45, 59), (90, 104), (71, 84), (24, 39), (112, 127), (50, 65),
       (120, 127)])           # mel 31: 16-tap window from 120 clamped to 112
B5_MOVED = 3                  # B5: this narrow filter on [5, 12], 8 taps from an odd start


@functools.lru_cache(maxsize=None)
def bank(name: str) -> np.ndarray:
    if name == "B0":    # H0: 32 HTK mels over 60-3800 Hz
        fb = omel.mel_fbank()
    elif name == "B1":  # 30 mels: v1 with the last lane's store guarded off
        fb = omel.mel_fbank(n_mels=30, f_max=4000.0)
    elif name == "B2":  # 32 triangles linear in Hz over 0-8000
        fb = linear_bank(32)
    elif name == "B3":
        fb = _runs_bank(_B3_RUNS, seed=3)
    elif name == "B4":
        fb = _runs_bank(_B4_RUNS, seed=4)
    elif name == "B5":
        fb = bank("B4").copy()
        fb[:, B5_MOVED] = 0.0
        fb[5:13, B5_MOVED] = np.random.default_rng(5).uniform(0.1, 1.0, 8).astype(np.float32)
    elif name == "M2":  # n_mels = 2: the first two columns of B3
        fb = np.ascontiguousarray(bank("B3")[:, :2])
    else:
        raise KeyError(name)
    fb.setflags(write=False)
    return fb


BANKS = ("B0", "B1", "B2", "B3", "B4", "B5", "M2")
WINDOWS = ("W0", "W1", "W2")


def route_on_host(fbank: np.ndarray, env=None) -> dict:
    """hbk_mel_plan_create's routing, restated: the kernel of variant 0 and what
    hbk_mel_plan_info reports beside it. ``env``: the HBK_MEL_* variables set."""
    env = env or {}
    n_freq, n_mels = fbank.shape
    if n_mels <= 0 or n_mels > 32 or n_mels % 2:
        return {"error": HBK_ERR_ARG}
    lo, hi = [], []
    for m in range(n_mels):
        k = np.nonzero(fbank[:, m])[0]
        lo.append(int(k[0]) if k.size else 0)
        hi.append(int(k[-1]) if k.size else 0)
    taps = max(h - l + 1 for l, h in zip(lo, hi))
    if taps > 16:
        return {"error": HBK_ERR_UNSUPPORTED}
    v2 = n_mels == 32 and max(hi) < 128 and "HBK_MEL_V1" not in env
    if v2:  # the even-start fit: 8 taps for mels 0-15, 16 for mels 16-31
        v2 = all(hi[m] - (lo[m] & ~1) + 1 <= (8 if m < 16 else 16) for m in range(32))
    kmax = max(min(l, n_freq - taps) + taps - 1 for l in lo)
    kernel = 1
    if v2:
        v4 = int(env.get("HBK_MEL_V4", "0"))
        kernel = 2 if v4 == 0 else 8 if v4 == 8 else 4
    return {"kernel": kernel, "taps": taps, "nk2": min(16, (min(kmax, 255) + 16) // 16),
            "need256": int(kmax >= 256), "n_mels": n_mels}


# --------------------------------------------------------------- clips ----

@functools.lru_cache(maxsize=None)
def clips(kind: str) -> np.ndarray:
    """[13, 23040] f32. "speech": the clips of tests/test_mel.py. "wide": those
    at half amplitude + 0.1 N(0, 1) + a DC and a Nyquist component, so that the
    1-tap DC and Nyquist filters are not far below the frame energy."""
    from heybuddy.synthetic import synthetic_clips
    x = synthetic_clips(N_CLIPS, length=CLIP_LEN, seed=7).numpy()
    if kind == "wide":
        rng = np.random.default_rng(11)
        alt = np.where(np.arange(CLIP_LEN) % 2 == 0, 1.0, -1.0)
        x = (0.5 * x + 0.1 * rng.standard_normal(x.shape) + 0.03 + 0.03 * alt).astype(np.float32)
    elif kind != "speech":
        raise KeyError(kind)
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def clips_for(bank_name: str) -> str:
    """B0 runs on the speech-like clips, where the flat bound holds. The other banks have
    filters (DC, Nyquist, 1-tap, above 4 kHz) that those clips leave far below the frame
    energy, where the model bound is slack (B4: 21 % of live bins above 2e-4): they run
    on the wideband clips."""
    return "speech" if bank_name == "B0" else "wide"


# ------------------------------------------------- reference and bound ----

DEFAULTS = dict(hop=160, in_scale=32767.0, log_floor=1e-10, out_div=10.0, out_add=2.0)


def reference(pcm, n_frames, win, fb, flat: bool, **kw):
    """(fp64-oracle output, per-bin bound, mel power) for one call."""
    p = dict(DEFAULTS, **kw)
    ref, mel_pow, energy = omel.mel_frames(pcm, n_frames, in_scale=p["in_scale"], window=win, fbank=fb,
                                           hop=p["hop"], log_floor=p["log_floor"], out_div=p["out_div"],
                                           out_add=p["out_add"])
    if flat:
        tol = np.full(ref.shape, 1e-4)
    else:
        tol = omel.fp32_noise_tolerance(np.maximum(mel_pow, p["log_floor"]), energy)
    return ref, tol * abs(10.0 / p["out_div"]), mel_pow


@functools.lru_cache(maxsize=None)
def case_reference(bank_name: str, window_name: str):
    """The 13 x 141 frames of a (bank, window) case at the default scaling,
    computed once and shared (read-only)."""
    out = reference(clips(clips_for(bank_name)), N_FRAMES, window(window_name), bank(bank_name),
                    flat=bank_name == "B0")
    for a in out:
        a.setflags(write=False)
    return out


def slack_share(tol, mel_pow, log_floor=1e-10, out_div=10.0) -> float:
    """Share of live bins (above the log floor) whose bound exceeds 2e-4."""
    live = mel_pow > log_floor
    return float(((tol > SLACK_BOUND * abs(10.0 / out_div)) & live).sum() / max(1, live.sum()))


def assert_bound_is_sharp(tol, mel_pow, **kw):
    """A condition on the inputs, checked before any kernel runs: a case whose
    bound has gone slack must fail, not pass vacuously."""
    share = slack_share(tol, mel_pow, **kw)
    assert share <= SLACK_SHARE, f"{share:.1%} of live bins have a bound above {SLACK_BOUND}"


def mel_mismatch(out, ref, tol):
    """None if every bin of ``out`` is within ``tol`` of ``ref`` (NaN only where
    the reference is NaN), else a description of the worst bin."""
    out, ref = np.asarray(out), np.asarray(ref)
    if out.shape != ref.shape:
        return f"shape {out.shape} != {ref.shape}"
    rnan = np.isnan(ref)
    onan = np.isnan(out)
    if (rnan != onan).any():
        i = tuple(int(v) for v in np.argwhere(rnan != onan)[0])
        return f"{int((rnan != onan).sum())} bins NaN on one side only, first at {i}: {out[i]} vs {ref[i]}"
    with np.errstate(invalid="ignore"):
        err = np.where(rnan, 0.0, np.abs(out.astype(np.float64) - ref))
    over = err > tol
    if not over.any():
        return None
    i = tuple(int(v) for v in np.unravel_index(np.argmax(err / tol), err.shape))
    return (f"{int(over.sum())} of {err.size} bins over the bound; worst at (clip, frame, mel) {i}: "
            f"{out[i]!r} vs {ref[i]!r}, |d| {err[i]:.3e} > {tol[i]:.3e}")


def worst_ratio(out, ref, tol):
    """(max |d|, max |d| / bound) over the finite bins: what the summary reports."""
    with np.errstate(invalid="ignore"):
        err = np.where(np.isnan(ref), 0.0, np.abs(np.asarray(out, dtype=np.float64) - ref))
    return float(err.max()), float((err / tol).max())


# ------------------------------------------- scaling and geometry cases ----

GEOMETRY = ("hop2", "hop640", "row_stride", "raw_db", "log_floor", "log_floor_mixed", "amp1", "amp1e-3", "amp1e-6")


def geometry_case(name: str, kind: str):
    """(pcm [B, T], n_frames, plan keywords) of one scaling / geometry case on
    the ``kind`` clips. "row_stride" is the default call: the GPU test runs it
    from a [13, 24000] buffer."""
    x = clips(kind)
    if name == "hop2":  # 300 frames two samples apart
        return np.ascontiguousarray(x[:3, 8000:8000 + 2 * 299 + 512]), 300, dict(hop=2)
    if name == "hop640":  # hop > n_fft: the samples between two frames are never read (NaN proves it)
        n = (CLIP_LEN - 512) // 640 + 1
        y = np.full_like(x, np.nan)
        for f in range(n):
            y[:, 640 * f:640 * f + 512] = x[:, 640 * f:640 * f + 512]
        return y, n, dict(hop=640)
    if name == "row_stride":
        return x, N_FRAMES, {}
    if name == "raw_db":
        return x, N_FRAMES, dict(in_scale=1.0, out_div=1.0, out_add=0.0)
    if name == "log_floor":  # nearly every bin on the floor (B0 98.7 %, B2 99.99 %)
        return x * np.float32(1e-3), N_FRAMES, dict(in_scale=1.0, log_floor=1e-3)
    if name == "log_floor_mixed":  # 10x the amplitude: bins on both sides of the clamp (B0 90 %, B2 14 % floored)
        return x * np.float32(1e-2), N_FRAMES, dict(in_scale=1.0, log_floor=1e-3)
    if name.startswith("amp"):
        return x * np.float32(float(name[3:])), N_FRAMES, {}
    raise KeyError(name)


# ------------------------------------------------- the f32 restatement ----

FAULTS = ("tap_dropped", "window_shifted", "nyquist_omitted", "dc_doubled", "edge_rows_skipped",
          "out_div_multiplies", "last_frame_from_next_clip")


def mel_frames_f32(pcm, n_frames, win, fb, hop=160, in_scale=32767.0, log_floor=1e-10, out_div=10.0,
                   out_add=2.0, fault=None, fault_mel=0):
    """hbk_mel_frames in f32 throughout, on the CPU; ``fault`` injects one of
    FAULTS (``fault_mel``: the filter that loses its heaviest tap)."""
    import scipy.fft
    f32 = np.float32
    pcm = np.asarray(pcm, dtype=f32)
    win = np.asarray(win, dtype=f32) * f32(in_scale)   # in_scale folded into the window, as the plan does
    fb = np.array(fb, dtype=f32)
    if fault == "tap_dropped":
        fb[np.argmax(fb[:, fault_mel]), fault_mel] = 0.0
    if fault == "window_shifted":
        win = np.roll(win, 1)
    if fault == "edge_rows_skipped":
        win = win.copy()
        win[:32] = 0.0
    idx = np.arange(n_frames)[:, None] * hop + np.arange(512)[None, :]
    frames = pcm[:, idx]
    if fault == "last_frame_from_next_clip":  # the flat frame index split wrongly (the last clip's "next" wraps)
        frames = frames.copy()
        frames[-1, -1] = frames[0, 0]
    spec = scipy.fft.rfft(frames * win, axis=-1)
    assert spec.dtype == np.complex64
    power = spec.real * spec.real + spec.imag * spec.imag
    if fault == "nyquist_omitted":
        power[..., 256] = 0.0
    if fault == "dc_doubled":
        power[..., 0] *= f32(2.0)
    mel = power @ fb
    assert mel.dtype == f32
    db = f32(10.0) * np.log10(np.maximum(mel, f32(log_floor)))
    out = db * f32(out_div) if fault == "out_div_multiplies" else db / f32(out_div)
    return (out + f32(out_add)).astype(f32)


# --------------------------------------------------------------- tests ----

EXPECTED_ROUTE = {  # bank -> (kernel of variant 0 with no HBK_MEL_* set, taps, nk2, need256)
    "B0": (2, 15, 8, 0),
    "B1": (1, 16, 8, 0),
    "B2": (1, 16, 16, 1),
    "B3": (1, 16, 16, 1),
    "B4": (2, 16, 9, 0),
    "B5": (1, 16, 9, 0),
    "M2": (1, 16, 16, 1),
}


@pytest.mark.parametrize("name", BANKS)
def test_bank_routes_on_host(name):
    r = route_on_host(bank(name))
    assert (r["kernel"], r["taps"], r["nk2"], r["need256"]) == EXPECTED_ROUTE[name]
    assert r["n_mels"] == bank(name).shape[1]
    if r["kernel"] == 2:
        assert route_on_host(bank(name), env={"HBK_MEL_V1": "1"})["kernel"] == 1
        assert route_on_host(bank(name), env={"HBK_MEL_V4": "1"})["kernel"] == 4
        assert route_on_host(bank(name), env={"HBK_MEL_V4": "8"})["kernel"] == 8


def test_banks_are_what_the_cases_need():
    assert [window_edge0(window(w)) for w in WINDOWS] == [True, False, False]
    assert np.count_nonzero(window("W1") == 0) == 1 and window("W1")[0] == 0
    assert np.all(window("W2") > 0)
    b1, b2, b3, b4, b5 = (bank(n) for n in ("B1", "B2", "B3", "B4", "B5"))
    assert b1.shape == (257, 30) and b3.shape == (257, 30) and bank("M2").shape == (257, 2)
    k = np.nonzero(b2.sum(axis=1))[0]
    assert b2.shape == (257, 32) and k.max() == 255 and np.nonzero(b2[:, 31])[0].min() == 241
    assert b3[0, 0] > 0 and b3[256, 1] > 0 and b3[256, 2] > 0 and b3[0, 3] > 0
    assert not b3[:, B3_ZERO_COLUMN].any()
    widths = sorted({r[1] - r[0] + 1 for r in _B3_RUNS if r})
    assert widths == list(range(1, 17))
    assert {r[0] % 2 for r in _B3_RUNS if r} == {0, 1}
    # B4: the clamps of the v2 filter layout (l = 128 - T) are hit by mels 15 and 31
    for m, T in ((15, 8), (31, 16)):
        k = np.nonzero(b4[:, m])[0]
        assert (k.min() & ~1) + T > 128 and k.max() == 127
    assert b4[0, 0] > 0 and np.nonzero(b4.sum(axis=1))[0].max() == 127
    k = np.nonzero(b5[:, B5_MOVED])[0]
    assert (k.min(), k.max()) == (5, 12) and np.array_equal(np.delete(b4, B5_MOVED, 1), np.delete(b5, B5_MOVED, 1))
    # the linear bank with 2 mels is far wider than 16 taps: n_mels = 2 is covered by M2 instead
    assert route_on_host(linear_bank(2))["error"] == HBK_ERR_UNSUPPORTED
    assert route_on_host(np.ascontiguousarray(b3[:, :3]))["error"] == HBK_ERR_ARG


def test_plan_create_refusals():
    """Refused before any device work: the status, a NULL plan and a message."""
    from heybuddy import _native
    lib = _native.lib()
    win = np.ascontiguousarray(window("W0"))
    wide = np.zeros((257, 32), dtype=np.float32)
    wide[40:57, 7] = 1.0  # 17 taps
    wp = win.ctypes.data

    def create(fb, n_mels, hop=160, out_div=10.0):
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        h = ctypes.c_void_p(0xdead)
        rc = lib.hbk_mel_plan_create(wp, fb.ctypes.data, 512, hop, n_mels, 32767.0, 1e-10, out_div, 2.0,
                                     ctypes.byref(h))
        return rc, h.value, lib.hbk_last_error()

    b0 = bank("B0")
    for rc_want, args in ((HBK_ERR_ARG, (np.zeros((257, 31), np.float32), 31)),
                          (HBK_ERR_ARG, (np.zeros((257, 34), np.float32), 34)),
                          (HBK_ERR_ARG, (b0, 32, 0)),
                          (HBK_ERR_ARG, (b0, 32, 160, 0.0)),
                          (HBK_ERR_UNSUPPORTED, (wide, 32))):
        rc, handle, msg = create(*args)
        assert rc == rc_want and handle is None and msg, (rc, handle, msg, args[1:])
    assert route_on_host(wide)["error"] == HBK_ERR_UNSUPPORTED
    info = (ctypes.c_int32 * 8)()
    assert lib.hbk_mel_plan_info(None, info) == HBK_ERR_ARG and lib.hbk_last_error()


@pytest.mark.parametrize("window_name", WINDOWS)
@pytest.mark.parametrize("bank_name", BANKS)
def test_f32_restatement_meets_every_bound(bank_name, window_name):
    ref, tol, mel_pow = case_reference(bank_name, window_name)
    assert_bound_is_sharp(tol, mel_pow)
    out = mel_frames_f32(clips(clips_for(bank_name)), N_FRAMES, window(window_name), bank(bank_name))
    bad = mel_mismatch(out, ref, tol)
    assert bad is None, bad
    if bank_name == "B3":  # the all-zero filter sits on the floor value exactly
        assert np.abs(out[..., B3_ZERO_COLUMN] - (10 * np.log10(1e-10) / 10 + 2)).max() <= 1e-6


@pytest.mark.parametrize("geom", GEOMETRY)
@pytest.mark.parametrize("bank_name", ["B0", "B2"])
def test_f32_restatement_meets_the_geometry_bounds(bank_name, geom):
    pcm, n_frames, kw = geometry_case(geom, clips_for(bank_name))
    win, fb = window("W2"), bank(bank_name)
    ref, tol, mel_pow = reference(pcm, n_frames, win, fb, flat=bank_name == "B0", **kw)
    p = dict(DEFAULTS, **kw)
    assert np.isfinite(ref).all()
    assert_bound_is_sharp(tol, mel_pow, log_floor=p["log_floor"], out_div=p["out_div"])
    floored = (mel_pow < p["log_floor"]).mean()
    if geom == "log_floor":
        assert 0.95 < floored < 1.0, floored
    elif geom == "log_floor_mixed":
        assert 0.05 < floored < 0.95, floored
    else:
        assert floored == 0.0
    bad = mel_mismatch(mel_frames_f32(pcm, n_frames, win, fb, **kw), ref, tol)
    assert bad is None, bad


# fault -> the (bank, window, filter that loses a tap) cases that target it
FAULT_CASES = {
    "tap_dropped": [("B0", "W0", 31), ("B3", "W2", 3), ("B3", "W0", 23), ("B4", "W1", 15), ("B2", "W2", 0)],
    "window_shifted": [("B0", "W0", 0), ("B0", "W1", 0), ("B2", "W2", 0)],
    "nyquist_omitted": [("B3", "W2", 0), ("M2", "W0", 0)],
    "dc_doubled": [("B3", "W2", 0), ("B4", "W0", 0), ("M2", "W2", 0)],
    "edge_rows_skipped": [("B0", "W2", 0), ("B2", "W2", 0), ("B4", "W2", 0)],
    "out_div_multiplies": [("B0", "W0", 0), ("B1", "W2", 0)],
    "last_frame_from_next_clip": [("B0", "W1", 0), ("B3", "W0", 0)],
}


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_reports_each_injected_fault(fault):
    for bank_name, window_name, mel in FAULT_CASES[fault]:
        ref, tol, _ = case_reference(bank_name, window_name)
        out = mel_frames_f32(clips(clips_for(bank_name)), N_FRAMES, window(window_name), bank(bank_name),
                             fault=fault, fault_mel=mel)
        assert mel_mismatch(out, ref, tol) is not None, \
            f"fault {fault} passed the checker on ({bank_name}, {window_name})"


def test_checker_flags_nan_and_shape():
    ref = np.zeros((2, 3, 4))
    tol = np.full(ref.shape, 1e-4)
    assert mel_mismatch(np.zeros((2, 3, 4), np.float32), ref, tol) is None
    out = np.zeros((2, 3, 4), np.float32)
    out[1, 2, 3] = np.nan
    assert "NaN" in mel_mismatch(out, ref, tol)
    assert "shape" in mel_mismatch(out[:1], ref, tol)
    out[1, 2, 3] = 2e-4
    assert "(1, 2, 3)" in mel_mismatch(out, ref, tol)
