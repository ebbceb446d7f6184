"""Every route hbk_mel_plan_create can take, against the fp64 oracle (GPU).

Each case builds a MelPlan, asserts through ``MelPlan.info()``
(hbk_mel_plan_info) that it got the intended kernel and edge0, runs it and
compares every output bin with ``oracle.mel.mel_frames``. The windows, banks,
clips, bounds and the checker are those of tests/test_mel_routes.py, which
shows on the CPU that the bounds are attainable in f32 and that the checker
fails on the kernel faults it is meant to find.

Kernels: 1 = mel_frames_kernel (v1), 2 = mel_frames_v2_kernel, 3 =
mel_frames_mfma_kernel, 4 / 8 = mel_frames_soa_kernel with 4 / 8 waves; 2, 3,
4 and 8 come with EDGE0 true (window W0) and false (W1, W2).

Every call runs on the current stream and on a stream masked to 4 CUs, where
the persistent grid shrinks to 8-32 blocks and each block walks its loop at
least three times (both prefetch buffers of the MFMA and SoA kernels, and the
clamped prefetch past the last group); the two outputs must be bit-identical.
"""
import numpy as np
import pytest
import torch

import test_mel_routes as R

pytestmark = pytest.mark.gpu

FLOOR_VALUE = 10.0 * np.log10(1e-10) / 10.0 + 2.0


@pytest.fixture(scope="module")
def masked():
    """A stream on 4 CUs (one hipExtStreamCreateWithCUMask stream for the module)."""
    from heybuddy.pipeline import masked_stream
    ms = masked_stream(torch.device("cuda", torch.cuda.current_device()), [0, 1, 2, 3])
    yield ms.stream
    ms.destroy()


def make_plan(monkeypatch, route, window_name, bank_name, **kw):
    """route: "bank" (whatever the bank selects), "v1env", "v2", "mfma", "soa4", "soa8"."""
    from heybuddy.kernels import MelPlan
    for name in ("HBK_MEL_V1", "HBK_MEL_V4", "HBK_MEL_MFMA"):
        monkeypatch.delenv(name, raising=False)
    env = {"v1env": {"HBK_MEL_V1": "1"}, "soa4": {"HBK_MEL_V4": "1"}, "soa8": {"HBK_MEL_V4": "8"}}.get(route, {})
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # read inside hbk_mel_plan_create
    plan = MelPlan(R.window(window_name), R.bank(bank_name), **kw)
    if route == "mfma":
        plan.set_variant(1)
    want = {"bank": 1, "v1env": 1, "v2": 2, "mfma": 3, "soa4": 4, "soa8": 8}[route]
    info = plan.info()
    host = R.route_on_host(R.bank(bank_name), env)
    assert info["kernel"] == want, info
    assert info["kernel"] == (3 if route == "mfma" else host["kernel"]), (info, host)
    assert info["edge0"] == int(want != 1 and R.window_edge0(R.window(window_name))), info
    assert {k: info[k] for k in ("taps", "nk2", "need256", "n_mels")} == \
        {k: host[k] for k in ("taps", "nk2", "need256", "n_mels")}, (info, host)
    return plan


def run_both(plan, dev, n_frames, masked):
    """The plan on the current stream and on the 4-CU stream: bit-identical."""
    out = plan(dev, n_frames)
    masked.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(masked):
        out_m = plan(dev, n_frames)
    masked.synchronize()
    a, b = out.cpu().numpy(), out_m.cpu().numpy()
    assert a.tobytes() == b.tobytes(), "the 4-CU masked stream and the whole device disagree"
    return a


ROUTES = (
    [("bank", w, b) for w in ("W0", "W2") for b in ("B1", "B2", "B3", "B5", "M2")]
    + [("v1env", "W0", "B0")]
    + [(r, w, b) for r in ("v2", "mfma") for w in ("W1", "W2") for b in ("B0", "B4")]
    # EDGE0 = true: the production plan (whole device and 4 CUs bit-identical: DESIGN.md, Parity)
    # and the clamped filter layout
    + [(r, "W0", b) for r in ("v2", "mfma") for b in ("B0", "B4")]
    + [("soa4", w, b) for w in ("W0", "W1", "W2") for b in ("B0", "B4")]
    + [("soa8", w, "B0") for w in ("W0", "W2")]
)


@pytest.mark.parametrize("route,window_name,bank_name", ROUTES)
def test_route_matches_oracle(monkeypatch, masked, route, window_name, bank_name):
    ref, tol, mel_pow = R.case_reference(bank_name, window_name)
    R.assert_bound_is_sharp(tol, mel_pow)
    plan = make_plan(monkeypatch, route, window_name, bank_name)
    dev = torch.tensor(R.clips(R.clips_for(bank_name))).cuda()
    n_mels = R.bank(bank_name).shape[1]
    for n_clips, n_frames in ((R.N_CLIPS, R.N_FRAMES), (3, 1), (1, R.N_FRAMES)):
        out = run_both(plan, dev[:n_clips], n_frames, masked)
        assert out.shape == (n_clips, n_frames, n_mels)
        sub = (slice(0, n_clips), slice(0, n_frames))
        err, ratio = R.worst_ratio(out, ref[sub], tol[sub])
        print(f"mel route kernel {plan.info()['kernel']} edge0 {plan.info()['edge0']} {window_name} {bank_name} "
              f"{n_clips}x{n_frames}: max |d| {err:.3e}, max |d|/bound {ratio:.3f}")
        bad = R.mel_mismatch(out, ref[sub], tol[sub])
        assert bad is None, bad
        if bank_name == "B3":  # the all-zero filter
            assert np.abs(out[..., R.B3_ZERO_COLUMN] - FLOOR_VALUE).max() <= 1e-6


GEOMETRY_ROUTES = [("bank", "W2", "B2"), ("v2", "W2", "B0"), ("mfma", "W2", "B0"), ("soa4", "W2", "B0")]


@pytest.mark.parametrize("geom", R.GEOMETRY)
@pytest.mark.parametrize("route,window_name,bank_name", GEOMETRY_ROUTES)
def test_scaling_and_geometry(monkeypatch, masked, route, window_name, bank_name, geom):
    pcm, n_frames, kw = R.geometry_case(geom, R.clips_for(bank_name))
    p = dict(R.DEFAULTS, **kw)
    ref, tol, mel_pow = R.reference(pcm, n_frames, R.window(window_name), R.bank(bank_name),
                                    flat=bank_name == "B0", **kw)
    R.assert_bound_is_sharp(tol, mel_pow, log_floor=p["log_floor"], out_div=p["out_div"])
    plan = make_plan(monkeypatch, route, window_name, bank_name, **kw)
    if geom == "row_stride":  # rows 24,000 apart; what lies between them is never read
        big = torch.full((pcm.shape[0], 24000), float("nan"))
        big[:, :pcm.shape[1]] = torch.tensor(pcm)
        dev = big.cuda()[:, :pcm.shape[1]]
        assert dev.stride(0) == 24000
    else:
        dev = torch.tensor(pcm).cuda()
    out = run_both(plan, dev, n_frames, masked)
    err, ratio = R.worst_ratio(out, ref, tol)
    print(f"mel geometry kernel {plan.info()['kernel']} {geom}: max |d| {err:.3e}, max |d|/bound {ratio:.3f}")
    bad = R.mel_mismatch(out, ref, tol)
    assert bad is None, bad


# A non-finite sample reaches frame f at offset s - 160 f. S_LIVE: offsets 420, 260, 100 of
# frames 48-50, where W0, W1 and W2 are all non-zero. S_EDGE: offsets 490, 330, 170, 10 of
# frames 47-50; W0 is zero at 490 and 10, inside the 32-sample edge rows.
S_LIVE, LIVE_FRAMES = 160 * 50 + 100, (48, 49, 50)
S_EDGE, EDGE_FRAMES, EDGE_ZERO_WEIGHT_FRAMES = 160 * 50 + 10, (47, 48, 49, 50), (47, 50)
NONFINITE_ROUTES = [("v1env", "W0", "B0"), ("v2", "W0", "B0"), ("mfma", "W0", "B0"), ("soa4", "W0", "B0"),
                    ("soa8", "W0", "B0"), ("bank", "W2", "B3"), ("v2", "W1", "B0"), ("mfma", "W2", "B0"),
                    ("soa4", "W1", "B0"), ("soa8", "W2", "B0")]


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("route,window_name,bank_name", NONFINITE_ROUTES)
def test_nonfinite_sample_under_nonzero_weight(monkeypatch, masked, route, window_name, bank_name, value):
    """All mels of exactly the covering frames are NaN (the clamp to the log
    floor keeps NaN); every other frame meets its bound."""
    ref, tol, _ = R.case_reference(bank_name, window_name)
    clip = 2
    pcm = R.clips(R.clips_for(bank_name))[:4].copy()
    pcm[clip, S_LIVE] = value
    plan = make_plan(monkeypatch, route, window_name, bank_name)
    out = run_both(plan, torch.tensor(pcm).cuda(), R.N_FRAMES, masked)
    want = np.array(ref[:4])
    want[clip, LIVE_FRAMES[0]:LIVE_FRAMES[-1] + 1] = np.nan
    bad = R.mel_mismatch(out, want, tol[:4])
    assert bad is None, bad


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("route", ["v1env", "v2", "mfma", "soa4", "soa8"])
def test_nonfinite_sample_under_zero_weight(monkeypatch, masked, route, value):
    """The oracle multiplies: NaN * 0 is NaN, so a frame is NaN even where the
    window is zero at the bad sample. v1 does the same. The EDGE0 kernels never
    load a frame's first and last 32 samples, so there they give the value of
    the clip with that sample zeroed (Parity)."""
    ref, tol, _ = R.case_reference("B0", "W0")
    clip = 1
    pcm = R.clips("speech")[:3].copy()
    pcm[clip, S_EDGE] = value
    plan = make_plan(monkeypatch, route, "W0", "B0")
    out = run_both(plan, torch.tensor(pcm).cuda(), R.N_FRAMES, masked)
    want = np.array(ref[:3])
    want[clip, EDGE_FRAMES[0]:EDGE_FRAMES[-1] + 1] = np.nan   # the oracle's answer, which v1 shares
    if plan.info()["edge0"]:
        for f in EDGE_ZERO_WEIGHT_FRAMES:                      # ... skipped rows: the sample zeroed
            want[clip, f] = ref[clip, f]
    bad = R.mel_mismatch(out, want, tol[:3])
    assert bad is None, bad


def test_two_plans_own_their_tables(monkeypatch, masked):
    """Each plan holds its tables in one device buffer of its own: two plans alive at once, run
    interleaved on 3 clips x 23 frames (69 frames: ragged for 16-, 24-, 32- and 64-frame groups), the
    first switched to the MFMA variant in between and then destroyed; the second one's output does not
    change by a bit, and every output meets the bound of its case."""
    n_clips, n_frames, length = 3, 23, 4032
    first = make_plan(monkeypatch, "v2", "W0", "B0")
    second = make_plan(monkeypatch, "bank", "W2", "B3")
    dev1 = torch.tensor(R.clips(R.clips_for("B0"))[:n_clips, :length]).cuda()
    dev2 = torch.tensor(R.clips(R.clips_for("B3"))[:n_clips, :length]).cuda()
    sub = (slice(0, n_clips), slice(0, n_frames))

    def check(out, bank_name, window_name):
        ref, tol, _ = R.case_reference(bank_name, window_name)
        bad = R.mel_mismatch(out, ref[sub], tol[sub])
        assert bad is None, bad

    check(run_both(first, dev1, n_frames, masked), "B0", "W0")
    out2 = run_both(second, dev2, n_frames, masked)
    check(out2, "B3", "W2")
    first.set_variant(1)
    assert first.info()["kernel"] == 3 and second.info()["kernel"] == 1
    check(run_both(first, dev1, n_frames, masked), "B0", "W0")
    torch.cuda.synchronize()
    first.__del__()  # hbk_mel_plan_destroy: the one hipFree of its buffer
    assert first._handle is None
    again = run_both(second, dev2, n_frames, masked)
    check(again, "B3", "W2")
    assert again.tobytes() == out2.tobytes(), "the second plan's output changed when the first was destroyed"
    assert np.abs(again[..., R.B3_ZERO_COLUMN] - FLOOR_VALUE).max() <= 1e-6


def test_refusals_on_a_plan(monkeypatch):
    from heybuddy import _native
    from heybuddy.kernels import MelPlan
    lib = _native.lib()
    for name in ("HBK_MEL_V1", "HBK_MEL_V4", "HBK_MEL_MFMA"):
        monkeypatch.delenv(name, raising=False)
    # the MFMA variant on a v1 plan: refused, the plan unchanged
    plan = MelPlan(R.window("W0"), R.bank("B1"))
    before = plan.info()
    assert before["kernel"] == 1
    assert lib.hbk_mel_set_variant(plan._handle, 1) == R.HBK_ERR_UNSUPPORTED and lib.hbk_last_error()
    assert lib.hbk_mel_set_variant(plan._handle, 2) == R.HBK_ERR_ARG and lib.hbk_last_error()
    assert plan.info() == before
    # odd hop and frames past clip_stride: refused at the hbk_mel_frames call, nothing written
    pcm = torch.zeros((2, 1024), device="cuda")
    out = torch.full((2, 8, 32), 7.0, device="cuda")
    odd = MelPlan(R.window("W0"), R.bank("B0"), hop=161)
    assert lib.hbk_mel_frames(odd._handle, pcm.data_ptr(), 2, 1024, 2, out.data_ptr(), None) == R.HBK_ERR_ARG
    assert b"even" in lib.hbk_last_error()
    ok = MelPlan(R.window("W0"), R.bank("B0"))
    assert lib.hbk_mel_frames(ok._handle, pcm.data_ptr(), 2, 1024, 5, out.data_ptr(), None) == R.HBK_ERR_ARG
    assert b"clip_stride" in lib.hbk_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    out4 = torch.full((2, 4, 32), 7.0, device="cuda")
    assert lib.hbk_mel_frames(ok._handle, pcm.data_ptr(), 2, 1024, 4, out4.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert float((out4 - FLOOR_VALUE).abs().max()) <= 1e-6  # silence sits on the log floor
