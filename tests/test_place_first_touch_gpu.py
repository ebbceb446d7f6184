"""Placement on first touch on the GPU: with it on (eq_kernel,
tanh_distortion_kernel and augment_kernel read the source rows through the
placement, place_kernel writes the other clips only) the augmented batch
equals the place-everything path bit for bit.

T = 23,040, batches of 4, 24 clips with forced coins, so that every route
occurs: EQ-first, tanh-first, EQ and tanh on one clip, augment-first with and
without background noise / reverb / folded colored noise, a clip the colored
group path does not cover (coloured from x, so placed), pitch-first and
band-stop-first (placed as before). Source lengths 1, 7, T - 1, T, T + 960 and
0 with pre 0, 3 (unaligned) and T - len rotate over the clips, so every route
sees every length. The source rows are random past their valid length too: a
load that is not masked shows.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 23040
N, BATCH = 24, 4
LENGTHS = (1, 7, T - 1, T, T + 960, 0)

EQ = (0, 5, 9, 13, 20, 21)
TANH = (1, 5, 6, 10, 14, 20, 22)  # 5 and 20: EQ and tanh on one clip
PITCH_BATCH, BANDSTOP_BATCH = 1, 2
COLORED_BATCHES = (3, 4)
COLORED_ODD_CLIP = 18             # another f_decay than its batch's first clip: coloured from x
NOISE_BATCHES, REVERB_BATCHES = (0, 3), (0, 4)
# placed by place_kernel: the pitch-shift and band-stop batches' clips that neither EQ nor tanh
# reads first, and the clip colored_noise_kernel colours
PLACED = (4, 7, 8, 11, 18)


@pytest.fixture(scope="module")
def generator():
    from heybuddy.dataset.augmented import AugmentedAudioGenerator
    from heybuddy.synthetic import impulse_responses, noise_bank
    gen = AugmentedAudioGenerator([], device_id=0, augmentation_dataset=noise_bank(6, seed=3),
                                  impulse_response_dataset=impulse_responses(4, seed=4), batch_size=BATCH)
    gen.augmenter.plan.COLORED_GROUP_MIN = BATCH  # the group (folded) path for batches of 4
    return gen


def _prepared(gen, lens, pre):
    """One call's draws with the coins forced to the tables above."""
    from heybuddy.dataset.augmented import eq_coefficients, eq_parameters
    np.random.seed(11)
    torch.manual_seed(11)
    aug = gen.augmenter
    aug.noise_idx = aug.ir_idx = 0
    coins = np.ones((N // BATCH, 2))
    coins[list(NOISE_BATCHES), 0] = 0.0
    coins[list(REVERB_BATCHES), 1] = 0.0
    pr = aug.prepare(N, coins)
    batch = np.arange(N) // BATCH
    eq_idx = np.array(EQ, dtype=np.int32)
    pr["eq"] = (torch.from_numpy(eq_coefficients(eq_parameters(eq_idx.size, 6.0))), torch.from_numpy(eq_idx))
    amount = np.full(N, np.nan, dtype=np.float32)
    amount[list(TANH)] = np.linspace(0.001, 0.1, len(TANH), dtype=np.float32)
    pr["tanh"] = torch.from_numpy(amount)
    f = aug.pitch_shifts[0]
    pr["pitch"] = [(f.numerator, f.denominator,
                    torch.from_numpy(np.flatnonzero(batch == PITCH_BATCH).astype(np.int32)))]
    bs = np.flatnonzero(batch == BANDSTOP_BATCH).astype(np.int32)
    pr["bandstop"] = (torch.from_numpy(bs), torch.full((bs.size,), 0.05), torch.full((bs.size,), 0.1))
    c_snr = np.where(np.isin(batch, COLORED_BATCHES), 10.0, np.nan).astype(np.float32)
    c_fd = np.full(N, 0.5, dtype=np.float32)
    c_fd[COLORED_ODD_CLIP] = 1.5
    pr["colored"] = (torch.from_numpy(c_fd), torch.from_numpy(c_snr), 1234)
    pr["route"] = aug.routes(pr)
    return {"lens": lens, "pre": pre, "chain": pr}


def _geometry(rot):
    lens = np.array([LENGTHS[(i + rot) % 6] for i in range(N)], dtype=np.int32)
    room = T - np.minimum(lens, T)
    kind = (np.arange(N) // 6 + rot) % 3
    pre = np.where(kind == 0, 0, np.where(kind == 1, np.minimum(3, room), room)).astype(np.int32)
    return lens, pre


@pytest.fixture(scope="module")
def source():
    g = torch.Generator().manual_seed(5)
    return (0.1 * torch.randn(N, T + 960, generator=g)).cuda()


@pytest.mark.parametrize("rot", range(6))
def test_first_touch_is_bit_identical(generator, source, monkeypatch, rot):
    from heybuddy.dataset.augmented import ROUTE_AUGMENT, ROUTE_EQ, ROUTE_PLACE, ROUTE_TANH
    lens, pre = _geometry(rot)
    outs = []
    for on in ("0", "1"):
        monkeypatch.setenv("HBK_PLACE_FIRST_TOUCH", on)
        generator.placed_rows = None
        prepared = _prepared(generator, lens, pre)
        outs.append(generator.augment_device(source, lens, prepared=prepared))
        route = prepared["chain"]["route"]
        if on == "0":
            assert generator.placed_rows is None  # place_kernel placed every clip
            continue
        # what place_kernel was given, and that every other route was taken
        assert generator.placed_rows.tolist() == list(PLACED)
        assert np.flatnonzero(route == ROUTE_PLACE).tolist() == list(PLACED)
        assert np.flatnonzero(route == ROUTE_EQ).tolist() == list(EQ)
        assert np.flatnonzero(route == ROUTE_TANH).tolist() == [c for c in TANH if c not in EQ]
        rest = [c for c in range(N) if c not in EQ + TANH + PLACED]
        assert np.flatnonzero(route == ROUTE_AUGMENT).tolist() == rest
        batches = {c // BATCH for c in rest}
        assert batches & set(NOISE_BATCHES) and batches & set(REVERB_BATCHES) and batches & set(COLORED_BATCHES)
        assert batches - set(NOISE_BATCHES) - set(REVERB_BATCHES) - set(COLORED_BATCHES)  # and a plain clip
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_kernels_read_the_view_like_place_kernel(source):
    """Each kernel alone: EQ and tanh over source rows through the view equal
    the same kernel over place_clips' rows, and place_clips with a list writes
    the listed rows only."""
    from heybuddy.dataset.augmented import eq_coefficients, eq_parameters
    from heybuddy.kernels import SourceView, place_clips, seven_band_eq, tanh_distortion
    lens, pre = _geometry(2)
    dl, dp = torch.from_numpy(lens).cuda(), torch.from_numpy(pre).cuda()
    placed = place_clips(source, lens, pre, T)
    rows = torch.arange(0, N, 2, dtype=torch.int32)
    part = torch.full((N, T), 7.0, device="cuda")
    place_clips(source, dl, dp, T, idx=rows, out=part)
    assert torch.equal(part[0::2], placed[0::2]) and bool((part[1::2] == 7.0).all())
    view = SourceView(source, dl, dp)
    np.random.seed(3)
    torch.manual_seed(3)
    idx = torch.arange(N, dtype=torch.int32)
    coef = torch.from_numpy(eq_coefficients(eq_parameters(N, 6.0)))
    want = seven_band_eq(placed.clone(), coef, idx=idx)
    got = seven_band_eq(torch.full((N, T), float("nan"), device="cuda"), coef, idx=idx, source=view)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    amount = torch.linspace(0.001, 0.1, N)
    want = tanh_distortion(placed.clone(), amount)
    buf = torch.full((N, T), float("nan"), device="cuda")
    got = tanh_distortion(buf, amount, out=buf, source=view)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
