"""Placement on first touch, the routing rule alone (no GPU).

first_touch_routes gives every clip exactly one first consumer from the
chain's order: eq_kernel for a clip in the EQ list, else
tanh_distortion_kernel for one whose tanh coin came up, else augment_kernel
unless a kernel without the source view reads the clip first (its batch drew a
pitch shift or a band-stop), else place_kernel.

The shares follow from the default probabilities alone (0.25 each, the four
coins independent): EQ 0.25; tanh 0.75 * 0.25 = 0.1875; augment
0.75 * 0.75 * (0.75 * 0.75) = 0.3164; placed 0.75 * 0.75 * (1 - 0.5625) =
0.2461. Each table has 1,024 clips in batches of 16 (the pitch-shift and
band-stop coins are per batch). Over the 16 seeded tables the largest standard
deviation of a share is the augment share's, below
0.5625 * sqrt(0.4375 * 0.5625 / 1024) + sqrt(0.32 * 0.68 / 16384) = 0.013, so
the pooled shares are asserted within the 3 points the routing rule is held to.
"""
import numpy as np

from heybuddy.constants import (DEFAULT_AUGMENT_BAND_STOP_PROB, DEFAULT_AUGMENT_PITCH_SHIFT_PROB,
                                DEFAULT_AUGMENT_SEVEN_BAND_PROB, DEFAULT_AUGMENT_TANH_DISTORTION_PROB)
from heybuddy.dataset.augmented import (ROUTE_AUGMENT, ROUTE_EQ, ROUTE_PLACE, ROUTE_TANH, first_touch_routes)

N, BATCH, TABLES = 1024, 16, 16


def _coins(seed):
    rng = np.random.default_rng(seed)
    batch = np.arange(N) // BATCH
    eq = rng.random(N) < DEFAULT_AUGMENT_SEVEN_BAND_PROB
    tanh = rng.random(N) < DEFAULT_AUGMENT_TANH_DISTORTION_PROB
    pitch = (rng.random(N // BATCH) < DEFAULT_AUGMENT_PITCH_SHIFT_PROB)[batch]
    bandstop = (rng.random(N // BATCH) < DEFAULT_AUGMENT_BAND_STOP_PROB)[batch]
    return eq, tanh, pitch, bandstop


def test_every_clip_has_exactly_one_first_consumer():
    for seed in range(TABLES):
        eq, tanh, pitch, bandstop = _coins(seed)
        route = first_touch_routes(eq, tanh, pitch | bandstop)
        assert route.shape == (N,)
        members = [route == r for r in (ROUTE_PLACE, ROUTE_EQ, ROUTE_TANH, ROUTE_AUGMENT)]
        assert (np.sum(members, axis=0) == 1).all()
        # the chain's order decides: EQ before tanh before the batch transforms before augment
        assert np.array_equal(route == ROUTE_EQ, eq)
        assert np.array_equal(route == ROUTE_TANH, tanh & ~eq)
        assert np.array_equal(route == ROUTE_AUGMENT, ~eq & ~tanh & ~(pitch | bandstop))
        assert np.array_equal(route == ROUTE_PLACE, ~eq & ~tanh & (pitch | bandstop))


def test_shares_follow_the_default_probabilities():
    counts = np.zeros(4)
    for seed in range(TABLES):
        eq, tanh, pitch, bandstop = _coins(seed)
        route = first_touch_routes(eq, tanh, pitch | bandstop)
        counts += [(route == r).sum() for r in (ROUTE_EQ, ROUTE_TANH, ROUTE_AUGMENT, ROUTE_PLACE)]
    shares = 100.0 * counts / (N * TABLES)
    print("shares (EQ, tanh, augment, placed) %:", shares)
    for got, want in zip(shares, (25.0, 18.75, 31.6, 24.6)):
        assert abs(got - want) <= 3.0, (shares, want)


def test_no_transform_sends_every_clip_to_augment():
    z = np.zeros(8, dtype=bool)
    assert (first_touch_routes(z, z, z) == ROUTE_AUGMENT).all()
    assert (first_touch_routes(z, z, ~z) == ROUTE_PLACE).all()
    assert (first_touch_routes(~z, ~z, ~z) == ROUTE_EQ).all()
