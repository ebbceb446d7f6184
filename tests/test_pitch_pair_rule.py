"""The rule hbk_pitch_shift pairs a call's clips by (ps_span_kernel / ps_rank_kernel
/ ps_group_kernel in csrc/hbk_pitch.hip), written in numpy and run on the
training clips' own spans.

A vocoder workgroup runs the union of its two clips' non-silent spans plus 36
frames. The rule: sort the list positions by (bucket of the last non-zero
sample, 360 samples per bucket, silent clips first; first non-zero sample; list
position), pair neighbours, start the pairs with the most frames first.

The clips are the bench's: speech_clips (half positives, half adversarials)
placed by target_length_offsets into 23,040 samples, every fourth treated as
having gone through the 7-band EQ, whose ringing keeps it non-zero to the last
sample. The bounds are the issue's: the paired union share stays within 0.03 of
the clips' own share, and below the union of list neighbours.
"""
import numpy as np

T = 23040
QUANT = 360  # kPsQuant
HOP, TAIL = 7, 36


def pair_order(lo, hi):
    """(list positions in span order, pairs of them most frames first) for spans
    [lo, hi] (hi < 0: silent)"""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    q = np.where(hi < 0, 0, 1 + hi // QUANT)
    first = np.where(hi < 0, 0, lo)
    order = np.lexsort((np.arange(lo.size), first, q))  # last key is the primary one
    pairs = [order[i:i + 2] for i in range(0, order.size, 2)]
    frames = np.array([_frames(lo[p].min(), hi[p].max()) for p in pairs])
    start = np.lexsort((np.arange(len(pairs)), -frames))
    return order, [pairs[i] for i in start]


def _frames(lo, hi):
    return 0 if hi < lo else (hi - lo + 1) / HOP + TAIL


def _share(pairs, lo, hi):
    """frames the workgroups run, as a share of every frame of every clip"""
    run = sum(len(p) * _frames(lo[p].min(), hi[p].max()) for p in pairs)
    return run / (lo.size * (T / HOP + TAIL))


def _spans(n=2048):
    from heybuddy.dataset.augmented import target_length_offsets
    from heybuddy.synthetic import speech_clips
    _, pos_len = speech_clips("hello world", n // 2, seed=11)
    _, adv_len = speech_clips("hello world", n - n // 2, seed=12, adversarial=True)
    lens = np.minimum(np.concatenate([pos_len, adv_len]).astype(np.int64), T)
    state = np.random.get_state()
    np.random.seed(5)
    pre = target_length_offsets(lens, T).astype(np.int64)
    np.random.set_state(state)
    perm = np.random.default_rng(7).permutation(n)  # a batch mixes positives and adversarials
    lo, hi = pre[perm], (pre + lens - 1)[perm]
    hi[::4] = T - 1  # EQ'd: non-zero to the end
    return lo, hi


def test_pairing_rule_keeps_the_union_near_the_clips_own_spans():
    lo, hi = _spans()
    n = lo.size
    own = _share([np.array([i]) for i in range(n)], lo, hi)
    listed = _share([np.arange(i, min(i + 2, n)) for i in range(0, n, 2)], lo, hi)
    order, pairs = pair_order(lo, hi)
    paired = _share(pairs, lo, hi)
    print(f"{n} clips: own span share {own:.3f}, list-order union {listed:.3f}, paired union {paired:.3f}")
    assert sorted(order.tolist()) == list(range(n))
    assert sorted(np.concatenate(pairs).tolist()) == list(range(n))
    assert paired <= own + 0.03
    assert paired < listed
    fr = [_frames(lo[p].min(), hi[p].max()) for p in pairs]
    assert all(a >= b for a, b in zip(fr, fr[1:]))  # the longest workgroups start first


def test_pairing_rule_edge_cases():
    # silent clips pair with each other and come last in the start order; an odd count leaves one alone
    none = 2 ** 31 - 1
    lo = np.array([100, none, 5000, none, 100, 0, none])
    hi = np.array([9000, -1, 23039, -1, 9000, 23039, -1])
    order, pairs = pair_order(lo, hi)
    assert order.tolist() == [1, 3, 6, 0, 4, 5, 2]
    assert [p.tolist() for p in pairs] == [[4, 5], [2], [6, 0], [1, 3]]
