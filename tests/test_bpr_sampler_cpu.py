"""No GPU: ranking.sample_negatives, the CPU statement of the negatives fmx_pair_epoch_sampled draws on the device
(include/fmx.h, "BPR on query x candidate interactions").

The literals below were computed once with Python integers from the formula
    draw(seed, epoch, p, a) = (mix64(seed ^ epoch * 0x9E3779B97F4A7C15 ^ (p * 0xD6E8FEB86659FD93 + a * 0xA24BAED4963EE407
                               + 0x9FB21C651E98DF25)) * C) >> 64      (all mod 2^64)
so that a vectorised implementation that loses bits is caught."""
import numpy as np

from libfm_amd.ranking import NEG_ATTEMPTS, sample_negatives

M = (1 << 64) - 1


def mix64(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M
    return x ^ (x >> 31)


def draw(seed, epoch, p, a, C):
    """the formula in Python integers"""
    return (mix64((seed ^ (epoch * 0x9E3779B97F4A7C15 & M)
                   ^ ((p * 0xD6E8FEB86659FD93 + a * 0xA24BAED4963EE407 + 0x9FB21C651E98DF25) & M)) & M) * C) >> 64


def lists_case(seed, Q, C, T, frac=0.25):
    """interactions and per-query exclusion lists (unsorted, with repeats, at most frac * C distinct rows each)"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, Q, T)
    c = rng.integers(0, C, T)
    ex = []
    for _ in range(Q):
        m = int(rng.integers(0, int(C * frac) + 1))
        e = rng.choice(C, m, replace=False)
        ex.append(np.concatenate([e, e[: m // 3]])[rng.permutation(m + m // 3)] if m else e)
    return q, c, ex


def test_hand_computed_draws():
    assert draw(7, 0, 0, 0, 50) == 12
    assert draw(123456789, 3, 1000, 2, 100000) == 93303
    assert draw((1 << 64) - 1, (1 << 40) + 5, (1 << 31) - 3, 15, 4294967295) == 192208353
    assert [draw(7, 0, p, 15, 50) for p in range(10)] == [9, 47, 39, 13, 43, 0, 6, 18, 23, 23]
    # through the product code: attempt 0 when nothing is rejected ...
    neg, forced = sample_negatives(7, 0, [0], [49], 1, 50)
    assert neg.tolist() == [12] and forced == 0 and neg.dtype == np.uint32
    # ... p = 1000 is interaction 1000 at n_neg = 1; attempts 0 and 1 are made to fail by excluding their draws
    d = [draw(123456789, 3, 1000, a, 100000) for a in range(3)]
    assert len(set(d)) == 3
    ex = [[] for _ in range(1001)]
    ex[5] = [d[1], d[0], d[0]]
    neg, forced = sample_negatives(123456789, 3, np.full(1001, 5), np.full(1001, 1), 1, 100000, exclude=ex)
    assert int(neg[1000]) == 93303 and forced == 0
    # ... a seed and an epoch that use all 64 bits, the largest candidate count
    neg, forced = sample_negatives((1 << 64) - 1, (1 << 40) + 5, [0, 0], [1, 1], 1, 4294967295)
    assert neg.tolist() == [draw((1 << 64) - 1, (1 << 40) + 5, p, 0, 4294967295) for p in range(2)]


def test_everything_excluded_is_forced_with_the_last_draw():
    neg, forced = sample_negatives(7, 0, np.zeros(10, int), np.zeros(10, int), 1, 50, exclude=[list(range(50))])
    assert forced == 10
    assert neg.tolist() == [9, 47, 39, 13, 43, 0, 6, 18, 23, 23]           # attempt 15 = the 16th draw
    neg, forced = sample_negatives(3, 2, [0, 0, 0], [0, 0, 0], 2, 1)         # one candidate, and it is the positive
    assert forced == 6 and neg.tolist() == [0] * 6


def test_no_negative_is_excluded_or_the_positive():
    Q, C, T, n_neg = 40, 64, 3000, 3
    q, c, ex = lists_case(11, Q, C, T)
    neg, forced = sample_negatives(5, 1, q, c, n_neg, C, exclude=ex)
    assert forced == 0 and len(neg) == T * n_neg and neg.max() < C
    sets = [set(int(x) for x in e) for e in ex]
    for p, d in enumerate(neg):
        t = p // n_neg
        assert int(d) != c[t] and int(d) not in sets[q[t]]
    # every negative is the first acceptable attempt of the formula
    for p in range(0, T * n_neg, 97):
        t = p // n_neg
        for a in range(NEG_ATTEMPTS):
            d = draw(5, 1, p, a, C)
            if d != c[t] and d not in sets[q[t]]:
                break
        assert int(neg[p]) == d
    # the CSR form of the lists gives the same
    ptr = np.concatenate([[0], np.cumsum([len(e) for e in ex])])
    neg2, _ = sample_negatives(5, 1, q, c, n_neg, C, exclude=(ptr, np.concatenate(ex)))
    assert np.array_equal(neg, neg2)


def test_counts_are_uniform_over_the_eligible_sets():
    Q, C, T = 20, 50, 200000
    q, c, ex = lists_case(21, Q, C, T)
    neg, forced = sample_negatives(9, 0, q, c, 1, C, exclude=ex)
    assert forced == 0
    elig = np.ones((Q, C))
    for i, e in enumerate(ex):
        elig[i, e] = 0
    # pair t draws uniformly from the eligible rows of q[t] other than c[t]
    e_t = elig[q].copy()
    e_t[np.arange(T), c] = 0
    prob = e_t / e_t.sum(1, keepdims=True)
    expect, var = prob.sum(0), (prob * (1 - prob)).sum(0)
    counts = np.bincount(neg, minlength=C)
    z = (counts - expect) / np.sqrt(var)
    assert np.abs(z).max() < 5.0, z


def test_epochs_differ_and_repeat():
    q, c, ex = lists_case(31, 30, 50, 5000)
    a0, _ = sample_negatives(1, 0, q, c, 1, 50, exclude=ex)
    a1, _ = sample_negatives(1, 1, q, c, 1, 50, exclude=ex)
    b0, _ = sample_negatives(1, 0, q, c, 1, 50, exclude=ex)
    s2, _ = sample_negatives(2, 0, q, c, 1, 50, exclude=ex)
    assert np.array_equal(a0, b0)
    assert 0.0 < np.mean(a0 == a1) < 0.1 and 0.0 < np.mean(a0 == s2) < 0.1      # chance agreement is about 1 / 40


def test_n_neg_uses_p_equal_t_times_n_neg_plus_s():
    q, c = np.array([0, 1, 2]), np.array([3, 4, 5])
    neg, forced = sample_negatives(13, 4, q, c, 4, 1000)
    assert forced == 0 and len(neg) == 12
    for t in range(3):
        for s in range(4):
            p = t * 4 + s
            for a in range(NEG_ATTEMPTS):
                d = draw(13, 4, p, a, 1000)
                if d != c[t]:
                    break
            assert int(neg[p]) == d


def test_empty_and_bad_arguments():
    import pytest
    neg, forced = sample_negatives(1, 0, [], [], 3, 10)
    assert len(neg) == 0 and forced == 0
    with pytest.raises(ValueError):
        sample_negatives(1, 0, [0], [0], 0, 10)
    with pytest.raises(ValueError):
        sample_negatives(1, 0, [0], [0], 1, 0)
    # exclusion lists must cover every query row that occurs, and name candidate rows only (FMX_E_ARG on the device)
    sample_negatives(1, 0, [1], [0], 1, 10, exclude=[[1], [2]])
    with pytest.raises(ValueError):
        sample_negatives(1, 0, [2], [0], 1, 10, exclude=[[1], [2]])           # lists for rows 0 and 1 only
    with pytest.raises(ValueError):
        sample_negatives(1, 0, [2], [0], 1, 10, exclude=(np.array([0, 1, 2]), np.array([1, 2])))
    with pytest.raises(ValueError):
        sample_negatives(1, 0, [0], [0], 1, 10, exclude=[[10]])               # would alias into the next query's keys
