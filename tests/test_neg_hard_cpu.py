"""No GPU: ranking.sample_negatives(..., draws=M, sums): the CPU statement of FMX_NEG_HARDEST | FMX_NEG_DRAWS(M) (include/fmx.h,
DESIGN.md section 13): the attempts are walked in order until M are accepted and the accepted draw with the highest
r = b_d + S_q . S_d wins, the earlier attempt on equal scores.

The hand-sized case is pinned to literals that were derived once with Python integers (the draws) and fractions.Fraction (the
scores) by hand() below, which the test runs again next to the product code."""
from fractions import Fraction as F

import numpy as np
import pytest

from libfm_amd.ranking import NEG_ATTEMPTS, sample_negatives
from test_bpr_sampler_cpu import draw, lists_case


def sums_case(seed, Q, C, k):
    rng = np.random.default_rng(seed)
    return dict(query_sums=rng.normal(0, 1, (Q, k)), cand_sums=rng.normal(0, 1, (C, k)), cand_scal=rng.normal(0, 1, C))


# ---- draws = 1 is the uniform sampler ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 8, 1000])
def test_one_draw_with_sums_is_the_uniform_sampler(C):
    Q, T = 30, 2000
    q, c, ex = lists_case(40 + C, Q, C, T)
    sums = sums_case(C, Q, C, 5)
    for n_neg, seed, epoch in ((1, 0, 0), (3, 7, 2), (2, (1 << 64) - 1, (1 << 40) + 5)):
        for lists in (ex, None):
            ref, ref_forced = sample_negatives(seed, epoch, q, c, n_neg, C, lists)
            neg, forced = sample_negatives(seed, epoch, q, c, n_neg, C, lists, draws=1, **sums)
            assert forced == ref_forced and neg.dtype == np.uint32 and np.array_equal(neg, ref)
            neg, forced = sample_negatives(seed, epoch, q, c, n_neg, C, lists, draws=1)      # ... and needs no sums
            assert forced == ref_forced and np.array_equal(neg, ref)
    if C == 1:
        assert ref_forced == T * 2                                # the only candidate is the positive


# ---- the hand-sized case -----------------------------------------------------------------------------------------------------
# Q = 3, C = 6, k = 2.  Candidates 1 and 4 tie for query 0 (1/4 + 1/2 + 1/2 = 1/4 + 1 = 5/4, the highest score of query 0); query 1
# excludes all but candidate 3 (its list repeats a row); query 2 excludes the whole catalogue.
SQ = [[F(1), F(1, 2)], [F(-1), F(1, 4)], [F(1, 2), F(1, 2)]]
SC = [[F(0), F(0)], [F(1, 2), F(1)], [F(-1), F(1)], [F(1, 4), F(-1, 2)], [F(1), F(0)], [F(-1, 2), F(-1, 2)]]
B = [F(1, 2), F(1, 4), F(0), F(-1, 4), F(1, 4), F(1)]
Q_ROW = [0, 1, 0, 2, 0, 1, 0, 2]
C_ROW = [2, 3, 0, 1, 5, 0, 3, 4]
EX = [[], [0, 1, 2, 4, 5, 1], [5, 4, 3, 2, 1, 0]]


def hand(seed, epoch, n_neg, M, C=6):
    """the rule, pair by pair, in Python integers and Fractions: (neg, forced, pairs in which an equal score met the best)"""
    neg, forced, ties = [], 0, []
    for p in range(len(Q_ROW) * n_neg):
        t = p // n_neg
        q = Q_ROW[t]
        best, accepted = None, 0
        for a in range(NEG_ATTEMPTS):
            d = draw(seed, epoch, p, a, C)
            if d == C_ROW[t] or d in EX[q]:
                continue
            accepted += 1
            r = B[d] + sum(x * y for x, y in zip(SQ[q], SC[d]))
            if best is None or r > best[0]:
                best = (r, d)
            elif r == best[0] and d != best[1]:
                ties.append(p)
            if accepted == M:
                break
        if best is None:
            forced += 1
            neg.append(draw(seed, epoch, p, NEG_ATTEMPTS - 1, C))
        else:
            neg.append(best[1])
    return neg, forced, ties


def test_hand_sized_case_is_pinned():
    want = [4, 4, 2, 5, 4, 1, 5, 4, 1, 4, 3, 3, 0, 1, 0, 2]
    neg, forced, ties = hand(0, 3, 2, 4)
    assert neg == want and forced == 6
    assert 1 in ties and want[1] == 4                             # pair 1: candidates 4 and 1 tie at 5/4, attempt of 4 came first
    f = lambda x: np.array(x, dtype=np.float64)
    got, got_forced = sample_negatives(0, 3, Q_ROW, C_ROW, 2, 6, EX, draws=4, query_sums=f(SQ), cand_sums=f(SC), cand_scal=f(B))
    assert got.dtype == np.uint32 and got.tolist() == want and got_forced == 6
    # query 1 (interactions 1 and 5): its only eligible candidate is 3 -- the positive of interaction 1 (forced), the pick of 5
    assert got[10:12].tolist() == [3, 3]
    assert got[2:4].tolist() == [draw(0, 3, p, 15, 6) for p in (2, 3)]
    # query 2 (interactions 3 and 7) excludes everything: forced, the 16th draw as it is
    assert [int(got[p]) for p in (6, 7, 14, 15)] == [draw(0, 3, p, 15, 6) for p in (6, 7, 14, 15)]
    # other M on the same case, against the hand rule
    for M in (2, 3, 16):
        neg, forced, _ = hand(0, 3, 2, M)
        got, got_forced = sample_negatives(0, 3, Q_ROW, C_ROW, 2, 6, EX, draws=M, query_sums=f(SQ), cand_sums=f(SC), cand_scal=f(B))
        assert got.tolist() == neg and got_forced == forced == 6


def test_nan_scores_lose_to_numbers_and_keep_the_first_among_themselves():
    f = lambda x: np.array(x, dtype=np.float64)
    scal = f(B)
    scal[4] = np.nan                                              # the tie partner of candidate 1 for query 0
    got, _ = sample_negatives(0, 3, Q_ROW, C_ROW, 2, 6, EX, draws=4, query_sums=f(SQ), cand_sums=f(SC), cand_scal=scal)
    assert got[1] == 1                                            # pair 1 drew 4 first, then 1: the number replaces the NaN
    scal[:] = np.nan
    got, forced = sample_negatives(0, 3, Q_ROW, C_ROW, 2, 6, EX, draws=4, query_sums=f(SQ), cand_sums=f(SC), cand_scal=scal)
    ref, ref_forced = sample_negatives(0, 3, Q_ROW, C_ROW, 2, 6, EX)
    assert forced == ref_forced and np.array_equal(got, ref)      # all NaN: the first accepted draw, as the uniform sampler


def test_the_pick_is_the_best_of_the_first_m_accepted():
    Q, C, T, n_neg, M, k = 25, 64, 1500, 2, 5, 7
    q, c, ex = lists_case(77, Q, C, T)
    sums = sums_case(3, Q, C, k)
    neg, forced = sample_negatives(5, 1, q, c, n_neg, C, ex, draws=M, **sums)
    assert forced == 0
    sets = [set(int(x) for x in e) for e in ex]
    for p in range(0, T * n_neg, 13):
        t = p // n_neg
        acc = [d for d in (draw(5, 1, p, a, C) for a in range(NEG_ATTEMPTS)) if d != c[t] and d not in sets[q[t]]][:M]
        r = [sums["cand_scal"][d] + sums["query_sums"][q[t]] @ sums["cand_sums"][d] for d in acc]
        assert int(neg[p]) == acc[int(np.argmax(r))]


def test_bad_arguments():
    sums = sums_case(1, 2, 10, 3)
    for draws in (0, -1, 17):
        with pytest.raises(ValueError):
            sample_negatives(1, 0, [0], [0], 1, 10, draws=draws, **sums)
    with pytest.raises(ValueError):
        sample_negatives(1, 0, [0], [0], 1, 10, draws=2)          # no sums
    with pytest.raises(ValueError):
        sample_negatives(1, 0, [0], [0], 1, 10, draws=2, query_sums=sums["query_sums"], cand_sums=sums["cand_sums"])
    with pytest.raises(ValueError):
        sample_negatives(1, 0, [0], [0], 1, 9, draws=2, **sums)   # the tables do not cover the catalogue
    neg, forced = sample_negatives(1, 0, [], [], 3, 10, draws=4, **sums)
    assert len(neg) == 0 and forced == 0
