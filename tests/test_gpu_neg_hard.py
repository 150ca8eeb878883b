"""GPU: BPR negatives drawn as the hardest of M accepted draws, scored on the device -- FMX_NEG_HARDEST | FMX_NEG_DRAWS(M) of
fmx_pair_sample / fmx_pair_epoch_sampled / fmx_pair_evaluate_sampled (include/fmx.h).

The device against ranking.sample_negatives(draws=M) with the fp64 factor sums of tests/topk_oracle.py: integer for integer where
every fp32 operation of the score is exact (dyadic parameters and values), within the forward bound of fp32 summation on real
values; M = 1 against the uniform sampler; the epoch and the pair metrics against the oracles on the pairs fmx_pair_sample
returns; bit reproducibility; refusals; the query slot as its own candidate slot with fmx_topk afterwards; the command line."""
import contextlib
import io

import numpy as np
import pytest

import bpr_oracle as B
import bpr_sampled_oracle as S
import datagen
import topk_oracle as T
from libfm_amd import ranking
from test_bpr_sampler_cpu import draw
from test_gpu_bpr import check_params, handle, model, start_model
from test_gpu_bpr_sampled import code, exclusion_lists, two_slots, upload
from topk_oracle import row_sums

pytestmark = pytest.mark.gpu
E_ARG = -1


def small_rows(rng, n, rows, max_nnz, values, empty_every=4):
    """rows of at most max_nnz entries, ids repeated inside a row, an empty row every `empty_every` rows"""
    ids, vals = [], []
    for r in range(rows):
        z = 0 if (empty_every and r % empty_every == empty_every - 1) else int(rng.integers(1, max_nnz + 1))
        rid = rng.integers(0, n, z)
        if z >= 2 and r % 2 == 0:
            rid[1] = rid[0]
        ids.append([int(a) for a in rid])
        vals.append([float(a) for a in values(z)])
    return datagen._pack(ids, vals, np.zeros(rows))[:2]


def sums(m, q_ent, q_rp, c_ent, c_rp):
    """the tables of the rule in fp64: S_q, S_c and b_c = linear term + 1/2 sum_f (S^2 - sum of squares)"""
    Sq, _, _ = row_sums(m, q_ent, q_rp)
    Sc, lin, half = row_sums(m, c_ent, c_rp)
    return dict(query_sums=Sq, cand_sums=Sc, cand_scal=lin + half)


def abs_sums(m, ent, rp):
    """per row: sum |v x| [rows][k], sum |w x| [rows], sum (v x)^2 [rows][k]"""
    rp = np.asarray(rp, dtype=np.int64)
    n, k = len(rp) - 1, m.v.shape[0]
    ids, xs = ent["id"].astype(np.int64), ent["value"].astype(np.float64)
    row = np.repeat(np.arange(n), np.diff(rp))
    aw = np.bincount(row, weights=np.abs(m.w[ids] * xs), minlength=n)
    av, sq = np.zeros((n, k)), np.zeros((n, k))
    for f in range(k):
        d = m.v[f, ids] * xs
        av[:, f] = np.bincount(row, weights=np.abs(d), minlength=n)
        sq[:, f] = np.bincount(row, weights=d * d, minlength=n)
    return av, aw, sq


def magnitude(m, q_ent, q_rp, c_ent, c_rp):
    """A [Q][C]: the sum of the absolute values of every product that enters r(q, d)"""
    avq, _, _ = abs_sums(m, q_ent, q_rp)
    avc, awc, sqc = abs_sums(m, c_ent, c_rp)
    return (awc + 0.5 * (avc * avc + sqc).sum(axis=1))[None, :] + avq @ avc.T


# ---- 1. exact: dyadic parameters and values ----------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 50])
@pytest.mark.parametrize("k", [1, 5, 64, 128, 1000])
def test_exact_on_dyadic_values(k, C, oracle):
    from libfm_amd import capi
    n, Q, T, g = 40, 9, 600, 7
    rng = np.random.default_rng(1000 * k + C)
    dy = lambda z: rng.choice([0.5, 1.0], z)
    q_ent, q_rp = small_rows(rng, n, Q, 3, dy)
    c_ent, c_rp = small_rows(rng, n, C, 3, dy, empty_every=4 if C > 2 else 0)
    q = rng.integers(0, Q, T).astype(np.uint32)
    c = rng.integers(0, C, T).astype(np.uint32)
    ex = exclusion_lists(rng, Q, C)
    m = model(oracle, n, k, True, True, (0.0, 0.0, 0.0), 0.25, rng.integers(-1, 2, n) / 4.0, rng.integers(-1, 2, (k, n)) / 4.0)
    # the precondition of exactness, on the fp64 side: every term of r (the products w x, v x, their squares halved, S_q S_d)
    # is a multiple of 2^-g, and the absolute values of all of them sum to less than 2^(24 - g): every partial sum, in any order,
    # is then a multiple of 2^-g below 2^(24 - g) in magnitude, which fp32 holds exactly
    for ent in (q_ent, c_ent):
        ids, xs = ent["id"].astype(np.int64), ent["value"].astype(np.float64)
        for term in (m.w[ids] * xs, m.v[:, ids] * xs, 0.5 * (m.v[:, ids] * xs) ** 2):
            assert np.array_equal(term * 2.0 ** g, np.rint(term * 2.0 ** g))
    tabs = sums(m, q_ent, q_rp, c_ent, c_rp)
    for t in (tabs["query_sums"][:, None, :] * tabs["cand_sums"][None, :, :], 0.5 * tabs["cand_sums"] ** 2, tabs["cand_scal"]):
        assert np.array_equal(t * 2.0 ** g, np.rint(t * 2.0 ** g))
    assert magnitude(m, q_ent, q_rp, c_ent, c_rp).max() < 2.0 ** (24 - g)
    h = handle(capi, n, k, True, True, (0.0, 0.0, 0.0), 0.05, m)
    upload(h, (q_ent, q_rp, c_ent, c_rp, q, c, ex))
    ties = 0
    for M in (2, 4, 16):
        for n_neg in (1, 3):
            ref, ref_forced = ranking.sample_negatives(11, M, q, c, n_neg, C, ex, draws=M, **tabs)
            neg, forced = h.pair_sample(0, n_neg, 11, M, draws=M)
            assert neg.dtype == np.uint32 and forced == ref_forced, (M, n_neg, forced, ref_forced)
            assert np.array_equal(neg, ref), (k, C, M, n_neg, int((neg != ref).sum()))
            if C == 1:
                assert forced == T * n_neg                         # the only candidate is the positive
            if C == 50:
                assert forced == 0
                uni, _ = h.pair_sample(0, n_neg, 11, M)
                assert (uni != neg).any()                          # ... and the pick is not just the first accepted draw
                r = tabs["cand_scal"][None, :] + tabs["query_sums"] @ tabs["cand_sums"].T
                rq = r[np.repeat(q, n_neg)]
                ties += int((rq == rq[np.arange(len(neg)), neg][:, None]).sum() - len(neg))
    if C == 50:
        assert ties > 0                                            # other candidates share the winners' scores: the tie rule matters
    h.close()


# ---- 2. real values: within the forward bound of fp32 summation ---------------------------------------------------------------
_DRAWS = {}


def accepted_draws(seed, epoch, q, c, C, sets, M):
    """per pair (n_neg = 1) the first M accepted draws, in Python integers"""
    key = (seed, epoch, C, M)
    if key not in _DRAWS:
        out = []
        for p in range(len(q)):
            acc = [d for d in (draw(seed, epoch, p, a, C) for a in range(ranking.NEG_ATTEMPTS)) if d != c[p] and d not in sets[q[p]]]
            out.append(acc[:M])
        _DRAWS[key] = out
    return _DRAWS[key]


@pytest.mark.parametrize("k", [1, 5, 64, 128])
def test_real_values_within_the_summation_bound(k, oracle):
    """tol = 4 (k + |x_q| + |x_d| + 4) 2^-24 A: the forward bound of fp32 recursive summation of the k + |x_q| + |x_d| + 4 or fewer
    terms per stage, A the sum of the absolute values of all products, and a factor 4 for the unspecified order.  Per pair the
    largest tol among its accepted draws is used.  The device's pick must be an accepted draw whose fp64 score is within 2 tol of
    the best, and equal the fp64 pick wherever every other distinct candidate trails the best by more than 2 tol; at most 2 % of
    the pairs may be excused from that (a CPU simulation of these distributions found 0 % at k = 1 and 5, 0.08 % at k = 64 and
    0.45 % at k = 128)."""
    from libfm_amd import capi
    n, Q, C, T, M, seed, epoch = 40, 30, 50, 4000, 8, 21, 2
    rng = np.random.default_rng(77)                                # (the rows and interactions are the same for every k)
    re = lambda z: rng.uniform(-1, 1, z)
    q_ent, q_rp = small_rows(rng, n, Q, 6, re, empty_every=7)
    c_ent, c_rp = small_rows(rng, n, C, 6, re, empty_every=9)
    q = rng.integers(0, Q, T).astype(np.uint32)
    c = rng.integers(0, C, T).astype(np.uint32)
    ex = exclusion_lists(rng, Q, C)
    prng = np.random.default_rng(k)
    m = model(oracle, n, k, True, True, (0.0, 0.0, 0.0), 0.25, prng.normal(0, 0.1, n), prng.normal(0, 0.1, (k, n)))
    h = handle(capi, n, k, True, True, (0.0, 0.0, 0.0), 0.05, m)
    upload(h, (q_ent, q_rp, c_ent, c_rp, q, c, ex))
    neg, forced = h.pair_sample(0, 1, seed, epoch, draws=M)
    h.close()
    assert forced == 0
    tabs = sums(m, q_ent, q_rp, c_ent, c_rp)
    ref, _ = ranking.sample_negatives(seed, epoch, q, c, 1, C, ex, draws=M, **tabs)
    r = tabs["cand_scal"][None, :] + tabs["query_sums"] @ tabs["cand_sums"].T
    lq, lc = np.diff(q_rp.astype(np.int64)), np.diff(c_rp.astype(np.int64))
    tol = 4.0 * (k + lq[:, None] + lc[None, :] + 4) * 2.0 ** -24 * magnitude(m, q_ent, q_rp, c_ent, c_rp)
    acc = accepted_draws(seed, epoch, q, c, C, [set(int(x) for x in e) for e in ex], M)
    excused = 0
    for p in range(T):
        a = np.array(acc[p])
        assert int(neg[p]) in acc[p], p                            # exact: integers only
        rp_, t2 = r[q[p], a], 2.0 * tol[q[p], a].max()
        assert r[q[p], neg[p]] >= rp_.max() - t2, (p, r[q[p], neg[p]], rp_.max(), t2)
        others = rp_[a != ref[p]]
        if len(others) and rp_.max() - others.max() <= t2:
            excused += 1
        else:
            assert neg[p] == ref[p], (p, int(neg[p]), int(ref[p]))
    print("k %d: %d of %d pairs within 2 tol of a second candidate, %d differ from the fp64 pick" % (k, excused, T, int((neg != ref).sum())))
    assert excused <= 0.02 * T


# ---- 3. M = 1 is the uniform sampler --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 1000])
def test_one_draw_equals_the_uniform_sampler(C, oracle):
    from libfm_amd import capi
    n, k = 40, 5
    d = two_slots(n, 20, C, 3000, 4, 30 + C)
    h = handle(capi, n, k, True, True, (0.0, 0.0, 0.0), 0.05, start_model(oracle, n, k))
    for exclude in (True, False):
        upload(h, d, exclude)
        for n_neg, seed, epoch in ((1, 0, 0), (3, 9, 4)):
            a, fa = h.pair_sample(0, n_neg, seed, epoch, draws=1)
            b, fb = h.pair_sample(0, n_neg, seed, epoch)
            assert fa == fb == 0 and np.array_equal(a, b)
    assert capi.neg_flags(1) == 0 and capi.neg_flags(4) == capi.NEG_HARDEST | (4 << 8)
    # the flag itself with one draw (not the wrapper's shortcut to flags = 0)
    st, f = h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, 64, 1, 9, 4, flags=capi.NEG_HARDEST | (1 << 8))
    assert f == 0 and st.rows == 3000
    h.close()


# ---- 4. the epoch trains on what the sampler returns ---------------------------------------------------------------------------
def hard_epochs(capi, O, d, n, k, lr, mode, batch, m0, n_neg, seed, draws=4, epochs=2, qs=0, cs=1):
    """`epochs` epochs on the device and, on the negatives fmx_pair_sample returns before each, of the oracle"""
    q_ent, q_rp, c_ent, c_rp, q, c, ex = d
    h = handle(capi, n, k, m0.k0, m0.k1, (m0.reg0, m0.regw, m0.regv), lr, m0)
    upload(h, d, ex is not None, qs, cs)
    ref = m0.copy()
    moved = 0
    for ep in range(epochs):
        neg, forced = h.pair_sample(qs, n_neg, seed, ep, draws=draws)
        uni, _ = h.pair_sample(qs, n_neg, seed, ep)
        moved += int((neg != uni).sum())
        ent, rp, pa, pb = S.join_rows(q_ent, q_rp, c_ent, c_rp, q, c, neg, n_neg)
        if mode == capi.SGD_SEQUENTIAL:
            B.pair_epoch_loop(ref, ent, rp, pa, pb, lr)
        else:
            B.pair_epoch_batch(ref, ent, rp, pa, pb, lr, batch)
        st, f = h.pair_epoch_sampled(qs, mode, batch, n_neg, seed, ep, draws=draws)
        assert f == forced == 0 and st.rows == len(neg)
        assert st.setup_seconds > 0 and st.device_seconds > 0
    assert moved > 0                                               # the negatives are not the uniform ones
    return h, ref


@pytest.mark.parametrize("k,mode,batch", [(5, "seq", 1), (64, "seq", 1), (5, "mb", 7), (64, "mb", 64), (8, "mb", 64)])
def test_epoch_trains_on_the_sampled_negatives(k, mode, batch, oracle):
    from libfm_amd import capi
    if k == 8:                                                     # the shape of test_minibatch_matches_the_batch_rule
        n, d, n_neg = 50, two_slots(50, 60, 40, 250, 7, 500, empty_every=11), 2
    else:
        n, d, n_neg = 40, two_slots(40, 30, 24, 60 if mode == "seq" else 120, 6, 400 + k, empty_every=7), 2
    m0 = start_model(oracle, n, k, seed=k)
    gmode = capi.SGD_SEQUENTIAL if mode == "seq" else capi.SGD_MINIBATCH
    h, ref = hard_epochs(capi, oracle, d, n, k, 0.05, gmode, batch, m0, n_neg, 17)
    check_params(h, ref, "hardest of 4, k %d %s batch %d" % (k, mode, batch))
    h.close()


# ---- 5. bit reproducibility, independence of the kept scratch ---------------------------------------------------------------------
def test_bit_reproducible_and_independent_of_the_scratch(oracle):
    from libfm_amd import capi
    n, k = 300, 64
    d = two_slots(n, 400, 300, 3000, 12, 800)
    m0 = start_model(oracle, n, k)
    out = []
    for first in (None, 16):
        h = handle(capi, n, k, True, True, (0.0, 0.01, 0.02), 0.05, m0)
        upload(h, d)
        if first:
            h.pair_sample(0, 2, 5, 0, draws=first)                 # another M before: the scratch it leaves changes nothing
        neg2, f2 = h.pair_sample(0, 2, 5, 0, draws=2)
        neg8, f8 = h.pair_sample(0, 2, 5, 0, draws=8)
        for ep in range(2):
            _, forced = h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, 64, 2, 5, ep, draws=8)
            assert forced == 0
        out.append((neg2, neg8, h.pair_sample(0, 2, 5, 2, draws=8)[0]) + h.get_params())
        h.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert (out[0][0] != out[0][1]).any()


# ---- 6. the pair metrics on the hardest-of-M pairs ----------------------------------------------------------------------------
def test_pair_evaluate_sampled_on_hard_negatives(oracle):
    from libfm_amd import capi
    n, k, n_neg, seed, ep = 80, 16, 2, 3, 11
    d = two_slots(n, 100, 90, 1500, 8, 900)
    q_ent, q_rp, c_ent, c_rp, q, c, ex = d
    m0 = start_model(oracle, n, k)
    h = handle(capi, n, k, True, True, (0.0, 0.0, 0.0), 0.05, m0)
    upload(h, d)
    h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, 128, n_neg, seed, 0, draws=4)
    w0, w, v = h.get_params()
    cur = model(oracle, n, k, True, True, (0.0, 0.0, 0.0), w0, w, v)
    neg, forced = h.pair_sample(0, n_neg, seed, ep, draws=4)
    assert forced == 0
    ent, rp, pa, pb = S.join_rows(q_ent, q_rp, c_ent, c_rp, q, c, neg, n_neg)
    dd = B.pair_d(cur, ent, rp, pa, pb)
    ev = h.pair_evaluate_sampled(0, n_neg, seed, ep, draws=4)
    assert ev.pairs == len(pa)
    ok = np.abs(dd) >= 1e-6
    assert abs(round(ev.accuracy * len(pa)) - (dd > 0).sum()) <= (~ok).sum()
    acc, loss = B.pair_metrics(dd)
    assert abs(ev.loss - loss) <= 1e-5 * loss
    assert h.pair_evaluate_sampled(0, n_neg, seed, ep, draws=4).loss == ev.loss
    uni = h.pair_evaluate_sampled(0, n_neg, seed, ep)
    assert uni.loss < ev.loss and uni.accuracy >= ev.accuracy      # harder negatives: a larger loss on the same interactions
    h.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(oracle):
    from libfm_amd import capi
    import ctypes as C
    n, k = 50, 4
    d = two_slots(n, 40, 30, 100, 6, 1000)
    q_ent, q_rp, c_ent, c_rp, q, c, ex = d
    m0 = start_model(oracle, n, k)
    h = handle(capi, n, k, True, True, (m0.reg0, m0.regw, m0.regv), 0.05, m0)
    upload(h, d)
    before = h.get_params()
    H, DR = capi.NEG_HARDEST, lambda M: M << 8
    for flags in (DR(4), H, H | DR(0), H | DR(17), H | DR(255), H | 1, H | 1 | DR(4), 1, H | DR(4) | (1 << 16), H | DR(4) | 4):
        assert code(capi, h.pair_epoch_sampled, 0, capi.SGD_MINIBATCH, 32, 2, 5, 0, flags=flags) == E_ARG, hex(flags)
        opts = capi.PairNegOpts(capi.SGD_SEQUENTIAL, 0, 2, flags, 5, 0)
        neg = np.full(2 * len(q), 0xDEADBEEF, dtype=np.uint32)
        forced = C.c_uint64(77)
        assert h.lib.fmx_pair_sample(h.h, 0, C.byref(opts), neg.ctypes.data_as(C.c_void_p), C.byref(forced)) == E_ARG
        assert (neg == 0xDEADBEEF).all() and forced.value == 0
        assert h.lib.fmx_pair_evaluate_sampled(h.h, 0, C.byref(opts), C.byref(capi.PairEval())) == E_ARG
    for draws in (0, 17):                                          # the wrappers pass such a count on, the library refuses it
        assert code(capi, h.pair_sample, 0, 2, 5, 0, draws=draws) == E_ARG
        assert code(capi, h.pair_evaluate_sampled, 0, 2, 5, 0, draws=draws) == E_ARG
        assert code(capi, h.pair_epoch_sampled, 0, capi.SGD_SEQUENTIAL, 0, 2, 5, 0, draws=draws) == E_ARG
    after = h.get_params()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    neg, forced = h.pair_sample(0, 2, 5, 0, draws=16)              # ... and a valid call afterwards succeeds
    ref, _ = ranking.sample_negatives(5, 0, q, c, 2, len(c_rp) - 1, ex, draws=16, **sums(m0, q_ent, q_rp, c_ent, c_rp))
    assert forced == 0 and len(neg) == 2 * len(q) and np.mean(neg == ref) > 0.9      # (real values: near ties may differ)
    st, f = h.pair_epoch_sampled(0, capi.SGD_SEQUENTIAL, 0, 2, 5, 0, flags=H | DR(16))
    assert f == 0 and st.rows == 2 * len(q)
    h.close()


# ---- 8. the query slot as its own candidate slot, and fmx_topk afterwards -------------------------------------------------------
def test_one_shared_slot_and_topk_afterwards(oracle):
    from libfm_amd import capi
    from test_gpu_topk import check_lists, dev_model, dyadic_model, dyadic_rows
    n, k, R, T_, K = 60, 8, 48, 200, 10
    ent, rp, _ = datagen.ragged_real(n, R, 5, 61, duplicates=True, empty_every=9)
    rng = np.random.default_rng(62)
    q = rng.integers(0, R, T_).astype(np.uint32)
    c = rng.integers(0, R, T_).astype(np.uint32)
    d = (ent, rp, ent, rp, q, c, exclusion_lists(rng, R, R))
    m0 = start_model(oracle, n, k)
    h, ref = hard_epochs(capi, oracle, d, n, k, 0.05, capi.SGD_MINIBATCH, 32, m0, 2, 19, qs=0, cs=0)
    check_params(h, ref, "one shared slot")
    assert h.interactions_info(0) == (0, T_)
    idx, sc = h.topk(0, 0, K)
    scores = T.scores_decomposed(dev_model(oracle, h, n, k), ent, rp, ent, rp)
    check_lists(idx, sc, scores, K)
    sel, _ = T.select(scores, 3)
    srt = -np.sort(-scores, axis=1)
    clear = (srt[:, :3] - srt[:, 1:4]).min(axis=1) > 1e-3          # queries whose first 4 scores are well apart: one possible top 3
    assert clear.sum() >= R // 4 and np.array_equal(idx[clear, :3], sel[clear])
    # ... and where every score is exact: the sampler's tables and fmx_topk's on one handle, bit for bit
    de, dr = dyadic_rows(rng, n, R, 3, dup_every=5, empty_every=7)
    w0, w, v = dyadic_model(rng, n, k)
    h.set_params(w0, w, v)
    h.upload_rows(0, de, dr, None)
    h.upload_interactions(0, 0, q, c)
    dm = model(oracle, n, k, True, True, (0.0, 0.0, 0.0), w0, w, v)
    neg, forced = h.pair_sample(0, 2, 3, 1, draws=4)
    want, want_forced = ranking.sample_negatives(3, 1, q, c, 2, R, None, draws=4, **sums(dm, de, dr, de, dr))
    assert forced == want_forced == 0 and np.array_equal(neg, want)
    idx, sc = h.topk(0, 0, K)
    sel, sel_sc = T.select(T.scores_decomposed(dm, de, dr, de, dr), K)
    assert np.array_equal(idx, sel) and np.array_equal(sc, sel_sc)
    h.close()


# ---- 9. the command line ----------------------------------------------------------------------------------------------------------
def test_cli_neg_draws(tmp_path, oracle, capsys):
    from libfm_amd import cli
    from libfm_amd import data as D
    from libfm_amd import learner as L
    from libfm_amd import refrand as R
    nu, ni, k, seed = 40, 30, 4, 7
    rng = np.random.default_rng(5)
    q_ent, q_rp, q_y = datagen._pack([[u] for u in range(nu)], [[1.0]] * nu, [0.0] * nu)
    c_ent, c_rp, c_y = datagen._pack([[nu + i] for i in range(ni)], [[1.0]] * ni, [0.0] * ni)
    tq, tc = rng.integers(0, nu, 300), rng.integers(0, ni, 300)
    f = {x: str(tmp_path / x) for x in ("q", "c", "tr", "m_cli", "m_py")}
    oracle.Data(q_ent, q_rp, q_y).write_libsvm(f["q"])
    oracle.Data(c_ent, c_rp, c_y).write_libsvm(f["c"])
    with open(f["tr"], "w") as fh:
        fh.write("".join("%d %d\n" % (x, z) for x, z in zip(tq, tc)))
    common = ["-train", f["q"], "-test", f["q"], "-candidates", f["c"], "-dim", "0,1,%d" % k, "-iter", "2", "-learn_rate", "0.05",
              "-regular", "0,0,0.002", "-init_stdev", "0.1", "-seed", str(seed)]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(["-method", "bpr", "-interactions", f["tr"], "-neg", "2", "-neg_draws", "4", "-gpu_mode", "minibatch",
                         "-batch", "64", "-save_model", f["m_cli"]] + common) == 0
    text = buf.getvalue()
    assert "interactions=300\ttest_interactions=0\tneg=2\tneg_draws=4" in text, text[-2000:]
    assert len([ln for ln in text.splitlines() if ln.startswith("#Iter=")]) == 2
    # the same run from Python
    train, cand = L.Data(*D.load(f["q"])), L.Data(*D.load(f["c"]))
    fm = L.FMModel()
    fm.num_attribute = max(train.num_feature, cand.num_feature)
    fm.k0, fm.k1, fm.num_factor, fm.init_stdev = False, True, k, 0.1
    R.srand(seed)
    fm.w0, fm.w = 0.0, np.zeros(fm.num_attribute)
    fm.v = R.init_v(fm.num_factor, fm.num_attribute, fm.init_mean, fm.init_stdev)
    fm.reg0, fm.regw, fm.regv = 0.0, 0.0, 0.002
    l = L.FMLearnPairSGD()
    l.learn_rate, l.mode, l.batch = 0.05, "minibatch", 64
    l.fm, l.num_iter, l.task = fm, 2, 0
    l.min_target, l.max_target = train.min_target, train.max_target
    l.device = -1
    l.out = io.StringIO()
    l.init()
    l.learn_implicit(train, cand, (tq.astype(np.uint32), tc.astype(np.uint32)), None, n_neg=2, seed=seed, neg_draws=4)
    assert [row["neg_draws"] for row in l.log] == [4, 4]
    fm.save_model(f["m_py"])
    l.close()
    assert open(f["m_cli"]).read() == open(f["m_py"]).read()
    # uniform negatives train another model: the flag reached the device
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(["-method", "bpr", "-interactions", f["tr"], "-neg", "2", "-gpu_mode", "minibatch", "-batch", "64",
                         "-save_model", f["m_py"]] + common) == 0
    assert "neg_draws=1" in buf.getvalue() and open(f["m_cli"]).read() != open(f["m_py"]).read()
    # -neg_draws outside -method bpr -interactions: the error of a misplaced -neg
    capsys.readouterr()
    assert cli.main(["-method", "sgd", "-task", "r", "-neg_draws", "4"] + common) == 0
    assert "ERROR: -interactions, -test_interactions, -neg and -neg_draws belong to -method bpr with -interactions" in capsys.readouterr().err
    assert cli.main(["-method", "bpr", "-interactions", f["tr"], "-neg_draws", "17"] + common) == 0
    assert "ERROR: -neg_draws needs 1 .. 16" in capsys.readouterr().err
