"""GPU: BPR on query x candidate interactions with negatives drawn on the device -- fmx_upload_interactions / fmx_pair_sample /
fmx_pair_epoch_sampled / fmx_pair_evaluate_sampled (include/fmx.h).

The sampler against ranking.sample_negatives (exact), both modes against tests/bpr_oracle.py on the materialised joined rows
(tests/bpr_sampled_oracle.py) and against fmx_pair_epoch on the device, determinism, the pair metrics, refusals, a forced case
and the command line.  Tolerances as tests/test_gpu_bpr.py: |gpu - ref| <= 1e-4 |ref| + 1e-5 on w and V, w0 to 1e-12 relative.
Except in the forced case every exclusion list holds at most a quarter of a catalogue of at least 8 rows, so a forced draw has
probability below (1/4 + 1/8)^16 < 2e-7 per pair, and every test asserts forced == 0."""
import contextlib
import io

import numpy as np
import pytest

import bpr_oracle as B
import bpr_sampled_oracle as S
import datagen
from libfm_amd import ranking
from test_gpu_bpr import check_params, close, handle, model, start_model

pytestmark = pytest.mark.gpu


def exclusion_lists(rng, Q, C):
    """per query at most C / 4 distinct candidate rows, unsorted, some repeated"""
    ex = []
    for _ in range(Q):
        m = int(rng.integers(0, C // 4 + 1))
        e = rng.choice(C, m, replace=False).astype(np.uint32)
        ex.append(np.concatenate([e, e[: m // 3]])[rng.permutation(m + m // 3)] if m else e)
    return ex


def two_slots(n, Q, C, T, max_nnz, seed, empty_every=0):
    """ragged query and candidate rows over ONE feature space (ids shared between a query and a candidate row, ids repeated
    inside a row, optionally empty rows), T interactions and exclusion lists"""
    q_ent, q_rp, _ = datagen.ragged_real(n, Q, max_nnz, seed, duplicates=True, empty_every=empty_every)
    c_ent, c_rp, _ = datagen.ragged_real(n, C, max_nnz, seed + 1, duplicates=True, empty_every=empty_every)
    rng = np.random.default_rng(seed + 2)
    q = rng.integers(0, Q, T).astype(np.uint32)
    c = rng.integers(0, C, T).astype(np.uint32)
    return q_ent, q_rp, c_ent, c_rp, q, c, exclusion_lists(rng, Q, C)


def upload(h, d, exclude=True, qs=0, cs=1):
    q_ent, q_rp, c_ent, c_rp, q, c, ex = d
    h.upload_rows(qs, q_ent, q_rp, None)
    h.upload_rows(cs, c_ent, c_rp, None)
    h.upload_interactions(qs, cs, q, c, ex if exclude else None)


def code(capi, fn, *a, **kw):
    with pytest.raises(capi.FmxError) as e:
        fn(*a, **kw)
    return e.value.code


# ---- 1. the sampler: device == specification ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 9, 50, 1000, 100000])
@pytest.mark.parametrize("n_neg", [1, 4])
def test_sampler_matches_the_specification(C, n_neg):
    from libfm_amd import capi
    Q, T = 37, 5000
    rng = np.random.default_rng(C + n_neg)
    ent, rp, _ = datagen._pack([[0]] * max(Q, 1), [[1.0]] * max(Q, 1), [0.0] * max(Q, 1))
    c_ent, c_rp, _ = datagen._pack([[1]] * C, [[1.0]] * C, [0.0] * C)
    q = rng.integers(0, Q, T).astype(np.uint32)
    c = rng.integers(0, C, T).astype(np.uint32)
    ex = exclusion_lists(rng, Q, C)
    h = capi.Handle(2, 2, True, True, capi.TASK_REGRESSION, 0, 0, 0, 0.01, 0.0, 1.0, device=0)
    h.upload_rows(0, ent, rp, None)
    h.upload_rows(1, c_ent, c_rp, None)
    for lists in (ex, None):
        h.upload_interactions(0, 1, q, c, lists)
        for seed, epoch in ((0, 0), (7, 1), ((1 << 64) - 1, (1 << 40) + 5), (123456789, 3)):
            ref, ref_forced = ranking.sample_negatives(seed, epoch, q, c, n_neg, C, lists)
            assert ref_forced == 0
            neg, forced = h.pair_sample(0, n_neg, seed, epoch)
            assert forced == 0 and neg.dtype == np.uint32
            assert np.array_equal(neg, ref), (C, n_neg, seed, epoch, int((neg != ref).sum()))
    h.close()


def test_sampler_one_candidate_and_query_slot_equal_to_candidate_slot():
    """C = 1: the only candidate is the positive, so every pair is forced to it (the specification says the same); and
    query_slot == cand_slot is allowed"""
    from libfm_amd import capi
    ent, rp, _ = datagen._pack([[0]], [[1.0]], [0.0])
    h = capi.Handle(2, 2, True, True, capi.TASK_REGRESSION, 0, 0, 0, 0.01, 0.0, 1.0, device=0)
    h.upload_rows(0, ent, rp, None)
    h.upload_interactions(0, 0, np.zeros(5, np.uint32), np.zeros(5, np.uint32))
    neg, forced = h.pair_sample(0, 2, 3, 2)
    ref, ref_forced = ranking.sample_negatives(3, 2, np.zeros(5, int), np.zeros(5, int), 2, 1)
    assert forced == ref_forced == 10 and np.array_equal(neg, ref)
    h.close()


# ---- 8. a forced case -------------------------------------------------------------------------------------------------
def test_forced_draws_match_the_specification():
    from libfm_amd import capi
    n, k, Q, C, T = 30, 4, 6, 12, 400
    d = two_slots(n, Q, C, T, 5, 301)
    q_ent, q_rp, c_ent, c_rp, q, c, ex = d
    ex[2] = np.arange(C, dtype=np.uint32)[::-1]                # query 2 excludes the whole catalogue
    assert (q == 2).sum() > 0
    h = capi.Handle(n, k, True, True, capi.TASK_REGRESSION, 0, 0, 0, 0.01, 0.0, 1.0, device=0)
    upload(h, d)
    for n_neg in (1, 3):
        ref, ref_forced = ranking.sample_negatives(5, 9, q, c, n_neg, C, ex)
        neg, forced = h.pair_sample(0, n_neg, 5, 9)
        assert ref_forced == int((q == 2).sum()) * n_neg
        assert forced == ref_forced and np.array_equal(neg, ref)
    _, forced = h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, 32, 3, 5, 9)
    assert forced == ref_forced
    h.close()


# ---- 2. / 3. both modes against the oracle on the materialised joined rows --------------------------------------------------
def run_both(capi, O, d, k, lr, mode, batch, n, m0, n_neg, seed, epochs=2, exclude=True):
    h = handle(capi, n, k, m0.k0, m0.k1, (m0.reg0, m0.regw, m0.regv), lr, m0)
    upload(h, d, exclude)
    q_ent, q_rp, c_ent, c_rp, q, c, ex = d
    ref = m0.copy()
    P = len(q) * n_neg
    for ep in range(epochs):
        st, forced = h.pair_epoch_sampled(0, mode, batch, n_neg, seed, ep)
        ref_forced = S.epoch(ref, q_ent, q_rp, c_ent, c_rp, q, c, n_neg, seed, ep, lr,
                             None if mode == capi.SGD_SEQUENTIAL else batch, ex if exclude else None)
        assert forced == 0 and ref_forced == 0
        assert st.rows == P
        if mode == capi.SGD_SEQUENTIAL:
            assert st.batches == P
        else:
            assert st.batch_used == batch and st.batches == (P + batch - 1) // batch and st.max_feature_count >= 1
        assert st.setup_seconds > 0 and st.device_seconds > 0
    return h, ref


@pytest.mark.parametrize("k", [1, 5, 64, 128, 1000])
def test_sequential_matches_the_loop(k, oracle):
    """ragged rows, empty query and candidate rows, ids shared between the query and the candidate row and repeated inside a
    row, two epochs with epoch = 0, 1"""
    from libfm_amd import capi
    n, lr = 40, 0.05
    T = 40 if k >= 128 else 120
    d = two_slots(n, 30, 24, T, 6, 400 + k, empty_every=7)
    q, c = d[4], d[5]
    q[3], c[3] = 6, 6                                          # an empty query row with an empty candidate row (empty_every = 7)
    q[4] = 13                                                  # an empty query row
    c[5] = 20                                                  # an empty candidate row
    m0 = start_model(oracle, n, k, seed=k)
    for n_neg in (1, 2):
        h, ref = run_both(capi, oracle, d, k, lr, capi.SGD_SEQUENTIAL, 1, n, m0, n_neg, 17)
        check_params(h, ref, "sequential k %d n_neg %d" % (k, n_neg))
        h.close()


@pytest.mark.parametrize("batch", [1, 7, 64, 600])
def test_minibatch_matches_the_batch_rule(batch, oracle):
    from libfm_amd import capi
    n, k, lr = 50, 8, 0.05
    d = two_slots(n, 60, 40, 250, 7, 500, empty_every=11)
    m0 = start_model(oracle, n, k)
    h, ref = run_both(capi, oracle, d, k, lr, capi.SGD_MINIBATCH, batch, n, m0, 2, 23)
    check_params(h, ref, "batch %d" % batch)
    h.close()


@pytest.mark.parametrize("k", [1, 5, 64, 128, 1000])
def test_minibatch_edge_cases(k, oracle):
    from libfm_amd import capi
    n, lr = 40, 0.05
    d = two_slots(n, 30, 24, 40 if k >= 128 else 120, 6, 600 + k, empty_every=7)
    d[4][3], d[5][3] = 6, 6
    m0 = start_model(oracle, n, k, seed=k)
    h, ref = run_both(capi, oracle, d, k, lr, capi.SGD_MINIBATCH, 7, n, m0, 1, 29, exclude=False)
    check_params(h, ref, "minibatch k %d" % k)
    h.close()


def test_a_query_feature_in_every_pair_of_a_4096_batch(oracle):
    from libfm_amd import capi
    n, k, lr, T = 400, 8, 0.001, 4096
    rng = np.random.default_rng(71)
    q_ids = [[0] + rng.integers(1, n, 2).tolist() for _ in range(300)]            # feature 0 in every query row
    q_val = [[1.0] + rng.uniform(-1, 1, 2).round(3).tolist() for _ in range(300)]
    c_ids = [rng.integers(1, n, 2).tolist() for _ in range(200)]
    c_val = [rng.uniform(-1, 1, 2).round(3).tolist() for _ in range(200)]
    q_ent, q_rp, _ = datagen._pack(q_ids, q_val, [0.0] * 300)
    c_ent, c_rp, _ = datagen._pack(c_ids, c_val, [0.0] * 200)
    q = rng.integers(0, 300, T).astype(np.uint32)
    c = rng.integers(0, 200, T).astype(np.uint32)
    d = (q_ent, q_rp, c_ent, c_rp, q, c, exclusion_lists(rng, 300, 200))
    m0 = start_model(oracle, n, k)
    h, ref = run_both(capi, oracle, d, k, lr, capi.SGD_MINIBATCH, T, n, m0, 1, 31, epochs=1)
    check_params(h, ref, "4096-pair batch")
    st, _ = h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, T, 1, 31, 1)
    assert st.max_feature_count == T                           # feature 0: ONE entry per pair (the query's entries are not doubled)
    h.close()


# ---- 4. the new path against the old path on the device ---------------------------------------------------------------------
@pytest.mark.parametrize("mode,batch", [("seq", 1), ("mb", 64)])
def test_sampled_epoch_equals_pair_epoch_on_the_joined_rows(mode, batch, oracle):
    from libfm_amd import capi
    n, k, lr, n_neg, seed = 300, 64, 0.05, 2, 41
    d = two_slots(n, 200, 150, 1500, 10, 700, empty_every=13)
    q_ent, q_rp, c_ent, c_rp, q, c, ex = d
    m0 = start_model(oracle, n, k)
    gmode = capi.SGD_SEQUENTIAL if mode == "seq" else capi.SGD_MINIBATCH
    new = handle(capi, n, k, True, True, (0.01, 0.01, 0.02), lr, m0)
    old = handle(capi, n, k, True, True, (0.01, 0.01, 0.02), lr, m0)
    upload(new, d)
    for ep in range(2):
        ent, rp, pa, pb, neg, forced = S.epoch_pairs(q_ent, q_rp, c_ent, c_rp, q, c, n_neg, seed, ep, ex)
        assert forced == 0
        old.upload_rows(2, ent, rp, None)                      # the join, materialised in a third slot
        old.upload_pairs(2, pa, pb)
        old.pair_epoch(2, gmode, batch)
        _, f = new.pair_epoch_sampled(0, gmode, batch, n_neg, seed, ep)
        assert f == 0
    w0o, wo, vo = old.get_params()
    w0n, wn, vn = new.get_params()
    close(wn, wo, mode + " w")
    close(vn, vo, mode + " v")
    assert abs(w0n - w0o) <= 1e-12 * abs(w0o)
    old.close()
    new.close()


# ---- 5. determinism -----------------------------------------------------------------------------------------------------
def test_minibatch_is_bit_reproducible(oracle):
    from libfm_amd import capi
    n, k, lr = 300, 64, 0.05
    d = two_slots(n, 400, 300, 3000, 12, 800)
    m0 = start_model(oracle, n, k)
    out = []
    for _ in range(2):
        h = handle(capi, n, k, True, True, (0.0, 0.01, 0.02), lr, m0)
        upload(h, d)
        for ep in range(2):
            _, forced = h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, 64, 2, 5, ep)
            assert forced == 0
        out.append(h.get_params())
        h.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


# ---- 6. the pair metrics --------------------------------------------------------------------------------------------------
def test_pair_evaluate_sampled_matches_numpy(oracle):
    from libfm_amd import capi
    n, k, n_neg, seed, ep = 80, 16, 2, 3, 11
    d = two_slots(n, 100, 90, 1500, 8, 900)
    q_ent, q_rp, c_ent, c_rp, q, c, ex = d
    m0 = start_model(oracle, n, k)
    h = handle(capi, n, k, True, True, (0.0, 0.0, 0.0), 0.05, m0)
    upload(h, d)
    h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, 128, n_neg, seed, 0)
    w0, w, v = h.get_params()
    cur = model(oracle, n, k, True, True, (0.0, 0.0, 0.0), w0, w, v)
    ent, rp, pa, pb, _, forced = S.epoch_pairs(q_ent, q_rp, c_ent, c_rp, q, c, n_neg, seed, ep, ex)
    assert forced == 0
    dd = B.pair_d(cur, ent, rp, pa, pb)
    ev = h.pair_evaluate_sampled(0, n_neg, seed, ep)
    assert ev.pairs == len(pa)
    ok = np.abs(dd) >= 1e-6
    assert abs(round(ev.accuracy * len(pa)) - (dd > 0).sum()) <= (~ok).sum()      # (the count is an integer: accuracy * P rounds to it)
    acc, loss = B.pair_metrics(dd)
    assert abs(ev.loss - loss) <= 1e-5 * loss
    assert h.pair_evaluate_sampled(0, n_neg, seed, ep).loss == ev.loss     # a fixed-order reduction
    assert h.pair_evaluate_sampled(0, n_neg, seed, ep + 1).loss != ev.loss  # another epoch: other negatives
    h.close()


# ---- 7. refusals and invalidation -------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(oracle):
    from libfm_amd import capi
    import ctypes as C
    n, k, lr = 50, 4, 0.05
    d = two_slots(n, 40, 30, 100, 6, 1000)
    q_ent, q_rp, c_ent, c_rp, q, c, ex = d
    m0 = start_model(oracle, n, k)
    h = handle(capi, n, k, True, True, (m0.reg0, m0.regw, m0.regv), lr, m0)
    y = np.zeros(len(q_rp) - 1, np.float32)
    h.upload_rows(0, q_ent, q_rp, y)
    h.upload_rows(1, c_ent, c_rp, None)
    E_ARG, E_STATE, E_UNSUPPORTED = -1, -3, -4
    assert code(capi, h.pair_epoch_sampled, 0) == E_STATE                  # no interactions yet
    assert code(capi, h.pair_evaluate_sampled, 0) == E_STATE
    assert code(capi, h.pair_sample, 0) == E_STATE
    bad = c.copy()
    bad[7] = len(c_rp) - 1                                                  # a candidate row outside its slot: nothing changes
    assert code(capi, h.upload_interactions, 0, 1, q, bad, ex) == E_ARG
    badq = q.copy()
    badq[3] = len(q_rp) - 1
    assert code(capi, h.upload_interactions, 0, 1, badq, c, ex) == E_ARG
    bad_ex = [e.copy() for e in ex]
    bad_ex[1] = np.array([len(c_rp) - 1], np.uint32)
    assert code(capi, h.upload_interactions, 0, 1, q, c, bad_ex) == E_ARG
    assert code(capi, h.upload_interactions, 0, 5, q, c) == E_STATE         # a slot without rows
    assert code(capi, h.pair_epoch_sampled, 0) == E_STATE
    assert code(capi, h.interactions_info, 0) == E_STATE
    h.upload_interactions(0, 1, q, c, ex)
    assert h.interactions_info(0) == (1, len(q))
    assert code(capi, h.pair_epoch_sampled, 0, capi.SGD_HOGWILD) == E_UNSUPPORTED
    assert code(capi, h.pair_epoch_sampled, 0, n_neg=0) == E_ARG
    assert code(capi, h.pair_sample, 0, 0) == E_ARG
    assert code(capi, h.pair_evaluate_sampled, 0, 0) == E_ARG
    assert code(capi, h.pair_epoch_sampled, 0, flags=1) == E_ARG
    assert h.lib.fmx_pair_epoch_sampled(h.h, 0, None, None, None) == E_ARG   # NULL opts
    assert h.lib.fmx_pair_sample(h.h, 0, None, None, None) == E_ARG
    assert h.lib.fmx_pair_evaluate_sampled(h.h, 0, None, C.byref(capi.PairEval())) == E_ARG
    h.als_begin(0)
    assert code(capi, h.pair_epoch_sampled, 0, capi.SGD_MINIBATCH) == E_STATE   # open ALS session on the query slot
    h.als_end()
    h.upload_rows(3, q_ent, q_rp, y)
    h.upload_interactions(1, 3, c[:10] * 0, q[:10])                          # ... and on the candidate slot of interactions
    h.als_begin(3)
    assert code(capi, h.pair_epoch_sampled, 1) == E_STATE
    h.als_end()
    h.free_rows(3)
    h.sgda_begin()
    assert code(capi, h.pair_epoch_sampled, 0) == E_STATE                   # open SGDA session
    h.sgda_end()
    h.set_params(m0.w0, m0.w, m0.v)
    blk_ent = np.zeros(1, dtype=q_ent.dtype)
    blk_ent["id"], blk_ent["value"] = 0, 1.0
    blocks = [(blk_ent, np.array([0, 1], np.uint64), np.zeros(len(q_rp) - 1, np.uint32), n - 1)]
    h.upload_block_rows(2, q_ent, q_rp, y, blocks, keep=True)
    h.upload_interactions(2, 1, q, c, ex)
    assert code(capi, h.pair_epoch_sampled, 2) == E_UNSUPPORTED              # kept -relation blocks on the query slot
    h.upload_interactions(1, 2, c[:10], q[:10])
    assert code(capi, h.pair_epoch_sampled, 1) == E_UNSUPPORTED              # ... on the candidate slot
    h.free_rows(2)
    assert code(capi, h.pair_epoch_sampled, 1) == E_STATE                    # freeing the candidate slot dropped them
    # an empty candidate slot: no interaction can name a row of it
    h.upload_rows(4, np.zeros(0, dtype=q_ent.dtype), np.zeros(1, np.uint64), None)
    assert code(capi, h.upload_interactions, 0, 4, q, c) == E_ARG
    # uploads into either slot drop the interactions
    h.upload_rows(1, c_ent, c_rp, None)
    assert code(capi, h.pair_epoch_sampled, 0) == E_STATE
    h.upload_interactions(0, 1, q, c, ex)
    h.upload_rows(0, q_ent, q_rp, y)
    assert code(capi, h.pair_sample, 0) == E_STATE
    h.upload_interactions(0, 1, q, c, ex)
    h.free_rows(1)
    assert code(capi, h.pair_evaluate_sampled, 0) == E_STATE
    h.upload_rows(1, c_ent, c_rp, None)
    h.upload_interactions(0, 1, q[:5], c[:5])
    h.upload_interactions(0, 1, q, c, ex)                                    # a new call replaces the old interactions
    ref = m0.copy()
    st, forced = h.pair_epoch_sampled(0, capi.SGD_SEQUENTIAL, n_neg=2, seed=9, epoch=4)   # ... and the handle still trains
    assert forced == 0 and st.rows == 2 * len(q)
    assert S.epoch(ref, q_ent, q_rp, c_ent, c_rp, q, c, 2, 9, 4, lr, None, ex) == 0
    check_params(h, ref, "after refusals")
    h.upload_interactions(0, 1, q[:0], c[:0])                                # no interactions: an epoch of nothing
    st, forced = h.pair_epoch_sampled(0, capi.SGD_MINIBATCH)
    assert st.rows == 0 and forced == 0
    check_params(h, ref, "empty epoch")
    h.close()
    s = capi.Handle(n, k, True, True, capi.TASK_REGRESSION, 0.0, 0.01, 0.01, lr, 1.0, 5.0, device=0, shard_rank=0, shard_world=2)
    s.set_params(m0.w0, m0.w, m0.v)
    s.upload_rows(0, q_ent, q_rp, y)
    s.upload_rows(1, c_ent, c_rp, None)
    s.upload_interactions(0, 1, q, c, ex)
    assert code(capi, s.pair_epoch_sampled, 0) == E_UNSUPPORTED              # feature shard
    assert code(capi, s.pair_evaluate_sampled, 0) == E_UNSUPPORTED
    assert code(capi, s.pair_sample, 0) == E_UNSUPPORTED
    s.close()


def test_sequential_pairs_longer_than_the_lds(oracle):
    """joined pairs of more than 2048 entries are staged in a global buffer instead of LDS"""
    from libfm_amd import capi
    n, k, lr = 3000, 8, 0.01
    rng = np.random.default_rng(121)
    mk = lambda rows, m: datagen._pack([rng.choice(n, m, replace=False).tolist() for _ in range(rows)],
                                       [rng.uniform(-1, 1, m).round(3).tolist() for _ in range(rows)], [0.0] * rows)
    q_ent, q_rp, _ = mk(4, 600)
    c_ent, c_rp, _ = mk(8, 700)
    q, c = np.array([0, 1, 2, 3, 1], np.uint32), np.array([0, 3, 5, 7, 2], np.uint32)
    d = (q_ent, q_rp, c_ent, c_rp, q, c, None)
    m0 = start_model(oracle, n, k)
    h, ref = run_both(capi, oracle, d, k, lr, capi.SGD_SEQUENTIAL, 1, n, m0, 1, 3, exclude=False)
    check_params(h, ref, "long rows")
    h.close()


# ---- 9. end to end through the command line ---------------------------------------------------------------------------------
def test_cli_implicit_feedback_end_to_end(tmp_path, oracle, capsys):
    """Users as query rows, items as candidate rows (movielens_shaped's ids: user u = feature u, item i = feature n_users + i),
    a user's interactions = its top items under a planted model with factors only (no item bias, so popularity
    carries little signal), 20 % held out.  recall@10 of recommend() on the held-out items, the training interactions excluded, for
    the trained model, the untrained model and a popularity ranking, next to the chance level 10 / (eligible candidates): the
    test prints the four figures; DESIGN.md section 12 records a run."""
    from libfm_amd import cli
    nu, ni, top, K = 200, 100, 15, 10
    rng = np.random.default_rng(5)
    pu, qi = rng.normal(0, 1.0, (nu, 4)), rng.normal(0, 1.0, (ni, 4))
    liked = np.argsort(-(pu @ qi.T), axis=1)[:, :top]                       # [nu][top]
    held = np.zeros((nu, top), bool)
    for u in range(nu):
        held[u, rng.choice(top, top // 5, replace=False)] = True            # 20 % held out
    users = np.repeat(np.arange(nu), top).reshape(nu, top)
    tr_q, tr_c = users[~held], liked[~held]
    te_q, te_c = users[held], liked[held]
    order = rng.permutation(len(tr_q))
    tr_q, tr_c = tr_q[order], tr_c[order]
    q_ent, q_rp, q_y = datagen._pack([[u] for u in range(nu)], [[1.0]] * nu, [0.0] * nu)
    c_ent, c_rp, c_y = datagen._pack([[nu + i] for i in range(ni)], [[1.0]] * ni, [0.0] * ni)
    f = {x: str(tmp_path / x) for x in ("q", "c", "tr", "te", "topk0", "topk1")}
    oracle.Data(q_ent, q_rp, q_y).write_libsvm(f["q"])
    oracle.Data(c_ent, c_rp, c_y).write_libsvm(f["c"])
    for name, (a, b) in (("tr", (tr_q, tr_c)), ("te", (te_q, te_c))):
        with open(f[name], "w") as fh:
            fh.write("".join("%d %d\n" % (x, z) for x, z in zip(a, b)))
    rel_ptr = np.concatenate([[0], np.cumsum(np.bincount(te_q, minlength=nu))])
    rel_idx = te_c[np.argsort(te_q, kind="stable")]

    def recall(iters, out):
        argv = ["-method", "bpr", "-train", f["q"], "-test", f["q"], "-candidates", f["c"], "-interactions", f["tr"],
                "-test_interactions", f["te"], "-neg", "4", "-dim", "0,1,8", "-iter", str(iters), "-learn_rate", "0.05",
                "-regular", "0,0,0.002", "-init_stdev", "0.1", "-seed", "7", "-gpu_mode", "minibatch", "-batch", "64",
                "-topk", str(K), "-exclude", f["tr"], "-topk_out", out]
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            assert cli.main(argv) == 0
        lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("#Iter=")]
        assert len(lines) == iters, buf.getvalue()[-2000:]
        final = [ln for ln in buf.getvalue().splitlines() if ln.startswith("Final")]
        assert len(final) == 1 and 0.0 < float(final[0].split("\t")[1].split("=")[1]) <= 1.0, final   # evaluated, also at -iter 0
        if iters:
            assert final[0].split("\t")[1:] == lines[-1].split("\t")[1:]                                # ... on the same fixed epoch
        idx = np.full((nu, K), 0xFFFFFFFF, dtype=np.int64)
        with open(out) as fh:
            for u, line in enumerate(fh):
                got = [int(t.split(":")[0]) for t in line.split()]
                idx[u, :len(got)] = got
        for u in range(nu):                                                   # recommend() excluded the training interactions
            assert not set(idx[u]) & set(tr_c[tr_q == u])
        return ranking.metrics(idx, rel_ptr, rel_idx)["recall"], lines + final

    untrained, _ = recall(0, f["topk0"])
    trained, lines = recall(20, f["topk1"])
    # popularity: the most frequent training items a user has not interacted with (reported, not asserted)
    pop = np.argsort(-np.bincount(tr_c, minlength=ni), kind="stable")
    pidx = np.array([[i for i in pop if i not in set(tr_c[tr_q == u])][:K] for u in range(nu)])
    popularity = ranking.metrics(pidx, rel_ptr, rel_idx)["recall"]
    chance = K / (ni - (top - top // 5))
    with capsys.disabled():
        print("\nrecall@%d: trained %.4f untrained %.4f popularity %.4f chance %.4f | %s" % (K, trained, untrained, popularity, chance, lines[-1]))
    assert trained > untrained
    assert trained > chance
