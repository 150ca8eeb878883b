"""GPU: fmx_evaluate_rank and its group form -- exact tie-averaged NDCG, recall and precision at K inside every query, reduced on
the device (include/fmx.h).

The oracle is libfm_amd.evalmetrics.rank_metrics applied to THE DEVICE'S OWN fmx_predict output of the same slot and parameters,
with the library's discount table (fmx_rank_discounts).  Every integer field is compared with ==, `by_query` field for field
with Handle.evaluate_by_query on the same handle, hits_q with == wherever no tie run of the query straddles the cutoff (every term
is then an integer), dcg_q and the other hits_q within the forward bound of a sum of T = min(rows_q, K) non-negative fp64 terms
(term_bound), hits and the three means within mean_bound.  The shapes are those of tests/test_gpu_query_eval.py, whose builders
this file uses: n = 50 features, k = 2 (one case at k = 0, one at k = 17), 1 .. 3 entries per row."""
import ctypes as C
import math

import numpy as np
import pytest

from libfm_amd.evalmetrics import rank_metrics, rank_runs
from test_gpu_query_eval import (INT_FIELDS, K, LAYOUTS, LINKS, MEANS, N, POOLED_FIELDS, ROW_COUNTS, _learner, _relational, _separable,
                                 _write_libfm, handle, make_params, make_queries, make_rows, same)

pytestmark = pytest.mark.gpu

CUTOFFS = (1, 10, 64, 65)
AT_FIELDS = ("ndcg", "recall", "precision")


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


@pytest.fixture(scope="module")
def hc(capi):
    h = handle(capi)
    yield h
    h.close()


def term_bound(want, terms):
    """|device - oracle| allowed for a query's dcg_q or hits_q: the device adds at most T = `terms` non-negative fp64 terms (one per
    tie run that begins above the cutoff) lane by lane and through the butterfly; the forward error of such a sum is at most
    (T - 1) u |sum| with u = 2^-53 whatever the order; the terms have the same bits on both sides, the oracle's sum (math.fsum) is
    correctly rounded; the factor 2 and the + 4 are slack as in test_gpu_query_eval.mean_bound"""
    return np.abs(want) * (terms + 4) * 2.0 ** -53 * 2


def mean_bound(want, relevant, k):
    """... for hits and the three means of a cutoff: R = `relevant` non-negative per-query terms, each carrying its own relative
    error of at most about K u (term_bound, one division more), summed in a fixed order and divided once"""
    return abs(want) * (relevant + k + 8) * 2.0 ** -53 * 2


def straddled(p, y, qid, cutoffs):
    """{(query, cutoff index)} where some tie run [a, b) of the query has a < K < b"""
    members = {}
    for i, g in enumerate(qid):
        members.setdefault(int(g), []).append(i)
    out = set()
    for g, rows in members.items():
        runs = rank_runs([float(p[i]) for i in rows], [y[i] >= 0 for i in rows])
        out |= {(g, j) for j, k in enumerate(cutoffs) for a, b, _ in runs if a < k < b}
    return out


def bytes_outside_the_times(capi, ev):
    b = bytearray(bytes(ev))
    q, x = capi.EvalRank.by_query.offset, capi.EvalRank.by_query.offset + capi.EvalQuery.pooled.offset
    for off in (capi.EvalRank.device_seconds.offset, capi.EvalRank.topk_seconds.offset, q + capi.EvalQuery.device_seconds.offset,
                q + capi.EvalQuery.rank_seconds.offset, x + capi.EvalEx.device_seconds.offset, x + capi.EvalEx.rank_seconds.offset):
        b[off:off + 8] = bytes(8)
    return bytes(b)


def check_struct(ev, want, bq, cutoffs):
    for f in INT_FIELDS:
        assert getattr(ev.by_query, f) == getattr(bq, f) == want["by_query"][f], f
    for f in MEANS:
        assert same(getattr(ev.by_query, f), getattr(bq, f)), f
    for f in POOLED_FIELDS:
        assert same(getattr(ev.by_query.pooled, f), getattr(bq.pooled, f)), f
    R = want["relevant_queries"]
    assert (ev.relevant_queries, ev.n_cutoffs, ev.reserved) == (R, len(cutoffs), 0)
    for j, k in enumerate(cutoffs):
        at, w = ev.at[j], want["at"][j]
        print("K", k, "R", R, "tied", at.tied_queries, "hits", at.hits, w["hits"], *[x for f in AT_FIELDS for x in (getattr(at, f), w[f])])
        assert (at.k, at.reserved, at.tied_queries) == (k, 0, w["tied_queries"])
        if R == 0:
            assert at.hits == 0.0 and all(math.isnan(getattr(at, f)) for f in AT_FIELDS)
            continue
        assert abs(at.hits - w["hits"]) <= mean_bound(w["hits"], R, k)
        for f in AT_FIELDS:
            assert abs(getattr(at, f) - w[f]) <= mean_bound(w[f], R, k), f
    for j in range(len(cutoffs), 4):
        assert bytes(ev.at[j]) == bytes(48)
    sorted_ = bq.rank_seconds > 0.0
    assert (ev.device_seconds >= ev.topk_seconds > 0.0) if sorted_ else ev.topk_seconds == 0.0


def check_against_oracle(capi, h, slot, rows, y, qid, nq, cutoffs=CUTOFFS, links=("logistic",), per_query=True):
    p = h.predict(slot, rows)
    D = capi.rank_discounts(max(cutoffs))
    out = None
    for link in links:
        want = rank_metrics(p, y, qid, nq, cutoffs, link, discounts=D, per_query=per_query)
        if per_query:
            ev, dcg, hits = h.evaluate_rank(slot, cutoffs, LINKS[link], per_query=True)
            assert dcg.dtype == hits.dtype == np.float64 and dcg.shape == hits.shape == (nq, len(cutoffs))
            wd, wh = np.asarray(want["dcg_q"]).reshape(nq, len(cutoffs)), np.asarray(want["hits_q"]).reshape(nq, len(cutoffs))
            if want["by_query"]["pooled"]["nan_rows"]:
                assert not dcg.any() and not hits.any()
            else:
                size = np.bincount(np.asarray(qid, dtype=np.int64), minlength=nq)
                T = np.minimum(size[:, None], np.asarray(cutoffs)[None, :])
                assert np.all(np.abs(dcg - wd) <= term_bound(wd, T))                                # every cell
                assert np.all(np.abs(hits - wh) <= term_bound(wh, T))
                exact = np.ones(hits.shape, dtype=bool)
                for g, j in straddled(p, y, qid, cutoffs):
                    exact[g, j] = False
                assert np.array_equal(hits[exact], wh[exact])
                print("cells", hits.size, "straddled", int((~exact).sum()), "dcg cells off by a rounding", int((dcg != wd).sum()))
        else:
            ev = h.evaluate_rank(slot, cutoffs, LINKS[link])
        check_struct(ev, want, h.evaluate_by_query(slot, LINKS[link]), cutoffs)
        out = out or (ev, want)
    return out


@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "real"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_every_field_and_array_against_the_oracle(capi, hc, rows, layout, dyadic):
    ent, rp, y = make_rows(capi, rows, rows + 7 * dyadic, dyadic)
    qid, nq = make_queries(layout, rows, rows)
    hc.set_params(*make_params(rows, dyadic))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    ev, want = check_against_oracle(capi, hc, 0, rows, y, qid, nq)
    if layout == "rows":                                     # every query one row: relevant ones have hits 1 at every cutoff
        assert ev.relevant_queries == int((y >= 0).sum()) and all(ev.at[j].hits == ev.relevant_queries for j in range(4))
        assert all(ev.at[j].ndcg == 1.0 and ev.at[j].recall == 1.0 and ev.at[j].tied_queries == 0 for j in range(4) if ev.relevant_queries)
    if dyadic and rows >= 255 and layout in ("one", "7"):    # ties dominate
        assert ev.at[3].tied_queries > 0


def test_both_links(capi, hc):
    rows = 257
    ent, rp, y = make_rows(capi, rows, 3, False)
    qid, nq = make_queries("7", rows, 3)
    hc.set_params(*make_params(5, False))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid)
    a, _ = check_against_oracle(capi, hc, 0, rows, y, qid, nq, links=("logistic", "probit"))
    b = hc.evaluate_rank(0, CUTOFFS, capi.LINK_PROBIT)
    assert a.by_query.pooled.logloss != b.by_query.pooled.logloss          # the link changes the pooled log loss only
    assert bytes(a.at) == bytes(b.at) and a.relevant_queries == b.relevant_queries


def _levels(capi, hc, plan, seed):
    """one entry per row, w = 1 everywhere, no factors: the score of a row is 0.125 + level / 8 exactly, and the level is the
    plan's, so the ranks inside every query are known.  plan: per query a list of (level, label) by descending rank.  The rows
    are uploaded in a seeded random order."""
    qid = np.concatenate([np.full(len(q), i) for i, q in enumerate(plan)]).astype(np.uint32)
    level = np.array([lv for q in plan for lv, _ in q], dtype=np.float64)
    y = np.array([lab for q in plan for _, lab in q], dtype=np.float32)
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(qid))
    qid, level, y = qid[order], level[order], y[order]
    ent = np.zeros(len(qid), dtype=capi.ENTRY_DTYPE)
    ent["id"], ent["value"] = rng.integers(0, N, len(qid)), level / 8.0
    hc.set_params(0.125, np.ones(N), np.zeros((K, N)))
    hc.upload_rows(0, ent, np.arange(len(qid) + 1, dtype=np.uint64), y)
    hc.set_row_queries(0, qid, len(plan))
    assert np.array_equal(hc.predict(0, len(qid)), 0.125 + level / 8.0)
    return qid, y


def _distinct(size, rng):
    return [(1000 - r, 1.0 if rng.random() < 0.4 else -1.0) for r in range(size)]


def test_window_and_run_boundaries_on_purpose(capi, hc):
    """the sorted layout is known (_levels).  Queries of 62, 63, 64, 65, 127, 128 and 129 tie-free rows end their windows one lane
    before, at and one lane after a wavefront step.  Query 7: the ranks 61 .. 66 share a score with labels + - + - - +, so the run
    straddles K = 64 exactly where the walk steps from its first 64 positions to the next (with k_max = 64 its head lies outside
    the window).  Query 8: a mixed run at the ranks 64 .. 67 BEGINS at K = 64 and adds nothing there.  Query 9: a mixed run at the
    ranks 60 .. 63 ENDS at K = 64 and lies inside."""
    rng = np.random.default_rng(19)
    plan = [_distinct(s, rng) for s in (62, 63, 64, 65, 127, 128, 129, 100, 100, 100)]
    for q, (first, labels) in {7: (61, [1, -1, 1, -1, -1, 1]), 8: (64, [1, -1, 1, 1]), 9: (60, [1, -1, -1, 1])}.items():
        for i, lab in enumerate(labels):
            plan[q][first + i] = (1000 - first, float(lab))
    qid, y = _levels(capi, hc, plan, 19)
    top = lambda q, n: sum(1 for _, lab in plan[q][:n] if lab > 0)
    for cutoffs in ((64,), CUTOFFS, (63, 64), (66, 128)):
        ev, want = check_against_oracle(capi, hc, 0, len(qid), y, qid, len(plan), cutoffs)
        _, dcg, hits = hc.evaluate_rank(0, cutoffs, per_query=True)
        if 64 in cutoffs:
            j = cutoffs.index(64)
            assert hits[7, j] == top(7, 61) + (3.0 * 3.0) / 6.0           # 3 relevant of 6, 3 of the run's 6 ranks above the cutoff
            assert hits[8, j] == top(8, 64) and hits[9, j] == top(9, 64)
            assert ev.at[j].tied_queries == 2                            # queries 7 and 9
        if 65 in cutoffs:
            j = cutoffs.index(65)
            assert ev.at[j].tied_queries == 3 and hits[8, j] == top(8, 64) + (3.0 * 1.0) / 4.0
        for q in range(7):                                               # tie-free queries: integer hits at every cutoff
            assert [hits[q, j] for j in range(len(cutoffs))] == [top(q, k) for k in cutoffs]


def test_zero_model(capi, hc):
    """every score equal: one run per query, hits_q = pos_q min(K, m) / m and dcg_q = pos_q D[min(K, m)] / m in the stated order"""
    rows = 300
    ent, rp, y = make_rows(capi, rows, 11, True)
    qid, nq = make_queries("7", rows, 11)
    hc.set_params(0.0, np.zeros(N), np.zeros((K, N)))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq + 2)                       # two empty queries at the end
    ev, dcg, hits = hc.evaluate_rank(0, CUTOFFS, per_query=True)
    D = capi.rank_discounts(max(CUTOFFS))
    for q in range(nq + 2):
        m, pos = int((qid == q).sum()), int(((qid == q) & (y >= 0)).sum())
        for j, k in enumerate(CUTOFFS):
            b = min(k, m)
            assert hits[q, j] == ((float(pos) * float(b - 0)) / float(m) if m else 0.0)
            assert dcg[q, j] == ((float(pos) * (D[b] - D[0])) / float(m) if m else 0.0)
    assert ev.by_query.valid_queries == 7 and all(ev.at[j].tied_queries == 7 for j in range(4))      # the two-class queries
    check_against_oracle(capi, hc, 0, rows, y, qid, nq + 2)


def test_no_ties_and_cutoffs_above_every_query(capi, hc):
    rng = np.random.default_rng(23)
    plan = [_distinct(s, rng) for s in (1, 2, 63, 64, 65, 130, 7, 1)]
    plan[6] = [(lv, -1.0) for lv, _ in plan[6]]              # a query without a relevant row
    qid, y = _levels(capi, hc, plan, 23)
    ev, want = check_against_oracle(capi, hc, 0, len(qid), y, qid, len(plan), (130, 200, 65536))
    _, dcg, hits = hc.evaluate_rank(0, (130, 200, 65536), per_query=True)
    pos = np.array([sum(1 for _, lab in q if lab > 0) for q in plan], dtype=np.float64)
    assert np.array_equal(hits, np.repeat(pos[:, None], 3, axis=1))
    R = int((pos > 0).sum())
    assert ev.relevant_queries == R < len(plan)
    for j in range(3):
        assert ev.at[j].recall == 1.0 and ev.at[j].hits == pos.sum() and ev.at[j].tied_queries == 0


def test_one_long_query(capi, hc):
    """70 000 rows in one query (and 500 in a second): the walk over the first takes 1024 steps at K = 65536 < m; K = 1000 lies
    below the first query's size and above the second's"""
    rows = 70500
    ent, rp, y = make_rows(capi, rows, 47, False)
    qid = np.zeros(rows, dtype=np.uint32)
    qid[70000:] = 1
    hc.set_params(*make_params(4, False))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, 2)
    ev, want = check_against_oracle(capi, hc, 0, rows, y, qid, 2, (1, 1000, 65536))
    assert ev.relevant_queries == 2 and ev.at[2].hits > 20000


def test_many_empty_queries(capi, hc):
    rows, nq = 300, 2 ** 24 + 3
    ent, rp, y = make_rows(capi, rows, 23, True)
    ids = np.array([0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 2], dtype=np.uint32)
    qid = ids[np.random.default_rng(23).integers(0, len(ids), rows)]
    hc.set_params(*make_params(23, True))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    ev, want = check_against_oracle(capi, hc, 0, rows, y, qid, nq, per_query=False)
    assert ev.by_query.empty_queries == nq - 5 and ev.relevant_queries == 5


@pytest.mark.parametrize("k", [0, 17])
def test_other_factor_widths(capi, k):
    h = handle(capi, k=k)
    ent, rp, y = make_rows(capi, 257, 3, False)
    qid, nq = make_queries("7", 257, 9)
    w0, w, v = make_params(5, False, k)
    h.set_params(w0, w, v if k else None)
    h.upload_rows(0, ent, rp, y)
    h.set_row_queries(0, qid, nq)
    check_against_oracle(capi, h, 0, 257, y, qid, nq, links=("logistic", "probit"))
    h.close()


def test_nan_and_infinite_weights(capi, hc):
    rows, j = 4097, 17
    ent, rp, y = make_rows(capi, rows, 21, False, positive_values=True)
    qid, nq = make_queries("65", rows, 21)
    w0, w, v = make_params(2, False)
    w[j] = np.nan
    hc.set_params(w0, w, v)
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    ev, want = check_against_oracle(capi, hc, 0, rows, y, qid, nq)
    assert ev.by_query.pooled.nan_rows > 0 and ev.relevant_queries == 0 and ev.topk_seconds == 0.0 and ev.by_query.rank_seconds == 0.0
    assert all(math.isnan(ev.at[c].ndcg) and ev.at[c].hits == 0.0 and ev.at[c].tied_queries == 0 for c in range(4))
    w[j] = np.inf                                            # +inf scores tie at the top of their queries
    hc.set_params(w0, w, v)
    assert np.isposinf(hc.predict(0, rows)).any()
    ev, want = check_against_oracle(capi, hc, 0, rows, y, qid, nq)
    assert ev.by_query.pooled.nan_rows == 0 and ev.relevant_queries == 65 and ev.at[0].tied_queries > 0
    w[j] = -np.inf                                           # -inf scores tie at the bottom: the run's tail lies inside the window
    hc.set_params(w0, w, v)                                  # only where the window reaches the end of the query's segment
    p = hc.predict(0, rows)
    sizes = np.bincount(qid, minlength=nq)
    assert np.isneginf(p).any() and not np.isposinf(p).any() and sizes.min() < 64 < 65 < sizes.max()
    ev, want = check_against_oracle(capi, hc, 0, rows, y, qid, nq)
    assert ev.by_query.pooled.nan_rows == 0 and ev.relevant_queries == 65
    lows = [q for q in range(nq) if np.isneginf(p[qid == q]).sum() > 1 and len(set(y[(qid == q) & np.isneginf(p)])) == 2]
    assert any(sizes[q] <= 64 for q in lows) and any(sizes[q] > 65 for q in lows)      # mixed -inf runs inside and outside K = 64 / 65
    assert ev.at[3].tied_queries >= ev.at[0].tied_queries


def test_regression_handle(capi):
    rows = 257
    ent, rp, y = make_rows(capi, rows, 31, False)
    y = np.random.default_rng(5).normal(0.0, 0.8, rows).astype(np.float32)
    h = handle(capi, task=0)
    h.set_params(*make_params(3, False))
    h.upload_rows(0, ent, rp, y)
    h.set_row_queries(0, *make_queries("7", rows, 1))
    ev, dcg, hits = h.evaluate_rank(0, CUTOFFS, per_query=True)
    bq = h.evaluate_by_query(0)
    for f in POOLED_FIELDS:
        assert same(getattr(ev.by_query.pooled, f), getattr(bq.pooled, f)), f
    assert ev.by_query.pooled.rmse > 0 and ev.by_query.queries == 7 and ev.topk_seconds == 0.0 and ev.relevant_queries == 0
    assert all(math.isnan(getattr(ev.at[c], f)) for c in range(4) for f in AT_FIELDS) and [ev.at[c].k for c in range(4)] == list(CUTOFFS)
    assert all(ev.at[c].hits == 0.0 and ev.at[c].tied_queries == 0 for c in range(4)) and not dcg.any() and not hits.any()
    h.close()


def test_one_class_and_empty_slots(capi, hc):
    rows = 300
    ent, rp, y = make_rows(capi, rows, 11, True)
    qid, nq = make_queries("7", rows, 11)
    hc.set_params(*make_params(1, False))
    for sign in (1.0, -1.0):                                 # pooled sorts nothing, the by-query pipeline and the top-K reduction run
        ys = np.full(rows, sign, dtype=np.float32)
        hc.upload_rows(0, ent, rp, ys)
        hc.set_row_queries(0, qid, nq + 2)
        ev, want = check_against_oracle(capi, hc, 0, rows, ys, qid, nq + 2)
        assert ev.relevant_queries == (7 if sign > 0 else 0) and ev.by_query.one_class_queries == 7 and ev.topk_seconds > 0.0
        if sign > 0:
            assert all(ev.at[c].ndcg == 1.0 and ev.at[c].tied_queries == 0 for c in range(4))
    hc.upload_rows(0, ent[:0], np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.float32))     # an empty slot
    hc.set_row_queries(0, np.zeros(0, dtype=np.uint32), 4)
    ev, dcg, hits = hc.evaluate_rank(0, (5, 6), per_query=True)
    assert (ev.by_query.queries, ev.by_query.empty_queries, ev.relevant_queries, ev.n_cutoffs) == (4, 4, 0, 2)
    assert math.isnan(ev.at[0].ndcg) and math.isnan(ev.at[1].precision) and ev.at[1].k == 6 and ev.by_query.pooled.rows == 0
    assert dcg.shape == (4, 2) and not dcg.any() and not hits.any() and ev.topk_seconds == 0.0
    assert bytes_outside_the_times(capi, ev)[:C.sizeof(capi.EvalQuery)] == bytes(hc.evaluate_by_query(0))[:C.sizeof(capi.EvalQuery)]


def test_two_calls_are_bit_identical(capi, hc):
    rows = 4097 * 8
    ent, rp, y = make_rows(capi, rows, 43, False)
    qid, nq = make_queries("sparse", rows, 43)
    hc.set_params(*make_params(4, False))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    a, b = hc.evaluate_rank(0, CUTOFFS, 1, per_query=True), hc.evaluate_rank(0, CUTOFFS, 1, per_query=True)
    assert bytes_outside_the_times(capi, a[0]) == bytes_outside_the_times(capi, b[0]) and a[0].relevant_queries > 1000
    for x, z in zip(a[1:], b[1:]):
        assert np.array_equal(x, z)
    c = hc.evaluate_rank(0, CUTOFFS, 1)                      # the means do not depend on whether the arrays were asked for
    assert bytes_outside_the_times(capi, c) == bytes_outside_the_times(capi, a[0])


def test_weight_side_stream(capi):
    rows = 4097
    ent, rp, y = make_rows(capi, rows, 51, False)
    qid, nq = make_queries("65", rows, 51)
    h = handle(capi)
    h.set_params(*make_params(6, False))
    h.upload_rows(0, ent, rp, y)
    h.set_row_queries(0, qid, nq)
    h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_FUSED, 256, 32, capi.FLAG_KEEP_WSIDE, 2)
    ev, _ = check_against_oracle(capi, h, 0, rows, y, qid, nq)
    assert ev.by_query.pooled.flags & capi.EVAL_WSIDE and ev.relevant_queries == 65
    h.close()


def test_kept_relation_blocks(capi, hc):
    rows = 4097
    ent, rp, y, rel = _relational(capi, rows, 61)
    qid, nq = make_queries("65", rows, 61)
    hc.set_params(*make_params(7, True))
    hc.upload_block_rows(0, ent, rp, y, rel, keep=True)
    hc.upload_block_rows(1, ent, rp, y, rel, keep=False)
    hc.set_row_queries(0, qid, nq)
    hc.set_row_queries(1, qid, nq)
    a, b = hc.evaluate_rank(0, CUTOFFS, per_query=True), hc.evaluate_rank(1, CUTOFFS, per_query=True)
    assert bytes_outside_the_times(capi, a[0]) == bytes_outside_the_times(capi, b[0]) and a[0].at[1].tied_queries > 0
    assert all(np.array_equal(x, z) for x, z in zip(a[1:], b[1:]))
    check_against_oracle(capi, hc, 0, rows, y, qid, nq)
    hc.free_rows(1)


@pytest.mark.parametrize("world", [2, 3])
def test_loopback_groups(capi, hc, world):
    rows = 4097
    ent, rp, y = make_rows(capi, rows, 71, True)             # dyadic: the shards' y-hat does not differ in rounding
    qid, nq = make_queries("sparse", rows, 71)
    params = make_params(8, True)
    hc.set_params(*params)
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    hs = [handle(capi, device=0, shard_rank=r, shard_world=world, shard_hash=1) for r in range(world)]
    g = capi.Group(hs)
    g.set_params(*params)
    g.upload_rows(0, ent, rp, y)
    with pytest.raises(capi.FmxError) as ei:
        g.evaluate_rank(0, CUTOFFS)
    assert ei.value.code == -3 and "no query ids" in ei.value.text and "fmx_group_evaluate_rank" in ei.value.text
    g.set_row_queries(0, qid, nq)
    for link in LINKS.values():
        one, grp = hc.evaluate_rank(0, CUTOFFS, link, per_query=True), g.evaluate_rank(0, CUTOFFS, link, per_query=True)
        R = one[0].relevant_queries
        assert grp[0].relevant_queries == R > 100 and grp[0].n_cutoffs == 4
        for f in INT_FIELDS:
            assert getattr(grp[0].by_query, f) == getattr(one[0].by_query, f), f
        for j, k in enumerate(CUTOFFS):
            assert (grp[0].at[j].k, grp[0].at[j].tied_queries) == (k, one[0].at[j].tied_queries)
            for f in ("hits",) + AT_FIELDS:
                assert abs(getattr(grp[0].at[j], f) - getattr(one[0].at[j], f)) <= mean_bound(getattr(one[0].at[j], f), R, k), f
        assert all(np.array_equal(x, z) for x, z in zip(one[1:], grp[1:]))
        gq = g.evaluate_by_query(0, link)
        for f in POOLED_FIELDS:
            assert same(getattr(grp[0].by_query.pooled, f), getattr(gq.pooled, f)), f
    with pytest.raises(capi.FmxError) as ei:                 # a shard handle passed to fmx_evaluate_rank itself
        hs[0].evaluate_rank(0, CUTOFFS)
    assert ei.value.code == -4 and "fmx_evaluate_rank" in ei.value.text
    g.close()
    for h in hs:
        h.close()


def test_one_handle_group_forwards(capi):
    rows = 257
    ent, rp, y = make_rows(capi, rows, 91, False)
    qid, nq = make_queries("7", rows, 91)
    h = handle(capi)
    g = capi.Group([h])
    h.set_params(*make_params(10, False))
    h.upload_rows(0, ent, rp, y)
    g.set_row_queries(0, qid, nq)
    assert bytes_outside_the_times(capi, g.evaluate_rank(0, CUTOFFS, 1)) == bytes_outside_the_times(capi, h.evaluate_rank(0, CUTOFFS, 1))
    assert g.evaluate_rank(0, (3,)).relevant_queries == 7
    g.close()
    h.close()


def test_state_and_arguments(capi):
    h = handle(capi)
    lib = capi.load()
    rows = 65
    ent, rp, y = make_rows(capi, rows, 3, True)
    qid, nq = make_queries("7", rows, 3)
    h.set_params(*make_params(3, True))

    def refused(fn, code, *needles):
        with pytest.raises(capi.FmxError) as ei:
            fn()
        assert ei.value.code == code
        for n in needles + ("fmx_evaluate_rank",):
            assert n in ei.value.text, ei.value.text

    refused(lambda: h.evaluate_rank(0, CUTOFFS), -3, "holds no rows")                           # a slot never uploaded
    h.upload_rows(0, ent, rp, y)
    refused(lambda: h.evaluate_rank(0, CUTOFFS), -3, "no query ids")                            # before set_row_queries
    h.set_row_queries(0, qid, nq)
    first = h.evaluate_rank(0, CUTOFFS, per_query=True)
    refused(lambda: h.evaluate_rank(0, ()), -1, "n_cutoffs")
    refused(lambda: h.evaluate_rank(0, (1, 2, 3, 4, 5)), -1, "n_cutoffs")
    refused(lambda: h.evaluate_rank(0, (0, 5)), -1, "cutoff 0")
    refused(lambda: h.evaluate_rank(0, (5, 65537)), -1, "cutoff 1", "65536")
    refused(lambda: h.evaluate_rank(0, (5, 5)), -1, "ascending")
    refused(lambda: h.evaluate_rank(0, (1, 10, 9)), -1, "ascending")
    refused(lambda: h.evaluate_rank(0, CUTOFFS, 2), -1, "unknown link")
    refused(lambda: h.evaluate_rank(8, CUTOFFS), -1, "out of range")
    bad = qid.copy()
    bad[40] = 7
    with pytest.raises(capi.FmxError):
        h.set_row_queries(0, bad, nq)
    again = h.evaluate_rank(0, CUTOFFS, per_query=True)                                         # the previous ids stay in force
    assert bytes_outside_the_times(capi, first[0]) == bytes_outside_the_times(capi, again[0])
    assert all(np.array_equal(x, z) for x, z in zip(first[1:], again[1:]))
    h.upload_rows(2, ent, rp, None)
    h.set_row_queries(2, qid, nq)
    refused(lambda: h.evaluate_rank(2, CUTOFFS), -3, "without targets")
    h.set_row_queries(0, None)
    refused(lambda: h.evaluate_rank(0, CUTOFFS), -3, "no query ids")
    h.set_row_queries(0, qid, nq)
    out, opts = capi.EvalRank(), capi.RankOpts(0, 0, 1, (5, 0, 0, 0), 0)
    assert lib.fmx_evaluate_rank(h.h, 0, C.byref(opts), None, None, None) == -1 and b"out is NULL" in lib.fmx_last_error(h.h)
    assert lib.fmx_evaluate_rank(h.h, 0, None, C.byref(out), None, None) == -1 and b"opts is NULL" in lib.fmx_last_error(h.h)
    assert lib.fmx_evaluate_rank(h.h, 0, C.byref(capi.RankOpts(0, 1, 1, (5, 0, 0, 0), 0)), C.byref(out), None, None) == -1
    assert b"fmx_evaluate_rank" in lib.fmx_last_error(h.h) and b"flags" in lib.fmx_last_error(h.h)
    assert lib.fmx_evaluate_rank(None, 0, C.byref(opts), C.byref(out), None, None) == -1
    assert lib.fmx_evaluate_rank(h.h, 0, C.byref(opts), C.byref(out), None, None) == 0 and out.at[0].k == 5 and out.n_cutoffs == 1
    h2 = handle(capi)                                        # per_query needs the ids set through the object
    h2.upload_rows(0, ent, rp, y)
    assert lib.fmx_set_row_queries(h2.h, 0, qid.ctypes.data, nq) == 0
    with pytest.raises(RuntimeError, match="not set through this object"):
        h2.evaluate_rank(0, CUTOFFS, per_query=True)
    h2.close()
    h.close()


def test_sgd_learner(capi, capsys):
    from libfm_amd import learner as L
    tr, te = L.Data(*_separable(capi, 200, 1)), L.Data(*_separable(capi, 200, 2))
    qid = np.random.default_rng(4).integers(0, 9, 200)

    def run(cutoffs):
        l = _learner(L, L.FMLearnSGD)
        l.learn_rate = 0.05
        if cutoffs is not None:
            l.rank_cutoffs = cutoffs
        l.init()
        l.set_queries(te, qid)                               # the test set only: Train prints nan
        l.learn(tr, te)
        return l, capsys.readouterr()

    plain, cap0 = run(None)
    assert plain.rank_cutoffs == () and "ndcg" not in cap0.err and not any("@" in key for key in plain.log[-1])
    plain.close()
    l, cap = run((5,))
    assert cap.out == cap0.out and cap.err.count("\tndcg@5: Train=nan\tTest=") == 5 == l.num_iter
    want = rank_metrics(l.predict_raw(te), te.target, qid, 9, (5, 10), discounts=capi.rank_discounts(10))
    ev = l.evaluate_rank(te, (5, 10))
    assert ev.relevant_queries == want["relevant_queries"] == 9
    for j in range(2):
        assert ev.at[j].tied_queries == want["at"][j]["tied_queries"]
        for f in ("hits",) + AT_FIELDS:
            assert abs(getattr(ev.at[j], f) - want["at"][j][f]) <= mean_bound(want["at"][j][f], 9, (5, 10)[j]), f
    assert abs(l.log[-1]["ndcg@5_test"] - want["at"][0]["ndcg"]) <= mean_bound(want["at"][0]["ndcg"], 9, 5) and want["at"][0]["ndcg"] > 0.7
    assert {"recall@5_test", "precision@5_test", "ndcg@5_train"} <= set(l.log[-1]) and math.isnan(l.log[-1]["ndcg@5_train"])
    with pytest.raises(ValueError):
        l.evaluate_rank(tr, (5,))
    l.close()
    with pytest.raises(NotImplementedError):
        L.FMLearnMCMC().evaluate_rank(te, (5,))


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-handle", "two-shards"])
def test_als_learner(capi, capsys, devices):
    from libfm_amd import learner as L
    tr, te = L.Data(*_separable(capi, 200, 1)), L.Data(*_separable(capi, 200, 2))
    qtr, qte = np.random.default_rng(5).integers(0, 9, 200), np.random.default_rng(6).integers(0, 5, 200)
    l = _learner(L, L.FMLearnALS)
    l.num_iter, l.w_lambda, l.v_lambda, l.devices, l.rank_cutoffs = 2, 1.0, 1.0, devices, (3, 20)
    l.init()
    l.set_queries(tr, qtr)
    l.set_queries(te, qte, 6)
    l.learn(tr, te)
    want = rank_metrics(l._h.predict(1, te.num_cases), te.target, qte, 6, (3, 20), "probit", discounts=capi.rank_discounts(20))
    ev = l.evaluate_rank(te, (3, 20))
    assert (ev.relevant_queries, ev.by_query.queries, ev.by_query.empty_queries) == (want["relevant_queries"], 6, 1)
    for j, k in enumerate((3, 20)):
        assert ev.at[j].tied_queries == want["at"][j]["tied_queries"]
        for got in (ev.at[j].ndcg, l.log[-1]["ndcg@%d_test" % k]):
            assert abs(got - want["at"][j]["ndcg"]) <= mean_bound(want["at"][j]["ndcg"], want["relevant_queries"], k)
        assert not math.isnan(l.log[-1]["ndcg@%d_train" % k])
    err = capsys.readouterr().err
    assert err.count("\tndcg@3: Train=") == 2 and err.count("\tndcg@20: Train=") == 2
    l.close()


def test_cli_rank_at(capi, tmp_path, capsys):
    from libfm_amd import cli
    trf, tef = str(tmp_path / "tr.libfm"), str(tmp_path / "te.libfm")
    _write_libfm(trf, *_separable(capi, 200, 1))
    _write_libfm(tef, *_separable(capi, 200, 2))
    qtr, qte = str(tmp_path / "qtr.txt"), str(tmp_path / "qte.txt")
    np.savetxt(qtr, np.random.default_rng(7).integers(0, 9, 200), fmt="%d")
    np.savetxt(qte, np.random.default_rng(8).integers(0, 9, 200), fmt="%d")
    rlog = str(tmp_path / "rlog.tsv")
    argv = ["-task", "c", "-train", trf, "-test", tef, "-dim", "1,1,2", "-iter", "3", "-method", "sgd", "-learn_rate", "0.05",
            "-init_stdev", "0.1", "-seed", "42", "-test_queries", qte]
    assert cli.main(argv) == 0
    plain = capsys.readouterr()
    assert cli.main(argv + ["-rank_at", "5,10"]) == 0
    ranked = capsys.readouterr()
    assert cli.main(argv + ["-rank_at", "5,10", "-train_queries", qtr, "-rlog", rlog]) == 0
    both = capsys.readouterr()
    assert ranked.out == plain.out == both.out and plain.out.count("#Iter=") == 3
    assert "ndcg" not in plain.err and plain.err.count("\tgauc: ") == 3
    assert ranked.err.count("\tndcg@5: Train=nan\tTest=") == 3 and ranked.err.count("\tndcg@10: Train=nan\tTest=") == 3
    assert both.err.count("\tndcg@5: Train=") == 3 and "nan" not in both.err
    header = {c.strip() for c in open(rlog).readline().split("\t")}
    assert {"%s@%d_%s" % (m, k, s) for m in AT_FIELDS for k in (5, 10) for s in ("train", "test")} <= header
