"""Per-query AUC (GAUC) of one slot on the MI355X: what fmx_evaluate_by_query costs on top of fmx_evaluate_ex, and against the host
route.

    python scripts/evalq_rate.py [--features 10000000] [--factors 64] [--nnz 32] [--rows 4194304] [--queries 100000] [--reps 3]

A classification handle with n = 1e7 features, k = 64, rows of 32 one-hot entries generated on the device (fmx_synth_rows),
parameters filled on the device (fmx_init_params); every row belongs to one of --queries queries whose sizes follow a Zipf law
(query r is drawn with weight 1 / (r + 1), seeded).  All three routes run in this process on that handle: one warm-up, then the
median of --reps, with the host clock around calls that end in a synchronise:

  (a) fmx_evaluate_ex: the pooled metrics alone;
  (b) fmx_predict to the host + a numpy per-query equivalent of evalmetrics.query_metrics (one lexsort by (qid, score), run
      counting in int64, segment sums per query): the route a host-side GAUC has to take;
  (c) fmx_evaluate_by_query, with its device_seconds and rank_seconds (by-query sort, scans, rank-sum and final kernels).

Prints one JSON line; (b) and (c) must agree on num2_within exactly, which the script asserts.  For the kernel split run
`rocprofv3 --kernel-trace --stats -- python scripts/evalq_rate.py --only-device` in a run of its own: a warm-up and one call of (c).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libfm_amd import capi  # noqa: E402


def zipf_queries(rows, n_queries, seed):
    """one query id per row: query r with probability proportional to 1 / (r + 1)"""
    rng = np.random.default_rng(seed)
    cdf = np.cumsum(1.0 / np.arange(1, n_queries + 1))
    return np.minimum(np.searchsorted(cdf / cdf[-1], rng.random(rows)), n_queries - 1).astype(np.uint32)


def host_query_metrics(p, y, qid):
    """query_metrics' integers and means with numpy instead of Python loops: (num2_within, den2_within, gauc, auc_macro, valid)"""
    p = p.astype(np.float32) + np.float32(0.0)                         # -0 -> +0
    order = np.lexsort((p, qid))                                       # by query, then by score
    ps, qs, lab = p[order], qid[order], (y >= 0)[order]
    head = np.concatenate(([True], (ps[1:] != ps[:-1]) | (qs[1:] != qs[:-1])))   # a run of equal scores inside one query
    run = np.cumsum(head) - 1
    rq = qs[head]                                                      # the query of every run
    neg_run = np.bincount(run, weights=~lab).astype(np.int64)
    pos_run = np.bincount(run, weights=lab).astype(np.int64)
    first = np.flatnonzero(np.concatenate(([True], rq[1:] != rq[:-1])))  # first run of every present query
    neg_before = np.cumsum(neg_run) - neg_run
    neg_below = neg_before - np.repeat(neg_before[first], np.diff(np.concatenate((first, [len(rq)]))))
    num2_q = np.add.reduceat(pos_run * (2 * neg_below + neg_run), first)
    pos_q, neg_q = np.add.reduceat(pos_run, first), np.add.reduceat(neg_run, first)
    valid = (pos_q > 0) & (neg_q > 0)
    num2_q, pos_q, neg_q = num2_q[valid], pos_q[valid], neg_q[valid]
    auc_q = num2_q / (2.0 * pos_q * neg_q)
    rows_q = pos_q + neg_q
    return (int(num2_q.sum()), int((2 * pos_q * neg_q).sum()), float(np.sum(rows_q * auc_q) / rows_q.sum()), float(auc_q.mean()),
            int(valid.sum()))


def timed(fn, reps):
    fn()                                                               # warm-up
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=10_000_000)
    ap.add_argument("--factors", type=int, default=64)
    ap.add_argument("--nnz", type=int, default=32)
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-device", action="store_true", help="a warm-up and one fmx_evaluate_by_query: the run to put under a profiler")
    a = ap.parse_args()
    h = capi.Handle(a.features, a.factors, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.0, 0.01, -1.0, 1.0)
    h.init_params(0.0, 0.01, 1)
    h.synth_rows(0, 123, 0, a.rows, a.nnz)
    y = np.zeros(a.rows, dtype=np.float32)
    h._chk(h.lib.fmx_download_rows(h.h, 0, None, None, y.ctypes.data))          # the targets alone
    qid = zipf_queries(a.rows, a.queries, 7)
    h.set_row_queries(0, qid, a.queries)

    def route_a():
        return h.evaluate_ex(0, capi.LINK_LOGISTIC)

    def route_b():
        return host_query_metrics(h.predict(0, a.rows), y, qid)

    def route_c():
        return h.evaluate_by_query(0, capi.LINK_LOGISTIC)

    if a.only_device:
        route_c()
        ev = route_c()
        print(json.dumps({"rows": a.rows, "queries": a.queries, "by_query_device_s": ev.device_seconds, "rank_s": ev.rank_seconds}), flush=True)
        h.close()
        return
    ta, ev_a = timed(route_a, a.reps)
    tb, (num2_b, den2_b, gauc_b, macro_b, valid_b) = timed(route_b, a.reps)
    tc, ev_c = timed(route_c, a.reps)
    assert int(ev_c.num2_within) == num2_b, (int(ev_c.num2_within), num2_b)
    assert int(ev_c.den2_within) == den2_b and int(ev_c.valid_queries) == valid_b
    sizes = np.bincount(qid, minlength=a.queries)
    print(json.dumps({"rows": a.rows, "features": a.features, "factors": a.factors, "nnz": a.nnz, "queries": a.queries, "reps": a.reps,
                      "largest_query": int(sizes.max()), "median_query": int(np.median(sizes)), "empty_queries": int(ev_c.empty_queries),
                      "evaluate_ex_s": ta, "evaluate_ex_device_s": ev_a.device_seconds, "evaluate_ex_rank_s": ev_a.rank_seconds,
                      "predict_host_numpy_s": tb,
                      "by_query_s": tc, "by_query_device_s": ev_c.device_seconds, "by_query_rank_s": ev_c.rank_seconds,
                      "by_query_minus_ex_s": tc - ta,
                      "gauc": ev_c.gauc, "gauc_host": gauc_b, "auc_macro": ev_c.auc_macro, "auc_macro_host": macro_b,
                      "auc_within": ev_c.auc_within, "num2_within": int(ev_c.num2_within), "valid_queries": int(ev_c.valid_queries),
                      "pooled_auc": ev_c.pooled.auc}), flush=True)
    h.close()


if __name__ == "__main__":
    main()
