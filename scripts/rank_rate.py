"""NDCG / recall / precision at K inside the queries of one slot on the MI355X: what fmx_evaluate_rank adds to
fmx_evaluate_by_query.

    python scripts/rank_rate.py [--features 33000000] [--factors 64] [--nnz 39] [--rows 4194304] [--queries 100000,1000000]
                                [--cutoffs 10,100] [--reps 3]

A classification handle with Criteo-shaped rows generated on the device (fmx_synth_rows_ex, FMX_SYNTH_CRITEO), parameters filled on
the device (fmx_init_params); every row gets one of Q seeded uniform query ids, for each Q of --queries.  One warm-up of each call,
then the median of --reps of

  topk_seconds             of fmx_evaluate_rank: the added kernels only (k_rankq_bounds, k_rankq_top, k_rankq_final2)
  by_query.rank_seconds    of the same call: the by-query sort, scans, rank-sum and final kernels
  rank_seconds             of a plain fmx_evaluate_by_query on the same slot

and the host clock around both calls.  Prints one JSON line per Q; the integers of both calls must agree, which the script asserts.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=33_000_000)
    ap.add_argument("--factors", type=int, default=64)
    ap.add_argument("--nnz", type=int, default=39)
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--queries", default="100000,1000000")
    ap.add_argument("--cutoffs", default="10,100")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    cutoffs = tuple(int(x) for x in a.cutoffs.split(","))
    h = capi.Handle(a.features, a.factors, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.0, 0.01, -1.0, 1.0)
    h.init_params(0.0, 0.01, 1)
    h.synth_rows(0, 123, 0, a.rows, a.nnz, capi.SYNTH_CRITEO)
    for nq in (int(x) for x in a.queries.split(",")):
        qid = np.random.default_rng(7).integers(0, nq, a.rows).astype(np.uint32)
        h.set_row_queries(0, qid, nq)
        h.evaluate_rank(0, cutoffs)
        h.evaluate_by_query(0)
        ranks, plains, wall_r, wall_p = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ranks.append(h.evaluate_rank(0, cutoffs))
            t1 = time.perf_counter()
            plains.append(h.evaluate_by_query(0))
            wall_r.append(t1 - t0)
            wall_p.append(time.perf_counter() - t1)
        ev, bq = ranks[-1], plains[-1]
        assert (ev.by_query.num2_within, ev.by_query.valid_queries) == (bq.num2_within, bq.valid_queries)
        med = statistics.median
        sizes = np.bincount(qid, minlength=nq)
        print(json.dumps({"rows": a.rows, "features": a.features, "factors": a.factors, "nnz": a.nnz, "queries": nq, "cutoffs": cutoffs,
                          "reps": a.reps, "median_query": int(np.median(sizes)), "largest_query": int(sizes.max()),
                          "relevant_queries": int(ev.relevant_queries),
                          "topk_s": med(e.topk_seconds for e in ranks), "rank_call_by_query_rank_s": med(e.by_query.rank_seconds for e in ranks),
                          "plain_by_query_rank_s": med(e.rank_seconds for e in plains),
                          "rank_call_device_s": med(e.device_seconds for e in ranks), "plain_device_s": med(e.device_seconds for e in plains),
                          "rank_call_wall_s": med(wall_r), "plain_wall_s": med(wall_p),
                          "at": [{"k": int(x.k), "ndcg": x.ndcg, "recall": x.recall, "precision": x.precision, "hits": x.hits,
                                  "tied_queries": int(x.tied_queries)} for x in ev.at[:ev.n_cutoffs]]}), flush=True)
    h.close()


if __name__ == "__main__":
    main()
