"""AUC and log loss of one slot on the MI355X: three routes to the metrics of a classification model.

    python scripts/eval_ex_rate.py [--features 10000000] [--factors 64] [--nnz 32] [--rows 4194304] [--reps 3]

A classification handle with n = 1e7 features, k = 64, rows of 32 one-hot entries generated on the device (fmx_synth_rows),
parameters filled on the device (fmx_init_params).  All three routes run in this process on that handle: one warm-up, then the
median of --reps, with the host clock around calls that end in a synchronise:

  (a) fmx_evaluate: the pass alone (accuracy only) -- what the scoring costs;
  (b) fmx_predict to the host + the numpy equivalent of evalmetrics.classification_metrics (stable argsort, run counting in
      int64, fp64 log loss): the route a host-side `-metrics` would have to take;
  (c) fmx_evaluate_ex, with its device_seconds and rank_seconds (sort + scans + rank-sum kernel).

Prints one JSON line; (b) and (c) must agree on the AUC numerator exactly, which the script asserts.  For the kernel split run
the script on its own under `rocprofv3 --kernel-trace --stats`.
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


def host_metrics(p, y):
    """classification_metrics' AUC numerator and logistic log loss with numpy instead of Python loops"""
    p = p.astype(np.float32) + np.float32(0.0)                         # -0 -> +0
    positive = y >= 0
    order = np.argsort(p, kind="stable")
    ps, lab = p[order], positive[order]
    run = np.cumsum(np.concatenate(([True], ps[1:] != ps[:-1]))) - 1   # index of the run of equal scores
    neg_run = np.bincount(run, weights=~lab).astype(np.int64)
    pos_run = np.bincount(run, weights=lab).astype(np.int64)
    neg_below = np.cumsum(neg_run) - neg_run
    num2 = int(np.sum(pos_run * (2 * neg_below + neg_run)))
    z = np.where(positive, p, -p).astype(np.float64)
    return num2, float(np.sum(np.maximum(-z, 0.0) + np.log1p(np.exp(-np.abs(z)))) / len(z))


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
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    h = capi.Handle(a.features, a.factors, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.0, 0.01, -1.0, 1.0)
    h.init_params(0.0, 0.01, 1)
    h.synth_rows(0, 123, 0, a.rows, a.nnz)
    y = np.zeros(a.rows, dtype=np.float32)
    h._chk(h.lib.fmx_download_rows(h.h, 0, None, None, y.ctypes.data))          # the targets alone

    def route_a():
        return h.evaluate(0)                                           # (ends in a stream synchronise)

    def route_b():
        return host_metrics(h.predict(0, a.rows), y)

    def route_c():
        return h.evaluate_ex(0, capi.LINK_LOGISTIC)

    ta, ev_a = timed(route_a, a.reps)
    tb, (num2_b, ll_b) = timed(route_b, a.reps)
    tc, ev_c = timed(route_c, a.reps)
    assert int(ev_c.auc_num2) == num2_b, (int(ev_c.auc_num2), num2_b)
    print(json.dumps({"rows": a.rows, "features": a.features, "factors": a.factors, "nnz": a.nnz, "reps": a.reps,
                      "evaluate_s": ta, "evaluate_device_s": ev_a.device_seconds,
                      "predict_host_numpy_s": tb,
                      "evaluate_ex_s": tc, "evaluate_ex_device_s": ev_c.device_seconds, "rank_s": ev_c.rank_seconds,
                      "ex_minus_evaluate_s": tc - ta,
                      "auc": ev_c.auc, "auc_num2": int(ev_c.auc_num2), "logloss": ev_c.logloss, "logloss_host": ll_b,
                      "pos": int(ev_c.pos), "neg": int(ev_c.neg)}), flush=True)
    h.close()


if __name__ == "__main__":
    main()
