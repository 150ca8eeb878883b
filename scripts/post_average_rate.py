"""One iteration of MCMC's averaged test prediction on the MI355X: the host route against the device's.

    python scripts/post_average_rate.py [--features 10000000] [--factors 64] [--nnz 32] [--rows 10000000] [--reps 3]

A classification handle with n = 1e7 features, k = 64, n_test = 1e7 rows of 32 one-hot entries generated on the device
(fmx_synth_rows), parameters filled on the device (fmx_init_params).  All routes run in this process on that handle: one
warm-up, then the median of --reps, with the host clock around calls that end in a synchronise.  Per iteration:

  (a) the host route of the learners without device_average: fmx_predict to the host, cdf_gaussian and the add into
      pred_sum_all in numpy, the accuracy of the mean in numpy -- wall clock;
  (b) fmx_post_accumulate: its device_seconds and the wall clock;
  (c) fmx_post_evaluate_ex(FMX_POST_ALL): its device_seconds and rank_seconds.

Prints one JSON line.  (a) and (b) must agree on the accuracy of the mean, which the script asserts on the first iteration
(one draw: the same fp32 predictions).
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
from libfm_amd.evalmetrics import ref_cdf_gaussian  # noqa: E402


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
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    h = capi.Handle(a.features, a.factors, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.0, 0.01, -1.0, 1.0)
    h.init_params(0.0, 0.01, 1)
    h.synth_rows(0, 123, 0, a.rows, a.nnz)
    y = np.zeros(a.rows, dtype=np.float32)
    h._chk(h.lib.fmx_download_rows(h.h, 0, None, None, y.ctypes.data))          # the targets alone
    state = {"sum": np.zeros(a.rows), "draws": 0}

    def route_a():
        p = h.predict(0, a.rows)
        state["sum"] += ref_cdf_gaussian(p)
        state["draws"] += 1
        return float(np.mean(((state["sum"] / state["draws"]) >= 0.5) == (y >= 0)))

    def route_b():
        return h.post_accumulate(0)

    def route_c():
        return h.post_evaluate_ex(0, capi.POST_ALL)

    acc_first = route_a()
    h.post_begin(0)
    first = h.post_accumulate(0)
    pos_zero = int(np.count_nonzero(y == 0))                           # (the reference's rule never counts a zero target)
    assert abs(first.m[capi.POST_ALL].accuracy - acc_first) <= pos_zero / a.rows + 1e-12, (first.m[capi.POST_ALL].accuracy, acc_first)
    ta, _ = timed(route_a, a.reps)
    tb, st = timed(route_b, a.reps)
    tc, ev = timed(route_c, a.reps)
    print(json.dumps({"rows": a.rows, "features": a.features, "factors": a.factors, "nnz": a.nnz, "reps": a.reps,
                      "host_route_s": ta,
                      "post_accumulate_s": tb, "post_accumulate_device_s": st.device_seconds,
                      "post_evaluate_ex_s": tc, "post_evaluate_ex_device_s": ev.device_seconds, "rank_s": ev.rank_seconds,
                      "draws": int(st.draws), "accuracy_all": st.m[capi.POST_ALL].accuracy, "ll_ref_all": st.m[capi.POST_ALL].ll_ref,
                      "auc": ev.auc, "logloss": ev.logloss}), flush=True)
    h.close()


if __name__ == "__main__":
    main()
