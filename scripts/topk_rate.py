"""Rate of top-K retrieval (fmx_topk) on one GPU; the figures of DESIGN.md section 11.

    python scripts/topk_rate.py --Q 65536 --C 1048576 --k 64 --K 100
    python scripts/topk_rate.py --Q 1 --C 10000000 --k 64 --K 100
    python scripts/topk_rate.py --Q 1024 --C 65536 --k 64 --K 100 --baseline

Queries are one user id plus 4 context features, candidates one item id plus 4 item features (values 1); parameters are random.
Prints one JSON line: device and score-and-select seconds of the second of two calls, scores/s, the dot products' TFLOP/s
(2 k Q C) against the 155 TF f32 matrix peak.  --baseline also times what the library offered before: the joined rows written
out on the host, uploaded and predicted with fmx_predict in chunks of queries, then a host top-K per query.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libfm_amd import capi  # noqa: E402

PEAK_TF = 155.0


def rows(rng, n_rows, first_id, n_ids, n_side, side0, per_row=4):
    ids = np.empty((n_rows, 1 + per_row), dtype=np.uint32)
    ids[:, 0] = first_id + np.arange(n_rows) % n_ids
    ids[:, 1:] = side0 + rng.integers(0, n_side, (n_rows, per_row))
    ent = np.zeros(ids.size, dtype=capi.ENTRY_DTYPE)
    ent["id"] = ids.ravel()
    ent["value"] = 1.0
    rp = np.arange(n_rows + 1, dtype=np.uint64) * (1 + per_row)
    return ent, rp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=65536)
    ap.add_argument("--C", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    n_users, n_items, n_side = min(a.Q, 1 << 20), min(a.C, 1 << 22), 1000
    n = n_users + n_items + 2 * n_side
    qe, qr = rows(rng, a.Q, 0, n_users, n_side, n_users + n_items)
    ce, cr = rows(rng, a.C, n_users, n_items, n_side, n_users + n_items + n_side)
    h = capi.Handle(n, a.k)
    h.set_params(0.1, rng.normal(0, 0.1, n), rng.normal(0, 0.1, (a.k, n)))
    h.upload_rows(0, qe, qr, np.zeros(a.Q, np.float32))
    h.upload_rows(1, ce, cr, np.zeros(a.C, np.float32))
    h.topk(0, 1, a.K)                                               # warm-up (code objects, allocations)
    t0 = time.perf_counter()
    idx, sc, st = h.topk(0, 1, a.K, stats=True)
    wall = time.perf_counter() - t0
    flop = 2.0 * a.k * a.Q * a.C
    out = {"Q": a.Q, "C": a.C, "k": a.k, "K": a.K, "splits": st.splits, "wall_s": wall, "device_s": st.device_seconds,
           "score_select_s": st.score_seconds, "other_device_s": st.device_seconds - st.score_seconds,
           "scores_per_s": st.scores / st.score_seconds if st.score_seconds else None,
           "dot_tflops": flop / st.score_seconds * 1e-12 if st.score_seconds else None}
    out["fraction_of_peak"] = out["dot_tflops"] / PEAK_TF if out["dot_tflops"] else None
    out["whole_call_fraction_of_peak"] = flop / st.device_seconds * 1e-12 / PEAK_TF if st.device_seconds else None
    if a.baseline:
        chunk = max(1, (1 << 22) // a.C)                            # queries per materialised batch (4 M joined rows)
        t0 = time.perf_counter()
        best = np.zeros((a.Q, a.K), dtype=np.int64)
        qrow = qe.reshape(a.Q, 5)
        crow = ce.reshape(a.C, 5)
        for q0 in range(0, a.Q, chunk):
            nq = min(chunk, a.Q - q0)
            j = np.concatenate([np.repeat(qrow[q0:q0 + nq], a.C, axis=0), np.tile(crow, (nq, 1))], axis=1)
            h.upload_rows(2, j.ravel(), np.arange(nq * a.C + 1, dtype=np.uint64) * 10, np.zeros(nq * a.C, np.float32))
            p = h.predict(2, nq * a.C).reshape(nq, a.C)
            part = np.argpartition(-p, a.K - 1, axis=1)[:, :a.K]
            order = np.argsort(-np.take_along_axis(p, part, 1), axis=1, kind="stable")
            best[q0:q0 + nq] = np.take_along_axis(part, order, 1)
        out["baseline_wall_s"] = time.perf_counter() - t0
        out["speedup_vs_baseline"] = out["baseline_wall_s"] / wall
        out["baseline_top1_agrees"] = float(np.mean(best[:, 0] == idx[:, 0]))
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
