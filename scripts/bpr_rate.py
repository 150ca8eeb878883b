"""Rate of the pairwise ranking learner (fmx_pair_epoch) on the MI355X, next to the pointwise SGD step on the same rows.

    python scripts/bpr_rate.py [--rows 2097152] [--pairs 2097152] [--seq-pairs 20000]

Rows: n = 1e7 features, k = 64, 32 one-hot entries per row (fmx_synth_rows).  Pairs: random (row a, row b).  Prints one JSON line:
pairs/s of FMX_SGD_SEQUENTIAL and of FMX_SGD_MINIBATCH at B = 65 536, the bytes a pair moves by the formula below and the fraction
of the HBM roofline that is, and the time per example of fmx_sgd_epoch (MINIBATCH, FMX_APPLY_SEGMENTED, the same batch) on the rows.

Bytes per pair of the batch rule (k = 64: a V row is 64 floats = 256 B read, the same written; E = 2 x 32 entries per pair):
  sums   E x (8 B entry + 256 B V row + 4 B w) + 2 x 256 B sums written + 8 B multiplier
  apply  E x (8 B sorted payload + 256 B sums row read) + D x (2 x 256 B V row + 2 x 4 B w), D = distinct (batch, feature) pairs per pair
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libfm_amd import capi  # noqa: E402

HBM_BYTES_PER_S = 8.0e12            # MI355X peak HBM3E bandwidth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--nnz", type=int, default=32)
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--pairs", type=int, default=1 << 21)
    ap.add_argument("--seq-pairs", type=int, default=20000)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--epochs", type=int, default=3)
    a = ap.parse_args()
    h = capi.Handle(a.n, a.k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0, device=0)
    h.init_params(0.0, 0.01, 1)
    h.synth_rows(0, 7, 0, a.rows, a.nnz)
    rng = np.random.default_rng(5)
    pa = rng.integers(0, a.rows, a.pairs).astype(np.uint32)
    pb = rng.integers(0, a.rows, a.pairs).astype(np.uint32)
    out = dict(n=a.n, k=a.k, nnz=a.nnz, rows=a.rows, pairs=a.pairs, batch=a.batch)

    h.upload_pairs(0, pa[:a.seq_pairs], pb[:a.seq_pairs])
    h.pair_epoch(0, capi.SGD_SEQUENTIAL)
    st = h.pair_epoch(0, capi.SGD_SEQUENTIAL)
    out["seq_pairs"] = a.seq_pairs
    out["seq_pairs_per_s"] = a.seq_pairs / st.device_seconds

    h.upload_pairs(0, pa, pb)
    st0 = h.pair_epoch(0, capi.SGD_MINIBATCH, a.batch)
    secs = [h.pair_epoch(0, capi.SGD_MINIBATCH, a.batch).device_seconds for _ in range(a.epochs)]
    t = float(np.median(secs))
    out["setup_seconds"] = st0.setup_seconds
    out["max_feature_count"] = st0.max_feature_count
    out["minibatch_pairs_per_s"] = a.pairs / t
    E = 2 * a.nnz
    row = 4 * a.k
    D = E                                       # uniform ids over 1e7 features: a feature of a batch is almost never repeated
    bytes_pair = E * (8 + row + 4) + 2 * row + 8 + E * (8 + row) + D * (2 * row + 8)
    out["bytes_per_pair"] = bytes_pair
    out["minibatch_roofline_fraction"] = bytes_pair * out["minibatch_pairs_per_s"] / HBM_BYTES_PER_S

    h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, a.batch, 0)
    esecs = [h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, a.batch, 0).device_seconds for _ in range(a.epochs)]
    out["sgd_segmented_ns_per_example"] = 1e9 * float(np.median(esecs)) / a.rows
    out["minibatch_ns_per_pair"] = 1e9 * t / a.pairs
    out["pair_over_example"] = out["minibatch_ns_per_pair"] / out["sgd_segmented_ns_per_example"]
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
