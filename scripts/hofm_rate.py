"""Rates of the third-order FM on one MI355X: fmx_hofm_epoch against fmx_adapt_epoch and fmx_hofm_evaluate against
fmx_evaluate on the SAME handle of width num_factor = k2 + k3 -- the same gather bytes, so the ratio is the cost of the three power
sums, the second scratch row and the owner's second sum -- on uniform and Criteo-shaped rows of 39 entries.

    python scripts/hofm_rate.py [--rows 1048576] [--reps 5] [--out profiles/hofm_rate.jsonl]

Every time is a device time between two events: the epochs' device_seconds, and for scoring the device_seconds of fmx_hofm_evaluate
and fmx_evaluate (the rest pass plus one reduction, no copy to the host); the median of --reps after one warm-up.  One JSON line per
(width, shape, batch), with the byte model of section 32 and the rate it implies."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libfm_amd import capi  # noqa: E402

NNZ, N = 39, 1 << 22


def model_bytes(rows, k2, k3):
    """(scoring, epoch) bytes of the model: the gather nnz ROW 4 per example; the epoch adds the scratch rows H (ROW floats) and P (ROW - c0
    floats, c0 = k2 rounded down to the lane map's granularity) written once per example and read once per occurrence, and the owner's V
    and accumulator rows read and written once per occurrence (an upper bound: a feature that occurs more than once in a batch moves its
    rows once)"""
    k = k2 + k3
    row = (k + 15) // 16 * 16
    kp = 1 << (k - 1).bit_length()
    vec = max(kp // 64, 1)
    scratch = 2 * min(row, kp) - k2 // vec * vec
    gather = rows * NNZ * row * 4
    return gather, gather + rows * (1 + NNZ) * scratch * 4 + rows * NNZ * 4 * row * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []
    for k2, k3 in ((32, 32), (64, 64)):
        score_b, epoch_b = model_bytes(a.rows, k2, k3)
        for shape, name in ((capi.SYNTH_UNIFORM, "uniform"), (capi.SYNTH_CRITEO, "criteo")):
            for batch in (4096, 65536):
                h = capi.Handle(N, k2 + k3, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.0, 0.05, -1.0, 1.0)
                try:
                    h.init_params(0.0, 0.01, 1)
                    h.synth_rows(0, 7, 0, a.rows, NNZ, shape)
                    h.adapt_begin("adagrad", 1.0, 0.05)
                    h.hofm_begin(k3)
                    med = {}
                    for what, fn in (("adapt", lambda: h.adapt_epoch(0, batch, 32).device_seconds), ("hofm", lambda: h.hofm_epoch(0, batch, 32).device_seconds),
                                     ("evaluate", lambda: h.evaluate(0).device_seconds), ("hofm_evaluate", lambda: h.hofm_evaluate(0).device_seconds)):
                        fn()
                        med[what] = float(np.median([fn() for _ in range(a.reps)]))
                finally:
                    h.close()
                line = {"shape": name, "k2": k2, "k3": k3, "rows": a.rows, "batch": batch,
                        "adapt_epoch_s": med["adapt"], "hofm_epoch_s": med["hofm"], "epoch_ratio": med["hofm"] / med["adapt"],
                        "hofm_examples_per_s": a.rows / med["hofm"], "adapt_examples_per_s": a.rows / med["adapt"],
                        "evaluate_s": med["evaluate"], "hofm_evaluate_s": med["hofm_evaluate"], "evaluate_ratio": med["hofm_evaluate"] / med["evaluate"],
                        "model_epoch_bytes": epoch_b, "model_epoch_gb_per_s": epoch_b / med["hofm"] * 1e-9,
                        "model_evaluate_bytes": score_b, "model_evaluate_gb_per_s": score_b / med["hofm_evaluate"] * 1e-9}
                print(json.dumps(line), flush=True)
                lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
