"""Rates of the field-aware FM on one MI355X: fmx_ffm_epoch against fmx_adapt_epoch and fmx_ffm_evaluate against
fmx_evaluate on a handle of the SAME width num_factor = 39 fields x 4 = 156 -- the same gather bytes, so the ratio is the cost of the
field tile, the transpose and the scratch -- on uniform and Criteo-shaped rows of 39 entries.

    python scripts/ffm_rate.py [--rows 1048576] [--reps 5] [--out profiles/ffm_rate.jsonl]

Every time is a device time between two events: the epochs' device_seconds, and for scoring the device_seconds of fmx_ffm_evaluate and
fmx_evaluate (the rest pass plus one reduction, no copy to the host); the median of --reps after one warm-up.  One JSON line per
(shape, batch), with the byte model of section 30 and the rate it implies."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libfm_amd import capi  # noqa: E402

KF, NNZ, FIELDS, N = 4, 39, 39, 1 << 22
W = KF * FIELDS
ROW = (W + 15) // 16 * 16                                            # floats of a device row, and of a scratch row


def model_bytes(rows):
    """(scoring, epoch) bytes of the model: the gather nnz ROW 4 per example; the epoch adds the scratch written once (F rows) and read
    once per occurrence, and the owner's V and accumulator rows read and written once per occurrence (an upper bound: a feature that
    occurs more than once in a batch moves its rows once)"""
    gather = rows * NNZ * ROW * 4
    return gather, gather + rows * (FIELDS + NNZ) * ROW * 4 + rows * NNZ * 4 * ROW * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []
    score_b, epoch_b = model_bytes(a.rows)
    for shape, name in ((capi.SYNTH_UNIFORM, "uniform"), (capi.SYNTH_CRITEO, "criteo")):
        for batch in (512, 4096, 65536):
            h = capi.Handle(N, W, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.0, 0.05, -1.0, 1.0)
            try:
                h.init_params(0.0, 0.01, 1)
                h.set_groups((np.arange(N) % FIELDS).astype(np.uint32))
                h.synth_rows(0, 7, 0, a.rows, NNZ, shape)
                h.adapt_begin("adagrad", 1.0, 0.05)
                h.ffm_begin(KF)
                med = {}
                for what, fn in (("adapt", lambda: h.adapt_epoch(0, batch, 32).device_seconds), ("ffm", lambda: h.ffm_epoch(0, batch, 32).device_seconds),
                                 ("evaluate", lambda: h.evaluate(0).device_seconds), ("ffm_evaluate", lambda: h.ffm_evaluate(0).device_seconds)):
                    fn()
                    med[what] = float(np.median([fn() for _ in range(a.reps)]))
            finally:
                h.close()
            line = {"shape": name, "latent": KF, "fields": FIELDS, "num_factor": W, "rows": a.rows, "batch": batch,
                    "adapt_epoch_s": med["adapt"], "ffm_epoch_s": med["ffm"], "epoch_ratio": med["ffm"] / med["adapt"],
                    "ffm_examples_per_s": a.rows / med["ffm"], "adapt_examples_per_s": a.rows / med["adapt"],
                    "evaluate_s": med["evaluate"], "ffm_evaluate_s": med["ffm_evaluate"], "evaluate_ratio": med["ffm_evaluate"] / med["evaluate"],
                    "model_epoch_bytes": epoch_b, "model_epoch_gb_per_s": epoch_b / med["ffm"] * 1e-9,
                    "model_evaluate_bytes": score_b, "model_evaluate_gb_per_s": score_b / med["ffm_evaluate"] * 1e-9}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
