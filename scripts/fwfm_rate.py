"""Rates of the field-weighted FM on one MI355X: fmx_fwfm_epoch against fmx_adapt_epoch -- the parent's rule, on
the same handle and rows -- and fmx_fwfm_predict against fmx_predict, at k = 64 with 39 fields, on uniform and Criteo-shaped rows.

    python scripts/fwfm_rate.py [--rows 1048576] [--reps 5] [--out profiles/fwfm_rate.jsonl]

Every time is a device time between two events: the epochs' device_seconds, and for scoring the device_seconds of fmx_fwfm_evaluate
and fmx_evaluate (the rest pass of predict plus one reduction, no copy to the host); the median of --reps after one warm-up.  One JSON line per (shape, batch)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libfm_amd import capi  # noqa: E402

K, NNZ, FIELDS, N = 64, 39, 39, 1 << 22


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []
    for shape, name in ((capi.SYNTH_UNIFORM, "uniform"), (capi.SYNTH_CRITEO, "criteo")):
        for batch in (512, 4096, 65536):
            h = capi.Handle(N, K, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.0, 0.05, -1.0, 1.0)
            try:
                h.init_params(0.0, 0.01, 1)
                h.set_groups((np.arange(N) % FIELDS).astype(np.uint32))
                h.synth_rows(0, 7, 0, a.rows, NNZ, shape)
                h.adapt_begin("adagrad", 1.0, 0.05)
                h.fwfm_begin()
                med = {}
                for what, fn in (("adapt", lambda: h.adapt_epoch(0, batch, 32).device_seconds), ("fwfm", lambda: h.fwfm_epoch(0, batch, 32).device_seconds)):
                    fn()
                    med[what] = float(np.median([fn() for _ in range(a.reps)]))
                for what, fn in (("predict", lambda: h.evaluate(0).device_seconds), ("fwfm_predict", lambda: h.fwfm_evaluate(0).device_seconds)):
                    fn()
                    med[what] = float(np.median([fn() for _ in range(a.reps)]))
            finally:
                h.close()
            line = {"shape": name, "k": K, "fields": FIELDS, "rows": a.rows, "batch": batch,
                    "adapt_epoch_s": med["adapt"], "fwfm_epoch_s": med["fwfm"], "epoch_ratio": med["fwfm"] / med["adapt"],
                    "fwfm_examples_per_s": a.rows / med["fwfm"], "adapt_examples_per_s": a.rows / med["adapt"],
                    "predict_s": med["predict"], "fwfm_predict_s": med["fwfm_predict"], "predict_ratio": med["fwfm_predict"] / med["predict"]}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
