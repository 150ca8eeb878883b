"""Rates of the field-matrixed FM on one MI355X: fmx_fmfm_epoch against fmx_fwfm_epoch and fmx_adapt_epoch on the
same handle and rows, and fmx_fmfm_evaluate against fmx_fwfm_evaluate, at k = 16 with 39 fields (WP = 624), on uniform and Criteo-shaped
rows of 39 entries.

    python scripts/fmfm_rate.py [--rows 1048576] [--reps 5] [--batches 512,4096,65536] [--out profiles/fmfm_rate.jsonl]

Every time is a device time between two events: the epochs' device_seconds and the device_seconds of the two evaluate calls (the rest
pass plus one reduction, no copy to the host); the median of --reps after one warm-up, all in one process.  The FwFM and FmFM sessions
exclude each other, so each is opened, timed and closed in turn on the handle.  One JSON line per (shape, batch).  Under
`rocprofv3 --kernel-trace --stats -- python scripts/fmfm_rate.py ...` the kernel table gives k_fmfm_gemm_t's and k_fmfm_mgrad's times."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libfm_amd import capi  # noqa: E402

K, NNZ, FIELDS, N = 16, 39, 39, 1 << 22


def median_of(fn, reps):
    fn()
    return float(np.median([fn() for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="512,4096,65536")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []
    for shape, name in ((capi.SYNTH_UNIFORM, "uniform"), (capi.SYNTH_CRITEO, "criteo")):
        for batch in (int(b) for b in a.batches.split(",")):
            h = capi.Handle(N, K, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.0, 0.05, -1.0, 1.0)
            try:
                h.init_params(0.0, 0.01, 1)
                h.set_groups((np.arange(N) % FIELDS).astype(np.uint32))
                h.synth_rows(0, 7, 0, a.rows, NNZ, shape)
                h.adapt_begin("adagrad", 1.0, 0.05)
                med = {"adapt": median_of(lambda: h.adapt_epoch(0, batch, 32).device_seconds, a.reps)}
                h.fwfm_begin()
                med["fwfm"] = median_of(lambda: h.fwfm_epoch(0, batch, 32).device_seconds, a.reps)
                med["fwfm_eval"] = median_of(lambda: h.fwfm_evaluate(0).device_seconds, a.reps)
                h.fwfm_end()
                h.fmfm_begin()
                med["fmfm"] = median_of(lambda: h.fmfm_epoch(0, batch, 32).device_seconds, a.reps)
                med["fmfm_eval"] = median_of(lambda: h.fmfm_evaluate(0).device_seconds, a.reps)
            finally:
                h.close()
            line = {"shape": name, "k": K, "fields": FIELDS, "rows": a.rows, "batch": batch, "adapt_epoch_s": med["adapt"],
                    "fwfm_epoch_s": med["fwfm"], "fmfm_epoch_s": med["fmfm"], "fmfm_examples_per_s": a.rows / med["fmfm"],
                    "epoch_vs_fwfm": med["fmfm"] / med["fwfm"], "epoch_vs_adapt": med["fmfm"] / med["adapt"],
                    "fwfm_evaluate_s": med["fwfm_eval"], "fmfm_evaluate_s": med["fmfm_eval"], "evaluate_vs_fwfm": med["fmfm_eval"] / med["fwfm_eval"]}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
