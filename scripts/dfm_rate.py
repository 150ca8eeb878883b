"""Rates of DeepFM on one MI355X: fmx_dfm_epoch against fmx_fmfm_epoch and fmx_adapt_epoch, and fmx_dfm_evaluate
against fmx_fmfm_evaluate and fmx_evaluate, on the same handle and rows, at k = 16 with 39 fields (WP = 624) and 256 hidden units, on
uniform and Criteo-shaped rows of 39 entries.

    python scripts/dfm_rate.py [--rows 1048576] [--reps 5] [--hidden 256] [--batches 512,4096,65536] [--out profiles/dfm_rate.jsonl]

Every time is a device time between two events: the epochs' device_seconds and the device_seconds of the evaluate calls (the rest pass
plus one reduction, no copy to the host); the median of --reps after one warm-up, all in one process.  The FmFM and DeepFM sessions
exclude each other, so each is opened, timed and closed in turn on the handle.  One JSON line per (shape, batch), with the multiply-adds
of the three GEMMs per example.  Under `rocprofv3 --kernel-trace --stats -- python scripts/dfm_rate.py ...` the kernel table gives the
times of k_dfm_gemm_h, k_dfm_gemm_z and k_dfm_wgrad."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libfm_amd import capi  # noqa: E402

K, NNZ, FIELDS, N = 16, 39, 39, 1 << 22
WP = (K * FIELDS + 15) // 16 * 16


def median_of(fn, reps):
    fn()
    return float(np.median([fn() for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--batches", default="512,4096,65536")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    hp = (a.hidden + 15) // 16 * 16
    rng = np.random.default_rng(1)
    net = rng.normal(0.0, 0.05, size=(K * FIELDS, a.hidden)), rng.normal(0.0, 0.05, size=a.hidden), rng.normal(0.0, 0.05, size=a.hidden)
    lines = []
    for shape, name in ((capi.SYNTH_UNIFORM, "uniform"), (capi.SYNTH_CRITEO, "criteo")):
        for batch in (int(b) for b in a.batches.split(",")):
            h = capi.Handle(N, K, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.0, 0.05, -1.0, 1.0)
            try:
                h.init_params(0.0, 0.01, 1)
                h.set_groups((np.arange(N) % FIELDS).astype(np.uint32))
                h.synth_rows(0, 7, 0, a.rows, NNZ, shape)
                h.adapt_begin("adagrad", 1.0, 0.05)
                med = {"adapt": median_of(lambda: h.adapt_epoch(0, batch, 32).device_seconds, a.reps),
                       "eval": median_of(lambda: h.evaluate(0).device_seconds, a.reps)}
                h.fmfm_begin()
                med["fmfm"] = median_of(lambda: h.fmfm_epoch(0, batch, 32).device_seconds, a.reps)
                med["fmfm_eval"] = median_of(lambda: h.fmfm_evaluate(0).device_seconds, a.reps)
                h.fmfm_end()
                h.dfm_begin(a.hidden)
                h.dfm_set_net(*net)
                med["dfm"] = median_of(lambda: h.dfm_epoch(0, batch, 32).device_seconds, a.reps)
                med["dfm_eval"] = median_of(lambda: h.dfm_evaluate(0).device_seconds, a.reps)
            finally:
                h.close()
            line = {"shape": name, "k": K, "fields": FIELDS, "hidden": a.hidden, "rows": a.rows, "batch": batch, "adapt_epoch_s": med["adapt"],
                    "fmfm_epoch_s": med["fmfm"], "dfm_epoch_s": med["dfm"], "dfm_examples_per_s": a.rows / med["dfm"],
                    "epoch_vs_fmfm": med["dfm"] / med["fmfm"], "epoch_vs_adapt": med["dfm"] / med["adapt"],
                    "evaluate_s": med["eval"], "fmfm_evaluate_s": med["fmfm_eval"], "dfm_evaluate_s": med["dfm_eval"],
                    "evaluate_vs_fmfm": med["dfm_eval"] / med["fmfm_eval"], "evaluate_vs_fm": med["dfm_eval"] / med["eval"],
                    "madds_per_example": {"gemm_h": WP * hp, "gemm_z": WP * hp, "wgrad": (WP + 128) * hp}}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
