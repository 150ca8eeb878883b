"""Per-row weights (fmx_set_row_weights) on the MI355X: what the weighted recurrence costs and what the weight buys (DESIGN.md
section 23).

    python scripts/weighted_rate.py [--what throughput,calibration] [--reps 3] [--batches 16384,65536,262144] [--out FILE]

throughput : the shapes and batches of scripts/adagrad_rate.py -- uniform rows (n = 1e6 features, k = 64, 2^20 rows of 32 one-hot
             entries; batches 16 384, 65 536 and 262 144) and Criteo-shaped rows (n = 3.3e7, 39 entries per row, 2^19 rows; the same
             batches).  fmx_adapt_epoch and fmx_ftrl_epoch with and without weights on the SAME handle, alternating in this process:
             one warm-up epoch each per batch size (it also builds the (batch, feature) segments), then the fastest of --reps epochs
             by fmx_epoch_stats::device_seconds (HIP events around the whole epoch).  The unweighted epoch of the same run is the
             baseline; the status words say which recurrence ran (parallel in time or the chain).  --batches 4096 is the case in
             which the unweighted epoch runs a one-wavefront chain too.
calibration: Criteo-shaped rows, classification, k = 64, AdaGrad at learn_rate 0.01.  Train on every positive and a seeded quarter
             of the negatives of 2^19 generated rows, with weight 4 on the kept negatives and without weights, each from the same
             start values; after five epochs the log loss of 2^17 held-out rows at the FULL rate (fmx_evaluate_ex) and the mean
             predicted rate (sigmoid of fmx_predict) next to the observed rate of positives.
Prints one JSON line per measurement (and appends them to --out)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libfm_amd import capi  # noqa: E402

WEIGHT_SET = [0, .5, .75, 1, 1, 1.25, 1.5, 2]            # the weights of the parity tests: mean 1


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def throughput(reps, out, batches=(16384, 65536, 262144)):
    shapes = (("uniform", 1_000_000, 32, 1 << 20, capi.SYNTH_UNIFORM), ("criteo", 33_000_000, 39, 1 << 19, capi.SYNTH_CRITEO))
    k = 64
    for shape, n, nnz, rows, synth in shapes:
        h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0)
        h.init_params(0.0, 0.01, 1)
        h.synth_rows(0, 123, 0, rows, nnz, synth)
        c = np.random.default_rng(3).choice(WEIGHT_SET, rows).astype(np.float32)
        for rule in ("adagrad", "ftrl"):
            if rule == "adagrad":
                h.adapt_begin("adagrad", 1.0, 0.01)
            else:
                h.ftrl_begin(0.01, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)

            def epoch(b, weighted):
                h.set_row_weights(0, c if weighted else None)               # (outside the timed events)
                return h.adapt_epoch(0, b, 0) if rule == "adagrad" else h.ftrl_epoch(0, b, 0)
            for b in batches:
                epoch(b, False), epoch(b, True)                             # warm-up (and the segments of this batch size)
                tu, tw, su, sw = [], [], 0, 0
                for _ in range(reps):                                       # alternating
                    st = epoch(b, False)
                    tu.append(st.device_seconds)
                    su |= int(st.status)
                    st = epoch(b, True)
                    tw.append(st.device_seconds)
                    sw |= int(st.status)
                emit({"what": "throughput", "shape": shape, "rule": rule, "batch": b, "rows": rows, "features": n, "factors": k,
                      "nnz": nnz, "reps": reps, "w0_chunk": int(st.w0_chunk_used), "unweighted_s": min(tu), "weighted_s": min(tw),
                      "unweighted_all_s": tu, "weighted_all_s": tw, "unweighted_Mex_s": rows / min(tu) / 1e6,
                      "weighted_Mex_s": rows / min(tw) / 1e6, "weighted_over_unweighted_time": min(tw) / min(tu),
                      "unweighted_scan_pit": bool(su & capi.STAT_SCAN_PIT), "unweighted_scan_serial": bool(su & capi.STAT_SCAN_SERIAL),
                      "weighted_status_ok": bool(sw & capi.STAT_WEIGHTED) and not sw & capi.STAT_SCAN_PIT}, out)
            h.set_row_weights(0, None)
            h.adapt_end() if rule == "adagrad" else h.ftrl_end()
        h.close()


def calibration(out):
    n, k, nnz, rows, held = 33_000_000, 64, 39, 1 << 19, 1 << 17
    lr, keep, epochs = 0.01, 0.25, 5
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, lr, -1.0, 1.0)
    h.synth_rows(0, 123, 0, rows, nnz, capi.SYNTH_CRITEO)
    h.synth_rows(1, 123, rows, held, nnz, capi.SYNTH_CRITEO)
    ent, rp, y = h.download_rows(0)
    _, _, y_held = h.download_rows(1)
    rng = np.random.default_rng(17)
    kept = (y >= 0) | (rng.random(rows) < keep)                             # every positive, a seeded quarter of the negatives
    sizes = np.diff(rp.astype(np.int64))
    sub_rp = np.concatenate([[0], np.cumsum(sizes[kept])]).astype(np.uint64)
    sub_ent = ent[np.repeat(kept, sizes)]
    sub_y = y[kept]
    h.free_rows(0)
    h.upload_rows(0, sub_ent, sub_rp, sub_y)
    c = np.where(sub_y >= 0, 1.0, 1.0 / keep).astype(np.float32)
    observed = float((y_held >= 0).mean())
    for name, weights in (("unweighted", None), ("weighted", c)):
        h.init_params(0.0, 0.05, 19)                                        # every run from the same start values
        h.set_row_weights(0, weights)
        h.adapt_begin("adagrad", 1.0, lr)                                   # (again = reset)
        lls, rates = [], []
        for _ in range(epochs):
            st = h.adapt_epoch(0, 0, 0)
            lls.append(h.evaluate_ex(1).logloss)
            p = h.predict(1, held)
            rates.append(float((1.0 / (1.0 + np.exp(-p))).mean()))
        emit({"what": "calibration", "run": name, "train_rows": int(kept.sum()), "generated_rows": rows, "held_out_rows": held,
              "kept_negative_share": keep, "train_positive_rate": float((sub_y >= 0).mean()), "held_out_positive_rate": observed,
              "batch_used": int(st.batch_used), "status": int(st.status), "held_out_logloss_per_epoch": lls,
              "mean_predicted_rate_per_epoch": rates, "learn_rate": lr}, out)
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="throughput,calibration")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="16384,65536,262144")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("weighted_rate.py needs a HIP device: nothing here is measured on a CPU")
    what = a.what.split(",")
    if "throughput" in what:
        throughput(a.reps, a.out, tuple(int(b) for b in a.batches.split(",")))
    if "calibration" in what:
        calibration(a.out)


if __name__ == "__main__":
    main()
