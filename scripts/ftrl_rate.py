"""FTRL-proximal with L1 on the minibatch rule (fmx_ftrl_epoch) on the MI355X: what it costs and what it buys.

    python scripts/ftrl_rate.py [--what throughput,convergence] [--reps 3] [--factors 64] [--out FILE]

throughput : scripts/adagrad_rate.py's shape: one handle, n = 1e6 features, k = --factors (64 by default; 8 times the path with several
             rows per wave-wide load), 2^20 rows of 32 one-hot entries generated on the device, batches 16 384 and 65 536. fmx_ftrl_epoch against fmx_adapt_epoch and fmx_sgd_epoch(MINIBATCH,
             FMX_APPLY_SEGMENTED) -- the three share the row sums and the recurrence and differ in the owner kernel -- taking turns in
             this process (the AdaGrad and the FTRL session exclude each other, so each turn opens and ends its session outside the
             timed epoch), one warm-up epoch each per batch size, then the fastest of --reps epochs by
             fmx_epoch_stats::device_seconds.  The byte model next to it: per touched feature the plain owner moves 2 rows, the
             AdaGrad owner 4, this one 6 (V, z, n, each read and written).
convergence: scripts/adagrad_rate.py's Criteo-shaped run (n = 3.3e7, 39 entries per row, classification, k = 64, learn_rate = alpha =
             0.01, beta 1, l2 = 0.001 on V, batch 4 096): five epochs each with l1 = (0, 0), (0.2, 0.1) and (2, 1), every run from the
             same start values; after every epoch the log loss of the held-out rows (fmx_evaluate_ex), the epoch's examples/s and
             the zero counts of the model (fmx_param_sparsity).
Prints one JSON line per measurement (and appends them to --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libfm_amd import capi  # noqa: E402


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def sparsity_dict(sp):
    return {f: int(getattr(sp, f)) for f, _ in capi.Sparsity._fields_}


def throughput(reps, k, out):
    n, nnz, rows = 1_000_000, 32, 1 << 20
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0)
    h.init_params(0.0, 0.01, 1)
    h.synth_rows(0, 123, 0, rows, nnz)
    for b in (16384, 65536):
        def plain():
            return h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, b, 0)

        def adapt():
            h.adapt_begin("adagrad", 1.0, 0.01)
            st = h.adapt_epoch(0, b, 0)
            h.adapt_end()
            return st

        def ftrl():
            h.ftrl_begin(0.01, 1.0, 0.05, 0.02, 0.0, 0.001)
            st = h.ftrl_epoch(0, b, 0)
            h.ftrl_end()
            return st
        plain(), adapt(), ftrl()                                           # warm-up (and the segments of this batch size)
        tp, ta, tf = [], [], []
        for _ in range(reps):                                              # taking turns
            tp.append(plain().device_seconds)
            ta.append(adapt().device_seconds)
            st = ftrl()
            tf.append(st.device_seconds)
        # the byte model's upper bound: every occurrence its own (batch, feature) segment
        row = 4 * k
        common = rows * nnz * row * 2 + rows * row                         # V rows for the sums + S rows per occurrence + S write
        emit({"what": "throughput", "batch": b, "rows": rows, "features": n, "factors": k, "nnz": nnz, "reps": reps,
              "sgd_segmented_s": min(tp), "adagrad_s": min(ta), "ftrl_s": min(tf),
              "sgd_segmented_all_s": tp, "adagrad_all_s": ta, "ftrl_all_s": tf,
              "sgd_segmented_Mex_s": rows / min(tp) / 1e6, "adagrad_Mex_s": rows / min(ta) / 1e6, "ftrl_Mex_s": rows / min(tf) / 1e6,
              "ftrl_over_adagrad_time": min(tf) / min(ta), "ftrl_over_sgd_time": min(tf) / min(tp),
              "byte_model_ftrl_over_adagrad_upper": (common + rows * nnz * 6 * row) / (common + rows * nnz * 4 * row),
              "max_feature_count": int(st.max_feature_count)}, out)
    h.close()


def convergence(out):
    n, k, nnz, rows, held = 33_000_000, 64, 39, 1 << 19, 1 << 17
    lr, batch = 0.01, 4096
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, lr, -1.0, 1.0)
    h.synth_rows(0, 123, 0, rows, nnz, capi.SYNTH_CRITEO)
    h.synth_rows(1, 123, rows, held, nnz, capi.SYNTH_CRITEO)
    for l1_w, l1_v in ((0.0, 0.0), (0.2, 0.1), (2.0, 1.0)):
        h.init_params(0.0, 0.05, 19)                                       # every run from the same start values
        h.ftrl_begin(lr, 1.0, l1_w, l1_v, 0.0, 0.001)                      # (again = reset, z from these start values)
        ll0 = h.evaluate_ex(1).logloss
        sp0 = sparsity_dict(h.param_sparsity())
        lls, rates, sps = [], [], []
        for _ in range(5):
            st = h.ftrl_epoch(0, batch, 0)
            rates.append(rows / st.device_seconds / 1e6)
            lls.append(h.evaluate_ex(1).logloss)
            sps.append(sparsity_dict(h.param_sparsity()))
        emit({"what": "convergence", "rule": "ftrl", "l1_w": l1_w, "l1_v": l1_v, "alpha": lr, "beta": 1.0, "l2_w": 0.0, "l2_v": 0.001,
              "batch_used": int(st.batch_used), "rows": rows, "held_out_rows": held, "logloss_start": ll0, "sparsity_start": sp0,
              "logloss_per_epoch": lls, "Mex_s_per_epoch": rates, "sparsity_per_epoch": sps}, out)
    h.ftrl_end()
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="throughput,convergence")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--factors", type=int, default=64, help="k of the throughput run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("ftrl_rate.py needs a HIP device: nothing here is measured on a CPU")
    what = a.what.split(",")
    if "throughput" in what:
        throughput(a.reps, a.factors, a.out)
    if "convergence" in what:
        convergence(a.out)


if __name__ == "__main__":
    main()
