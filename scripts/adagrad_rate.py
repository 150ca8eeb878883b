"""AdaGrad on the minibatch rule (fmx_adapt_epoch) on the MI355X: what it costs and what it buys.

    python scripts/adagrad_rate.py [--what throughput,convergence] [--reps 3] [--out FILE]

throughput : one handle, n = 1e6 features, k = 64, 2^20 rows of 32 one-hot entries generated on the device, batches 16 384 and 65 536.
             fmx_adapt_epoch against fmx_sgd_epoch(MINIBATCH, FMX_APPLY_SEGMENTED) -- its three-launch sibling: the same row sums, the
             same recurrence, k_apply_seg instead of k_adapt_apply_seg -- alternating in this process, one warm-up epoch each per batch
             size (it also builds the (batch, feature) segments), then the fastest of --reps epochs by fmx_epoch_stats::device_seconds
             (HIP events around the epoch's launches).  The byte model next to it: per example both move nnz V rows (the sums) and write
             and read one S row per occurrence; per touched feature the plain owner moves 2 rows (V read + write), the AdaGrad owner 4
             (V and accumulator, read + write).
convergence: Criteo-shaped rows (fmx_synth_rows_ex(FMX_SYNTH_CRITEO): n = 3.3e7, 39 entries per row), classification, k = 64,
             learn_rate 0.01: 2^19 train rows and 2^17 held-out rows of the same generator.  Five epochs each of plain SGD
             (fmx_sgd_epoch, FMX_APPLY_FUSED, the library's batch), AdaGrad at that batch, at 4 096 and at 65 536, every run from the
             same start values; after every epoch the log loss of the held-out rows (fmx_evaluate_ex) and the epoch's examples/s.
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


def throughput(reps, out):
    n, k, nnz, rows = 1_000_000, 64, 32, 1 << 20
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0)
    h.init_params(0.0, 0.01, 1)
    h.synth_rows(0, 123, 0, rows, nnz)
    h.adapt_begin("adagrad", 1.0, 0.01)
    for b in (16384, 65536):
        def plain():
            return h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, b, 0)

        def adapt():
            return h.adapt_epoch(0, b, 0)
        plain(), adapt()                                                   # warm-up (and the segments of this batch size)
        tp, ta = [], []
        for _ in range(reps):                                              # alternating
            tp.append(plain().device_seconds)
            st = adapt()
            ta.append(st.device_seconds)
        # the byte model's upper bound: every occurrence its own (batch, feature) segment (the library does not report the number of
        # segments; features that repeat inside a batch share one owner, which moves the ratio towards 1)
        row = 4 * k
        common = rows * nnz * row * 2 + rows * row                         # V rows for the sums + S rows per occurrence + S write
        emit({"what": "throughput", "batch": b, "rows": rows, "features": n, "factors": k, "nnz": nnz, "reps": reps,
              "sgd_segmented_s": min(tp), "adagrad_s": min(ta), "sgd_segmented_all_s": tp, "adagrad_all_s": ta,
              "sgd_segmented_Mex_s": rows / min(tp) / 1e6, "adagrad_Mex_s": rows / min(ta) / 1e6,
              "adagrad_over_sgd_time": min(ta) / min(tp),
              "byte_model_ratio_upper": (common + rows * nnz * 4 * row) / (common + rows * nnz * 2 * row),
              "max_feature_count": int(st.max_feature_count)}, out)
    h.adapt_end()
    h.close()


def convergence(out):
    n, k, nnz, rows, held = 33_000_000, 64, 39, 1 << 19, 1 << 17
    lr = 0.01
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, lr, -1.0, 1.0)
    h.synth_rows(0, 123, 0, rows, nnz, capi.SYNTH_CRITEO)
    h.synth_rows(1, 123, rows, held, nnz, capi.SYNTH_CRITEO)
    for name, batch in (("sgd", 0), ("adagrad", 0), ("adagrad", 4096), ("adagrad", 65536)):
        h.init_params(0.0, 0.05, 19)                                       # every run from the same start values
        if name == "adagrad":
            h.adapt_begin("adagrad", 1.0, lr)                              # (again = reset)
        ll0 = h.evaluate_ex(1).logloss
        lls, rates, used = [], [], 0
        for _ in range(5):
            if name == "sgd":
                st = h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_FUSED, batch, 0, 0, 2)
            else:
                st = h.adapt_epoch(0, batch, 0)
            used = int(st.batch_used)
            rates.append(rows / st.device_seconds / 1e6)
            lls.append(h.evaluate_ex(1).logloss)
        emit({"what": "convergence", "rule": name, "batch_requested": batch, "batch_used": used, "rows": rows, "held_out_rows": held,
              "learn_rate": lr, "logloss_start": ll0, "logloss_per_epoch": lls, "Mex_s_per_epoch": rates}, out)
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="throughput,convergence")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("adagrad_rate.py needs a HIP device: nothing here is measured on a CPU")
    what = a.what.split(",")
    if "throughput" in what:
        throughput(a.reps, a.out)
    if "convergence" in what:
        convergence(a.out)


if __name__ == "__main__":
    main()
