"""The bf16 serving snapshot on the MI355X: what scoring from it costs against scoring from the fp32 model, and what the rounding does
to a trained model's held-out metrics.

    python scripts/compact_rate.py [--what rate,quality] [--reps 3] [--out profiles/compact_rate.jsonl]

rate    : fmx_evaluate (the slot's weight side stream not current: the plain gather of w) and fmx_compact_evaluate take turns on one
          handle and slot, one warm-up each, then the fastest of --reps by fmx_eval::device_seconds, at three shapes:
            headline    n = 1e8,   k = 64, 32 one-hot entries per row, 2^22 rows (bench.py's workload)
            configs[1]  n = 1e7,   k = 32, 16 entries per row,         2^23 rows
            criteo      n = 3.3e7, k = 64, 39 entries per row,         2^20 rows, Criteo-shaped ids (FMX_SYNTH_CRITEO)
          Next to the measured ratio: the byte model's bound (4 rs + 72) / (2 rs + 72) per entry -- rs the row stride in elements,
          64 the sector of the 4-byte w gather, 8 the entry -- and the snapshot's bytes against the model's.
quality : scripts/ftrl_rate.py's Criteo-shaped FTRL run (n = 3.3e7, 39 entries per row, k = 64, alpha 0.01, beta 1, l2 0.001 on V,
          l1 = (0.2, 0.1), batch 4 096, five epochs), then the log loss and the exact AUC of the held-out rows from the fp32 model
          (fmx_evaluate_ex) and from the snapshot (fmx_compact_evaluate_ex), and the snapshot's fmx_compact_info.
Prints one JSON line per measurement and appends it to --out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libfm_amd import capi  # noqa: E402

SHAPES = (("headline", 100_000_000, 64, 32, 1 << 22, capi.SYNTH_UNIFORM),
          ("configs[1]", 10_000_000, 32, 16, 1 << 23, capi.SYNTH_UNIFORM),
          ("criteo", 33_000_000, 64, 39, 1 << 20, capi.SYNTH_CRITEO))


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def info_dict(ci):
    return {f: getattr(ci, f) for f, _ in capi.CompactInfo._fields_}


def rate(reps, out):
    for name, n, k, nnz, rows, shape in SHAPES:
        h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0)
        h.init_params(0.0, 0.01, 1)
        h.synth_rows(0, 123, 0, rows, nnz, shape)
        ci = h.compact_begin()
        a, b = h.evaluate(0), h.compact_evaluate(0)                        # warm-up
        assert not (a.flags & capi.EVAL_WSIDE)
        t32, t16 = [], []
        for _ in range(reps):                                              # taking turns
            a, b = h.evaluate(0), h.compact_evaluate(0)
            t32.append(a.device_seconds)
            t16.append(b.device_seconds)
        rs = (ci.bytes_compact // ci.features - 4) // 2
        emit({"what": "rate", "shape": name, "features": n, "factors": k, "nnz": nnz, "rows": rows, "reps": reps, "row_stride": int(rs),
              "fp32_s": min(t32), "bf16_s": min(t16), "fp32_all_s": t32, "bf16_all_s": t16,
              "fp32_Mrows_s": rows / min(t32) / 1e6, "bf16_Mrows_s": rows / min(t16) / 1e6,
              "speedup": min(t32) / min(t16), "byte_model_bound": (4 * rs + 72) / (2 * rs + 72),
              "fp32_model_GBs": rows * nnz * (4 * rs + 72) / min(t32) / 1e9, "bf16_model_GBs": rows * nnz * (2 * rs + 72) / min(t16) / 1e9,
              "accuracy_fp32": a.accuracy, "accuracy_bf16": b.accuracy, "compact": info_dict(ci)}, out)
        h.close()
        capi.release_cached_memory()


def quality(out):
    n, k, nnz, rows, held = 33_000_000, 64, 39, 1 << 19, 1 << 17
    lr, batch, l1_w, l1_v = 0.01, 4096, 0.2, 0.1
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, lr, -1.0, 1.0)
    h.synth_rows(0, 123, 0, rows, nnz, capi.SYNTH_CRITEO)
    h.synth_rows(1, 123, rows, held, nnz, capi.SYNTH_CRITEO)
    h.init_params(0.0, 0.05, 19)
    h.ftrl_begin(lr, 1.0, l1_w, l1_v, 0.0, 0.001)
    for _ in range(5):
        h.ftrl_epoch(0, batch, 0)
    ci = h.compact_begin()                                                 # (inside the open session)
    a, b = h.evaluate_ex(1), h.compact_evaluate_ex(1)
    emit({"what": "quality", "rule": "ftrl", "l1_w": l1_w, "l1_v": l1_v, "epochs": 5, "rows": rows, "held_out_rows": held,
          "logloss_fp32": a.logloss, "logloss_bf16": b.logloss, "auc_fp32": a.auc, "auc_bf16": b.auc,
          "auc_num2_fp32": int(a.auc_num2), "auc_num2_bf16": int(b.auc_num2), "accuracy_fp32": a.accuracy, "accuracy_bf16": b.accuracy,
          "compact": info_dict(ci)}, out)
    h.ftrl_end()
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="rate,quality")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "compact_rate.jsonl"))
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("compact_rate.py needs a HIP device: nothing here is measured on a CPU")
    what = a.what.split(",")
    if "rate" in what:
        rate(a.reps, a.out)
    if "quality" in what:
        quality(a.out)


if __name__ == "__main__":
    main()
