"""The serving snapshots on the MI355X: what scoring from the bf16 and from the int8 row-wise copy costs against scoring from the
fp32 model, and what each rounding does to a trained model's held-out metrics (DESIGN.md sections 19 and 21).

    python scripts/compact_rate.py [--what rate,quality] [--reps 3] [--out profiles/compact_int8_rate.jsonl]

rate    : fmx_evaluate (the slot's weight side stream not current: the plain gather of w), fmx_compact_evaluate from bf16 and
          fmx_compact_evaluate from int8 take turns on one handle and slot (a handle holds one snapshot: each turn of a format takes
          it again, outside the timed call), one warm-up each, then the fastest of --reps by fmx_eval::device_seconds, at three shapes:
            headline    n = 1e8,   k = 64, 32 one-hot entries per row, 2^22 rows (bench.py's workload)
            configs[1]  n = 1e7,   k = 32, 16 entries per row,         2^23 rows
            criteo      n = 3.3e7, k = 64, 39 entries per row,         2^20 rows, Criteo-shaped ids (FMX_SYNTH_CRITEO)
          Next to the measured ratio: the byte model's bound (4 rs + 72) / (2 rs + 72) per entry -- rs the row stride in elements,
          64 the sector of the 4-byte w gather, 8 the entry -- and the snapshot's bytes against the model's.  int8 has no w
          gather: (4 rs + 72) / (P + 8) per entry, and per entry one access of ceil(P / 64) sectors against two of rs / 16 + 1.
quality : scripts/ftrl_rate.py's Criteo-shaped FTRL run (n = 3.3e7, 39 entries per row, k = 64, alpha 0.01, beta 1, l2 0.001 on V,
          l1 = (0.2, 0.1), batch 4 096, five epochs), then the log loss and the exact AUC of the held-out rows from the fp32 model
          (fmx_evaluate_ex) and from each snapshot (fmx_compact_evaluate_ex), and each snapshot's fmx_compact_info.
No rate is printed unless the timed passes scored right (check_scores): on every turn each snapshot's accuracy on the timed slot
lies within 0.01 of the fp32 model's, and after the last turn of a format a second slot of 256 rows, whose ids are drawn over the
whole table, is scored from the snapshot that was just timed and compared with libfm_amd/compact.py's restatement built from the
rows those ids name (fmx_get_param_rows), the snapshot's own rows bit for bit included.
Prints one JSON line per measurement; --out is written anew by every run and every line carries the run's id."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libfm_amd import capi, compact  # noqa: E402

RUN_ID = "%d-%d" % (int(time.time()), os.getpid())

SHAPES = (("headline", 100_000_000, 64, 32, 1 << 22, capi.SYNTH_UNIFORM),
          ("configs[1]", 10_000_000, 32, 16, 1 << 23, capi.SYNTH_UNIFORM),
          ("criteo", 33_000_000, 64, 39, 1 << 20, capi.SYNTH_CRITEO))


def emit(rec, out):
    line = json.dumps(dict(rec, run=RUN_ID))
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def info_dict(ci):
    return {f: getattr(ci, f) for f, _ in capi.CompactInfo._fields_}


def check_rows(h, n, nnz, seed=5, rows=256):
    """slot 1: `rows` rows of nnz entries whose ids are drawn over the whole table; what the restatement needs of the model for them"""
    rng = np.random.default_rng(seed)
    ent = np.zeros(rows * nnz, dtype=capi.ENTRY_DTYPE)
    ent["id"], ent["value"] = rng.integers(0, n, rows * nnz), 1.0
    ent["id"][:nnz] = np.arange(n - nnz, n)
    rp = (np.arange(rows + 1) * nnz).astype(np.uint64)
    h.upload_rows(1, ent, rp, np.ones(rows, dtype=np.float32))
    ids, inv = np.unique(ent["id"], return_inverse=True)
    local = ent.copy()
    local["id"] = inv
    w, v = h.get_param_rows(ids.astype(np.uint32))
    return {"ids": ids.astype(np.uint32), "ent": local, "rp": rp, "rows": rows, "w0": 0.0,          # (init_params: w0 = 0)
            "w": w, "v": v}


def check_scores(h, chk, fmt, shape):
    """the snapshot the handle holds now scores slot 1 as the restatement does, and holds the rows the restatement holds; else SystemExit"""
    got = h.compact_predict(1, chk["rows"])
    cw, cv = h.compact_rows(chk["ids"])
    cm = compact.CompactModel(chk["w0"], chk["w"], chk["v"], True, True, format=fmt)
    want = cm.predict(chk["ent"], chk["rp"])
    rows_equal = np.array_equal(np.asarray(cv, dtype=np.float32).view(np.uint32), cm.v.astype(np.float32).view(np.uint32)) and np.array_equal(cw, chk["w"])
    err = float(np.abs(got - want).max())
    if not rows_equal or not np.all(np.abs(got - want) <= 1e-4 * np.abs(want) + 2e-5):
        raise SystemExit("compact_rate: the %s snapshot at %s does not score as its restatement (rows equal: %s, max difference %g): "
                         "no rate is reported" % (fmt, shape, rows_equal, err))
    return err


def rate(reps, out):
    for name, n, k, nnz, rows, shape in SHAPES:
        h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0)
        h.init_params(0.0, 0.01, 1)
        h.synth_rows(0, 123, 0, rows, nnz, shape)
        chk = check_rows(h, n, nnz)
        acc = {"fp32": [], "bf16": [], "int8": []}
        err16 = err8 = None
        t32, t16, t8 = [], [], []
        for rep in range(reps + 1):                                        # taking turns; turn 0 is the warm-up
            a = h.evaluate(0)
            ci = h.compact_begin(capi.COMPACT_BF16)
            b = h.compact_evaluate(0)
            c8 = h.compact_begin(capi.COMPACT_INT8)
            c = h.compact_evaluate(0)
            assert not (a.flags & capi.EVAL_WSIDE)
            for f, e in (("fp32", a), ("bf16", b), ("int8", c)):
                acc[f].append(e.accuracy)
                if abs(e.accuracy - a.accuracy) > 0.01:
                    raise SystemExit("compact_rate: turn %d at %s: accuracy from %s %.5f, from fp32 %.5f: no rate is reported" % (
                        rep, name, f, e.accuracy, a.accuracy))
            if rep == reps:                                                # the snapshots that were just timed, int8 first (it is held)
                err8 = check_scores(h, chk, "int8", name)
                h.compact_begin(capi.COMPACT_BF16)
                err16 = check_scores(h, chk, "bf16", name)
            if rep:
                t32.append(a.device_seconds)
                t16.append(b.device_seconds)
                t8.append(c.device_seconds)
        rs = (ci.bytes_compact // ci.features - 4) // 2
        P = c8.bytes_compact // c8.features
        emit({"what": "rate", "shape": name, "features": n, "factors": k, "nnz": nnz, "rows": rows, "reps": reps, "row_stride": int(rs),
              "int8_row_bytes": int(P),
              "fp32_s": min(t32), "bf16_s": min(t16), "int8_s": min(t8), "fp32_all_s": t32, "bf16_all_s": t16, "int8_all_s": t8,
              "fp32_Mrows_s": rows / min(t32) / 1e6, "bf16_Mrows_s": rows / min(t16) / 1e6, "int8_Mrows_s": rows / min(t8) / 1e6,
              "speedup": min(t32) / min(t16), "byte_model_bound": (4 * rs + 72) / (2 * rs + 72),
              "speedup_int8": min(t32) / min(t8), "int8_over_bf16": min(t16) / min(t8), "byte_model_bound_int8": (4 * rs + 72) / (P + 8),
              "sectors_per_entry": {"fp32": int(rs // 16 + 1), "bf16": int((2 * rs + 63) // 64 + 1), "int8": int((P + 63) // 64)},
              "accesses_per_entry": {"fp32": 2, "bf16": 2, "int8": 1},
              "fp32_model_GBs": rows * nnz * (4 * rs + 72) / min(t32) / 1e9, "bf16_model_GBs": rows * nnz * (2 * rs + 72) / min(t16) / 1e9,
              "int8_model_GBs": rows * nnz * (P + 8) / min(t8) / 1e9,
              "accuracy_fp32": a.accuracy, "accuracy_bf16": b.accuracy, "accuracy_int8": c.accuracy, "accuracy_all_turns": acc,
              "check_rows": chk["rows"], "check_max_abs_diff_bf16": err16, "check_max_abs_diff_int8": err8,
              "compact": info_dict(ci), "compact_int8": info_dict(c8)}, out)
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
    a = h.evaluate_ex(1)
    ci = h.compact_begin(capi.COMPACT_BF16)                                # (inside the open session)
    b = h.compact_evaluate_ex(1)
    c8 = h.compact_begin(capi.COMPACT_INT8)
    c = h.compact_evaluate_ex(1)
    emit({"what": "quality", "rule": "ftrl", "l1_w": l1_w, "l1_v": l1_v, "epochs": 5, "rows": rows, "held_out_rows": held,
          "logloss_fp32": a.logloss, "logloss_bf16": b.logloss, "logloss_int8": c.logloss,
          "auc_fp32": a.auc, "auc_bf16": b.auc, "auc_int8": c.auc,
          "auc_num2_fp32": int(a.auc_num2), "auc_num2_bf16": int(b.auc_num2), "auc_num2_int8": int(c.auc_num2),
          "accuracy_fp32": a.accuracy, "accuracy_bf16": b.accuracy, "accuracy_int8": c.accuracy,
          "compact": info_dict(ci), "compact_int8": info_dict(c8)}, out)
    h.ftrl_end()
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="rate,quality")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "compact_int8_rate.jsonl"))
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("compact_rate.py needs a HIP device: nothing here is measured on a CPU")
    what = a.what.split(",")
    if a.out and os.path.exists(a.out):
        os.remove(a.out)                                                   # one file, one run
    if "rate" in what:
        rate(a.reps, a.out)
    if "quality" in what:
        quality(a.out)


if __name__ == "__main__":
    main()
