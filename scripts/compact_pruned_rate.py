"""The pruned serving snapshot on the MI355X: what scoring through the rank directory costs against scoring from the dense int8
snapshot, and what the snapshot weighs.

    python scripts/compact_pruned_rate.py [--shapes criteo,headline] [--reps 3] [--out profiles/compact_pruned_rate.jsonl]

fmx_compact_evaluate from the dense int8 snapshot and from the pruned int8 snapshot take turns on one handle and slot (a handle holds
one snapshot: each turn takes it again, outside the timed call), one warm-up each, then the fastest of --reps by
fmx_eval::device_seconds, at two shapes:
    criteo    n = 3.3e7, k = 64, 39 entries per row, Criteo-shaped ids (FMX_SYNTH_CRITEO); the snapshot keeps the features that the
              2^19 training rows of slot 0 name (FMX_PRUNE_DEAD | FMX_PRUNE_SEEN), the 2^20 timed rows of slot 2 are further rows of
              the same stream: the features among them that training never met score as rows of zero.  The kept share is reported.
    headline  n = 1e8, k = 64, 32 one-hot entries per row, 2^22 rows (bench.py's workload), FMX_PRUNE_DEAD alone on a model without
              dead rows: every row is kept -- the worst case, the directory lookup is paid and nothing is saved.
No rate is printed unless the timed passes scored right: on every turn the pruned snapshot's fmx_eval equals, field for field, the
dense snapshot's where every row is kept; and after the last turn a second slot of 256 rows -- half of its ids among the first 1 300
features, which every Criteo-shaped row names, half drawn over the whole table -- is scored from each snapshot and compared with
libfm_amd/compact.py's restatement built from the rows those ids name (fmx_get_param_rows) and, for the pruned one, the kept mask the
directory reports for them (fmx_compact_slot_of), the snapshot's own rows bit for bit included; that mask is held against the dead
rule evaluated on the host from the fetched rows (no kept id may be dead; under FMX_PRUNE_DEAD alone the two must be equal) -- which
of the live ids the keep slot names is the device's word alone, its rows never come to the host.  The counts of fmx_compact_prune_info
must add up and the slots of the check ids must ascend with the ids.
Prints one JSON line per shape; --out is written anew by every run and every line carries the run's id."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libfm_amd import capi, compact  # noqa: E402

RUN_ID = "%d-%d" % (int(time.time()), os.getpid())

# name, features, factors, entries per row, keep-slot rows (0: FMX_PRUNE_DEAD alone), timed rows, id shape
SHAPES = {"criteo": (33_000_000, 64, 39, 1 << 19, 1 << 20, capi.SYNTH_CRITEO),
          "headline": (100_000_000, 64, 32, 0, 1 << 22, capi.SYNTH_UNIFORM)}


def emit(rec, out):
    line = json.dumps(dict(rec, run=RUN_ID))
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def struct_dict(st):
    return {f: getattr(st, f) for f, _ in st._fields_}


def check_rows(h, n, nnz, seed=5, rows=256):
    """slot 1: `rows` rows of nnz entries, half of the ids below 1 300, half over the whole table; what the restatement needs for them"""
    rng = np.random.default_rng(seed)
    ent = np.zeros(rows * nnz, dtype=capi.ENTRY_DTYPE)
    ent["id"] = np.where(rng.random(rows * nnz) < 0.5, rng.integers(0, 1300, rows * nnz), rng.integers(0, n, rows * nnz))
    ent["id"][:nnz] = np.arange(n - nnz, n)
    ent["value"] = 1.0
    rp = (np.arange(rows + 1) * nnz).astype(np.uint64)
    h.upload_rows(1, ent, rp, np.ones(rows, dtype=np.float32))
    ids, inv = np.unique(ent["id"], return_inverse=True)
    local = ent.copy()
    local["id"] = inv
    w, v = h.get_param_rows(ids.astype(np.uint32))
    return {"ids": ids.astype(np.uint32), "ent": local, "rp": rp, "rows": rows, "w0": 0.0, "w": w, "v": v}      # (init_params: w0 = 0)


def check_scores(h, chk, shape, pruned, dead_alone=False):
    """the snapshot the handle holds now scores slot 1 as the restatement does and holds the rows the restatement holds; else SystemExit.
    Returns (max difference, kept ids among the check ids)."""
    keep = None
    if pruned:
        slots = h.compact_slot_of(chk["ids"])
        keep = slots != capi.SLOT_NONE
        live = ~compact.dead_mask(chk["w"], chk["v"], True)                # the host's own statement of the rule, from the fetched rows
        if np.any(keep & ~live) or (dead_alone and not np.array_equal(keep, live)):
            raise SystemExit("compact_pruned_rate: the kept ids at %s are not what the dead rule gives: no rate is reported" % shape)
        if np.any(np.diff(slots[keep].astype(np.int64)) <= 0):
            raise SystemExit("compact_pruned_rate: the slots at %s do not ascend with the ids: no rate is reported" % shape)
    got = h.compact_predict(1, chk["rows"])
    cw, cv = h.compact_rows(chk["ids"])
    cm = compact.CompactModel(chk["w0"], chk["w"], chk["v"], True, True, format="int8", keep=keep)
    want = cm.predict(chk["ent"], chk["rp"])
    rows_equal = np.array_equal(np.asarray(cv, dtype=np.float32).view(np.uint32), cm.v.astype(np.float32).view(np.uint32)) and np.array_equal(cw, cm.w)
    err = float(np.abs(got - want).max())
    if not rows_equal or not np.all(np.abs(got - want) <= 1e-4 * np.abs(want) + 2e-5):
        raise SystemExit("compact_pruned_rate: the %s int8 snapshot at %s does not score as its restatement (rows equal: %s, max "
                         "difference %g): no rate is reported" % ("pruned" if pruned else "dense", shape, rows_equal, err))
    return err, (int(keep.sum()) if pruned else len(chk["ids"]))


def rate(name, reps, out):
    n, k, nnz, keep_rows, rows, shape = SHAPES[name]
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0)
    h.init_params(0.0, 0.01, 1)
    if keep_rows:
        h.synth_rows(0, 123, 0, keep_rows, nnz, shape)                     # the training rows: which features were seen
    h.synth_rows(2, 123, keep_rows, rows, nnz, shape)                      # the timed rows: the stream's next rows
    chk = check_rows(h, n, nnz)
    td, tp, acc, bd, bp = [], [], [], [], []
    for rep in range(reps + 1):                                            # taking turns; turn 0 is the warm-up
        t0 = time.perf_counter()
        cd = h.compact_begin(capi.COMPACT_INT8)
        t1 = time.perf_counter()
        a = h.compact_evaluate(2)
        if rep == reps:
            err_d, _ = check_scores(h, chk, name, False)
        t2 = time.perf_counter()
        cp, pi = h.compact_begin_pruned(capi.COMPACT_INT8, 0 if keep_rows else None)
        t3 = time.perf_counter()
        b = h.compact_evaluate(2)
        if rep == reps:
            err_p, chk_kept = check_scores(h, chk, name, True, dead_alone=not keep_rows)
        if pi.kept + pi.dropped_dead + pi.dropped_unseen != n or cp.bytes_compact != pi.bytes_directory + pi.bytes_rows:
            raise SystemExit("compact_pruned_rate: the counts at %s do not add up: no rate is reported" % name)
        if pi.kept == n and (a.rmse, a.mae, a.accuracy, a.rows) != (b.rmse, b.mae, b.accuracy, b.rows):
            raise SystemExit("compact_pruned_rate: every row is kept at %s and the two snapshots score differently: no rate is reported" % name)
        if abs(a.accuracy - b.accuracy) > 0.05:
            raise SystemExit("compact_pruned_rate: turn %d at %s: accuracy %.5f dense, %.5f pruned: no rate is reported" % (rep, name, a.accuracy, b.accuracy))
        acc.append((a.accuracy, b.accuracy))
        bd.append(t1 - t0)
        bp.append(t3 - t2)
        if rep:
            td.append(a.device_seconds)
            tp.append(b.device_seconds)
    P = cd.bytes_compact // cd.features
    emit({"what": "pruned_rate", "shape": name, "features": n, "factors": k, "nnz": nnz, "rows": rows, "keep_rows": keep_rows, "reps": reps,
          "int8_row_bytes": int(P), "dense_s": min(td), "pruned_s": min(tp), "dense_all_s": td, "pruned_all_s": tp,
          "dense_Mrows_s": rows / min(td) / 1e6, "pruned_Mrows_s": rows / min(tp) / 1e6, "pruned_over_dense_time": min(tp) / min(td),
          "bytes_compact_dense": int(cd.bytes_compact), "bytes_compact_pruned": int(cp.bytes_compact),
          "kept_share": pi.kept / n, "begin_dense_host_s": min(bd), "begin_pruned_host_s": min(bp), "begin_dense_all_s": bd, "begin_pruned_all_s": bp,
          "accuracy_all_turns": acc, "check_rows": chk["rows"], "check_ids": len(chk["ids"]), "check_ids_kept": chk_kept,
          "check_max_abs_diff_dense": err_d, "check_max_abs_diff_pruned": err_p,
          "compact_dense": struct_dict(cd), "compact_pruned": struct_dict(cp), "prune": struct_dict(pi)}, out)
    h.close()
    capi.release_cached_memory()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,headline")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "compact_pruned_rate.jsonl"))
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("compact_pruned_rate.py needs a HIP device: nothing here is measured on a CPU")
    if a.out and os.path.exists(a.out):
        os.remove(a.out)                                                   # one file, one run
    for name in a.shapes.split(","):
        rate(name, a.reps, a.out)


if __name__ == "__main__":
    main()
