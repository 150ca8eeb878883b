"""The bits the read side returns: one SHA-256 per case and entry point over the raw bytes of what it returns (timing fields left out)
-- to be run on two builds of the library (before and after a change to row_sums, k_rowsums, k_fetch_rows, the row sources, slot_scores
or the reductions behind the evaluate entry points) and compared line by line.  Not a test and no hash is an expected value: a
compiler update may move them.

    python scripts/score_bits.py [--out FILE] [--label NAME]          (another build: FMX_LIB=<path of its libfmx.so>)

Cases:
  widths : the 47-row slots of tests/test_gpu_compact.py (make_rows / make_params) at every (k, n, k1, task) of its CASES.  Per case
           predict, evaluate, evaluate_ex (both links), evaluate_by_query with the per-query arrays (five queries); post_accumulate of
           three draws (the model moved between them) with burn_in 1, then post_get and post_evaluate_ex of the three vectors;
           compact_predict / _evaluate / _evaluate_ex / _topk (the slot against itself, K = 5) / _rows; get_param_rows of every
           feature; adapt_state_rows and ftrl_state_rows after one epoch (batch 16, micro-chunk 4); and, where n > 1, predict,
           evaluate_ex and evaluate_by_query of a two-shard loopback group
  blocks : one slot with a kept relation block (k 8): predict, evaluate, evaluate_ex and the three draws of the accumulator as above
  wside  : one slot whose weight side stream is current, i.e. after a FMX_FLAG_KEEP_WSIDE epoch (k 8, 3000 features, 1200 rows):
           predict, evaluate, evaluate_ex, evaluate_by_query, post_accumulate; the line says whether FMX_EVAL_WSIDE was reported
Prints one JSON line per case and entry point (and appends them to --out)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from libfm_amd import capi  # noqa: E402

TIMING = ("device_seconds", "rank_seconds")


def flat(x):
    """what a call returned as a list of arrays: structs field by field without the timing fields, tuples item by item"""
    if isinstance(x, C.Structure):
        return [a for f, _ in x._fields_ if f not in TIMING for a in flat(getattr(x, f))]
    if isinstance(x, C.Array):
        return [a for item in x for a in flat(item)]
    if isinstance(x, (tuple, list)):
        return [a for item in x for a in flat(item)]
    return [np.ascontiguousarray(x)]


def digest(x):
    h = hashlib.sha256()
    for a in flat(x):
        h.update(str(a.dtype).encode() + a.tobytes())
    return h.hexdigest()


def call(fn, *args, **kw):
    """the call's result, or its refusal (a refusal is part of the behaviour, too)"""
    try:
        return fn(*args, **kw)
    except capi.FmxError as e:
        return ("refused", np.int64(e.code))


def read_side(emit, tag, h, rows, cls, queries=True):
    """the fp32 entry points on slot 0 of a handle or a group"""
    emit(tag, "predict", call(h.predict, 0, rows))
    if isinstance(h, capi.Handle):
        emit(tag, "evaluate", call(h.evaluate, 0))
    for name, link in (("logistic", capi.LINK_LOGISTIC), ("probit", capi.LINK_PROBIT)) if cls else (("logistic", capi.LINK_LOGISTIC),):
        emit(tag, "evaluate_ex " + name, call(h.evaluate_ex, 0, link))
    if queries:
        emit(tag, "evaluate_by_query", call(h.evaluate_by_query, 0, capi.LINK_LOGISTIC, True))


def post(emit, tag, h, rows, params):
    w0, w, v = params
    h.post_begin(0, burn_in=1)
    for d in range(3):
        h.set_params(w0 + 0.1 * d, w * (1.0 - 0.2 * d), v * (1.0 + 0.1 * d))
        emit(tag, "post_accumulate draw %d" % d, call(h.post_accumulate, 0))
    for which in (capi.POST_THIS, capi.POST_ALL, capi.POST_LATE):
        emit(tag, "post_get %d" % which, call(h.post_get, 0, which, rows))
        emit(tag, "post_evaluate_ex %d" % which, call(h.post_evaluate_ex, 0, which))
    h.post_end(0)
    h.set_params(w0, w, v)


def state_rows(h, rule, ids, params):
    """the optimiser's state rows after one epoch from the start values"""
    h.set_params(*params)
    if rule == "adapt":
        h.adapt_begin("adagrad", 1.0, 0.05)
    else:
        h.ftrl_begin(0.05, 1.0, 0.001, 0.001, 0.01, 0.01, 0.0)
    try:
        getattr(h, rule + "_epoch")(0, 16, 4)
        return getattr(h, rule + "_state_rows")(ids)
    finally:
        getattr(h, rule + "_end")()


def widths(emit):
    import test_gpu_compact as G
    for (k, n, k1, task), name in zip(G.CASES, G.IDS):
        ent, rp, y = G.make_rows(n, 10 + k, task)
        params = G.make_params(n, k, k + 1)
        qid = np.arange(G.ROWS, dtype=np.uint32) % 5
        ids = np.arange(n, dtype=np.uint32)
        h = G.handle(capi, n, k, k1, task, params, lr=0.05)
        try:
            h.upload_rows(0, ent, rp, y)
            h.set_row_queries(0, qid)
            read_side(emit, name, h, G.ROWS, task == 1)
            post(emit, name, h, G.ROWS, params)
            emit(name, "get_param_rows", call(h.get_param_rows, ids))
            h.compact_begin()
            emit(name, "compact_predict", call(h.compact_predict, 0, G.ROWS))
            emit(name, "compact_evaluate", call(h.compact_evaluate, 0))
            emit(name, "compact_evaluate_ex", call(h.compact_evaluate_ex, 0))
            emit(name, "compact_topk", call(h.compact_topk, 0, 0, 5))
            emit(name, "compact_rows", call(h.compact_rows, ids))
            h.compact_end()
            emit(name, "adapt_state_rows", call(state_rows, h, "adapt", ids, params))
            emit(name, "ftrl_state_rows", call(state_rows, h, "ftrl", ids, params))
        finally:
            h.close()
        if n > 1:
            hs = [G.handle(capi, n, k, k1, task, None, device=0, shard_rank=r, shard_world=2, shard_hash=1) for r in range(2)]
            grp = capi.Group(hs)
            try:
                grp.set_params(*params)
                grp.upload_rows(0, ent, rp, y)
                grp.set_row_queries(0, qid)
                read_side(emit, name + " group of 2", grp, G.ROWS, task == 1)
            finally:
                grp.close()
                for m in hs:
                    m.close()


def blocks(emit):
    import test_gpu_compact as G
    k, n = 8, 200
    params = G.make_params(n, k, 5)
    main = np.zeros(6, dtype=capi.ENTRY_DTYPE)
    main["id"], main["value"] = np.arange(6), 1.0
    bent = np.zeros(3, dtype=capi.ENTRY_DTYPE)
    bent["id"], bent["value"] = np.arange(3), 0.5
    rel = [(bent, np.arange(4, dtype=np.uint64), np.array([0, 1, 2, 0, 1, 2], dtype=np.uint32), 10)]
    h = G.handle(capi, n, k, True, 1, params)
    try:
        h.upload_block_rows(0, main, np.arange(7, dtype=np.uint64), np.array([1, -1, 1, -1, -1, 1], np.float32), rel, keep=True)
        read_side(emit, "kept block k8", h, 6, True, queries=False)
        post(emit, "kept block k8", h, 6, params)
    finally:
        h.close()


def wside(emit):
    import datagen
    from oracle import oracle as O
    n, k, nnz, rows = 3000, 8, 6, 1200
    ent, rp, y = datagen.onehot_fields(n, nnz, rows, seed=5, classification=True)
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.001, 0.002, 0.01, -1.0, 1.0)
    try:
        h.set_params(0.0, O.init_values(10, n, 1, 0.05)[0], O.init_values(9, n, k, 0.05))
        h.upload_rows(0, ent, rp, y)
        h.set_row_queries(0, np.arange(rows, dtype=np.uint32) % 37)
        h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_FUSED, 256, 32, capi.FLAG_KEEP_WSIDE, 2)
        tag = "side stream k8 (FMX_EVAL_WSIDE %d)" % bool(h.evaluate(0).flags & capi.EVAL_WSIDE)
        read_side(emit, tag, h, rows, True)
        h.post_begin(0, burn_in=1)
        emit(tag, "post_accumulate", call(h.post_accumulate, 0))
        h.post_end(0)
    finally:
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="widths,blocks,wside")
    ap.add_argument("--out", default="")
    ap.add_argument("--label", default="", help="copied into every line (which build this is)")
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("score_bits.py needs a HIP device")

    def emit(case, entry, result):
        line = json.dumps({"label": a.label, "case": case, "entry": entry, "sha256": digest(result)})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for name, fn in (("widths", widths), ("blocks", blocks), ("wside", wside)):
        if name in a.cases.split(","):
            fn(emit)


if __name__ == "__main__":
    main()
