"""The bits the segment owners leave behind: one SHA-256 per case over the raw bytes of get_params() and, where the rule keeps state, of
every state row -- to be run on two builds of the library (before and after a change to apply_seg_block, seg_tail, the stateful owner
block or their drivers) and compared line by line.  Not a test and no hash is an expected value: a compiler update may move them.

    python scripts/owner_bits.py [--cases parity,hot,fused,sgda] [--out FILE] [--label NAME]

Cases (every one trains from seeded start values):
  parity   : tests/test_ftrl_cpu.parity_case(k) for k in 1, 8, 64, 100, 256, 1024 (6400 features, 512 rows of 32 entries), batch 64,
             micro-chunk 16, two epochs, regression and classification taking turns over k on purpose (a before-and-after comparison
             needs every width once, not every width under both tasks) -- AdaGrad, FTRL with the tests' PARITY options, and fmx_sgd_epoch(MINIBATCH, FMX_APPLY_SEGMENTED)
  hot      : tests/test_adagrad_cpu.hot_case (a segment of 512 occurrences: the tail past 64 descriptors, and a tail batch) at k 64 and 8,
             batch 512, micro-chunk 8, two epochs -- the same three rules
  fused    : fmx_sgd_epoch(MINIBATCH, FMX_APPLY_FUSED) on 2^18 device-generated rows at k 64 and 8, with bias_lag 2 (what bench.py passes):
             200 000 features, 32 entries per row, batches 512, 4 096 and 65 536 (the one-launch small batch, the deferred-feature pass
             that carries the recurrence, sixteen segments per wavefront); 800 000 and 1 600 000 features, 4 entries per row, batch
             32 768 (a short deferred list: four segments and one segment per wavefront); and with bias_lag 0 (the library's default:
             depth 1) at 200 000 features, batches 4 096 and 65 536
  sgda     : the batch form of tests/test_gpu_sgda.py::test_sgda_batch_form_mid_size (k 16, batch 1 024), the learned regularisation included
Prints one JSON line per case (and appends them to --out)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from libfm_amd import capi  # noqa: E402


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def handle_for(m, task, lr):
    h = capi.Handle(m.n, m.k, m.k0, m.k1, task, m.reg0, m.regw, m.regv, lr, -1.0, 1.0)
    h.set_params(m.w0, m.w, m.v)
    return h


def three_rules(d, m, task, lr, batch, chunk, opts):
    """{rule: hash} after two epochs of each rule from the same start"""
    ids = np.arange(m.n, dtype=np.uint32)
    out = {}
    for rule in ("sgd_segmented", "adagrad", "ftrl"):
        h = handle_for(m, task, lr)
        try:
            h.upload_rows(0, d.entries, d.row_ptr, d.target)
            if rule == "adagrad":
                h.adapt_begin("adagrad", 1.0, 0.05)
            elif rule == "ftrl":
                h.ftrl_begin(**opts)
            for _ in range(2):
                if rule == "sgd_segmented":
                    h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, batch, chunk)
                elif rule == "adagrad":
                    h.adapt_epoch(0, batch, chunk)
                else:
                    h.ftrl_epoch(0, batch, chunk)
            w0, w, v = h.get_params()
            state = () if rule == "sgd_segmented" else h.adapt_state_rows(ids) if rule == "adagrad" else h.ftrl_state_rows(ids)
            out[rule] = digest((np.float64(w0), w, v) + tuple(state))
        finally:
            h.close()
    return out


def fused(k, n, nnz, batch, lag):
    rows = 1 << 18
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0)
    try:
        h.init_params(0.0, 0.01, 1)
        h.synth_rows(0, 123, 0, rows, nnz)
        for _ in range(2):
            st = h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_FUSED, batch, 0, 0, lag)
        w0, w, v = h.get_params()
        return digest((np.float64(w0), w, v)), int(st.deferred_features), int(st.batches)
    finally:
        h.close()


def sgda():
    import datagen
    from oracle import oracle as O
    n, nnz, k, lr = 6400, 8, 16, 0.002
    ent, rp, y = datagen.onehot_fields(n, nnz, 20000, seed=3, classification=False)
    ev, rv, yv = datagen.onehot_fields(n, nnz, 5000, seed=4, classification=False)
    h = capi.Handle(n, k, True, True, 0, 0.0, 0.0, 0.0, lr, float(y.min()), float(y.max()))
    try:
        h.set_params(0.0, np.zeros(n), O.init_values(9, n, k, 0.05))
        h.upload_rows(0, ent, rp, y)
        h.upload_rows(1, ev, rv, yv)
        h.sgda_begin()
        for i in range(3):
            h.sgda_epoch_minibatch(0, 1, i > 0, 1024, 64)
        reg = h.sgda_get_reg()
        w0, w, v = h.get_params()
        h.sgda_end()
        return digest((np.float64(w0), w, v, reg))
    finally:
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="parity,hot,fused,sgda")
    ap.add_argument("--out", default="")
    ap.add_argument("--label", default="", help="copied into every line (which build this is)")
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("owner_bits.py needs a HIP device")
    from test_adagrad_cpu import hot_case
    from test_ftrl_cpu import PARITY, parity_case
    from oracle import oracle as O

    def emit(case, sha, **more):
        line = json.dumps(dict({"label": a.label, "case": case, "sha256": sha}, **more))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    cases = a.cases.split(",")
    if "parity" in cases:
        for i, k in enumerate((1, 8, 64, 100, 256, 1024)):
            d, m = parity_case(k)
            for rule, sha in three_rules(d, m, i % 2, 0.01, 64, 16, PARITY).items():  # (regression and classification take turns)
                emit("parity k=%d %s" % (k, rule), sha)
    if "hot" in cases:
        d, m8 = hot_case()
        for k in (64, 8):
            m = O.Model(m8.n, k, True, True, 0.0, 0.002, 0.001)
            m.v[:] = O.init_values(1, m.n, k, 0.05)
            for rule, sha in three_rules(d, m, 0, 0.05, 512, 8, PARITY).items():
                emit("hot k=%d %s" % (k, rule), sha)
    if "fused" in cases:
        for k in (64, 8):
            for n, nnz, batch, lag in ((200_000, 32, 512, 2), (200_000, 32, 4096, 2), (200_000, 32, 65536, 2), (800_000, 4, 32768, 2),
                                       (1_600_000, 4, 32768, 2), (200_000, 32, 4096, 0), (200_000, 32, 65536, 0)):
                sha, deferred, batches = fused(k, n, nnz, batch, lag)
                emit("fused k=%d n=%d nnz=%d batch=%d bias_lag=%d" % (k, n, nnz, batch, lag), sha, deferred_features_per_batch=deferred / max(batches, 1))
    if "sgda" in cases:
        emit("sgda batch form k=16 batch=1024", sgda())


if __name__ == "__main__":
    main()
