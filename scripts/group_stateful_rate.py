"""AdaGrad and FTRL over feature shards (fmx_group_adapt_epoch / fmx_group_ftrl_epoch) on ONE MI355X: what a sharded epoch costs at the
batches the per-coordinate rules allow, next to the plain sharded rule at the batch its stability cut leaves.

    python scripts/group_stateful_rate.py [--features N] [--rows R] [--reps 3] [--out FILE]

Eight loopback shards on device 0 hold BASELINE configs[2]'s model -- Criteo-shaped rows (fmx_synth_rows_ex(FMX_SYNTH_CRITEO), 39
entries per row), k = 64, classification, learn_rate 0.01; --features scales the 3.3e7 features down where the memory is short.  Per
rule, AdaGrad then FTRL, and per batch 512, 4 096 and 65 536: parameters reset, session begun, one warm-up epoch (it also buckets the
rows for the batch size), then --reps epochs; the fastest by wall clock is reported as examples/s, with the device seconds of the
same epoch (HIP events on shard 0's stream around the whole epoch).  In the same run fmx_group_sgd_epoch with batch 0 -- its
stability cut -- under the bias-lag schedule the driver picks its in-stream form for.

Loopback serialises on one device what eight GPUs would do in parallel -- the eight partial sums, the eight updates and the eight
REDUNDANT bias recurrences of a batch -- and its exchange is a local reduction kernel, not a wire: the figures say what the schedule
costs the host and one device, not what eight devices would reach.  Nothing here runs on more than one GPU.

launches per batch are counted from the driver's code, not measured: per shard the partial sums, rest_e, the recurrence (one launch;
batches beyond 4 096 rows that take the parallel-in-time form add a memset node per piece) and the owner kernel, plus the one
reduction kernel of the loopback exchange.

Last, one timed AdaGrad epoch at batch 4 096 is held against ONE unsharded handle given the same start values and the same call: the
bias, 65 536 sampled parameter rows and every prediction at rtol 1e-4 (atol 2e-5 on parameters, 1e-4 on predictions).
Prints one JSON line per measurement (and appends them to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libfm_amd import capi  # noqa: E402

WORLD, K, NNZ, LR = 8, 64, 39, 0.01
REG = (0.0, 0.0, 0.001)
ADAGRAD = dict(init_acc=1.0, learn_rate=LR)
FTRL = dict(alpha=LR, beta=1.0, l1_w=0.01, l1_v=0.0, l2_w=0.0, l2_v=0.001, init_acc=0.0)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def make_group(n, rows):
    hs = [capi.Handle(n, K, True, True, capi.TASK_CLASSIFICATION, REG[0], REG[1], REG[2], LR, -1.0, 1.0, device=0, shard_rank=r,
                      shard_world=WORLD, shard_hash=1) for r in range(WORLD)]
    for h in hs:
        h.synth_rows(0, 123, 0, rows, NNZ, capi.SYNTH_CRITEO)
    return hs, capi.Group(hs)


def reset(hs):
    for h in hs:
        h.init_params(0.0, 0.05, 19)


def timed(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        st = fn()
        wall = time.perf_counter() - t0
        if best is None or wall < best[0]:
            best = (wall, st)
    return best


def launches(st, world):
    """launches of one batch, from the driver's code: per shard 4 (+ a memset node where the recurrence ran parallel in time), + 1 exchange"""
    per_shard = 4 + (1 if st.status & capi.STAT_SCAN_PIT else 0)
    return per_shard, per_shard * world + 1


def rates(n, rows, reps, out):
    hs, grp = make_group(n, rows)
    try:
        for rule in ("adagrad", "ftrl"):
            for batch in (512, 4096, 65536):
                reset(hs)
                if rule == "adagrad":
                    grp.adapt_begin("adagrad", ADAGRAD["init_acc"], ADAGRAD["learn_rate"])
                    run = lambda: grp.adapt_epoch(0, batch, 0)      # noqa: E731
                else:
                    grp.ftrl_begin(**FTRL)
                    run = lambda: grp.ftrl_epoch(0, batch, 0)       # noqa: E731
                warm = run()
                wall, st = timed(run, reps)
                per_shard, per_batch = launches(st, WORLD)
                emit({"what": "rate", "rule": rule, "shards": WORLD, "features": n, "factors": K, "rows": rows, "batch": batch,
                      "batches": int(st.batches), "w0_chunk": int(st.w0_chunk_used), "wall_s": wall, "device_s": st.device_seconds,
                      "Mex_s": rows / wall / 1e6, "setup_s_warmup": warm.setup_seconds, "status": int(st.status),
                      "launches_per_shard_and_batch": per_shard, "launches_per_batch": per_batch, "reps": reps}, out)
                (grp.adapt_end if rule == "adagrad" else grp.ftrl_end)()
        reset(hs)
        run = lambda: grp.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_DEFAULT, 0, 0, capi.FLAG_BIAS_LAG, 2)   # noqa: E731
        run()
        wall, st = timed(run, reps)
        emit({"what": "rate", "rule": "sgd", "shards": WORLD, "features": n, "factors": K, "rows": rows, "batch": int(st.batch_used),
              "batches": int(st.batches), "w0_chunk": int(st.w0_chunk_used), "wall_s": wall, "device_s": st.device_seconds,
              "Mex_s": rows / wall / 1e6, "collision_mass": st.collision_mass, "status": int(st.status), "reps": reps}, out)
    finally:
        grp.close()
        for h in hs:
            h.close()


def parity(n, rows, out):
    """one timed sharded AdaGrad epoch at batch 4 096 against one unsharded handle: same start values, same call"""
    batch = 4096
    hs, grp = make_group(n, rows)
    rng = np.random.default_rng(7)
    ids = np.unique(rng.integers(0, n, 65536)).astype(np.uint32)
    try:
        reset(hs)
        grp.adapt_begin("adagrad", ADAGRAD["init_acc"], ADAGRAD["learn_rate"])
        t0 = time.perf_counter()
        st = grp.adapt_epoch(0, batch, 0)
        wall = time.perf_counter() - t0
        owner, _ = capi.shard_place(n, WORLD, 1, ids)
        w, v = np.zeros(len(ids)), np.zeros((K, len(ids)))
        for r, h in enumerate(hs):
            sel = np.flatnonzero(owner == r)
            if len(sel):
                w[sel], v[:, sel] = h.get_param_rows(ids[sel])
        w0, pred = hs[0].get_w0(), grp.predict(0, rows)
        grp.adapt_end()
    finally:
        grp.close()
        for h in hs:
            h.close()
    one = capi.Handle(n, K, True, True, capi.TASK_CLASSIFICATION, REG[0], REG[1], REG[2], LR, -1.0, 1.0, device=0)
    try:
        one.init_params(0.0, 0.05, 19)
        one.synth_rows(0, 123, 0, rows, NNZ, capi.SYNTH_CRITEO)
        one.adapt_begin("adagrad", ADAGRAD["init_acc"], ADAGRAD["learn_rate"])
        st1 = one.adapt_epoch(0, batch, 0)
        w1, v1 = one.get_param_rows(ids)
        w01, pred1 = one.get_w0(), one.predict(0, rows)
        start = capi.Handle(n, K, device=0)
        start.init_params(0.0, 0.05, 19)
        _, v_start = start.get_param_rows(ids)
        start.close()
    finally:
        one.close()
    gap = {"w0": abs(w0 - w01), "w": float(np.abs(w - w1).max()), "v": float(np.abs(v - v1).max()), "pred": float(np.abs(pred - pred1).max())}
    ok = bool(abs(w0 - w01) <= 1e-4 * abs(w01) + 2e-5 and np.allclose(w, w1, rtol=1e-4, atol=2e-5) and np.allclose(v, v1, rtol=1e-4, atol=2e-5)
              and np.allclose(pred, pred1, rtol=1e-4, atol=1e-4))
    emit({"what": "parity", "rule": "adagrad", "batch": batch, "shards": WORLD, "rows": rows, "sampled_ids": int(len(ids)), "gaps": gap,
          "moved_v": float(np.abs(v1 - v_start).max()), "wall_s": wall, "single_handle_device_s": st1.device_seconds,
          "group_device_s": st.device_seconds, "ok": ok}, out)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=33_000_000)
    ap.add_argument("--rows", type=int, default=1 << 19)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("group_stateful_rate.py needs a HIP device: nothing here is measured on a CPU")
    rates(a.features, a.rows, a.reps, a.out)
    if not parity(a.features, a.rows, a.out):
        raise SystemExit("the sharded epoch and the single handle disagree beyond 1e-4")


if __name__ == "__main__":
    main()
