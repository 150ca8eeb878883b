"""The routes of the SGD epoch drivers (libfm_amd/csrc/fmx_sgd.hip, fmx_comm.hip), one small configuration each.

Which kernels an epoch of the batch rule enqueues depends on the mode, the apply form, the batch (32 768 rows: the recurrence gets its own
stream), the bias lag, the micro-chunk, the row length, the factor count and a handful of switches read from the environment.  CONFIGS
names the smallest shapes that reach each of them: 20 000 attributes, 4 entries per row (24 for the masked second pass), k = 8 (64 where the
route needs a wave-wide row).  run() trains one configuration and returns the last epoch's stats and the parameters;
tests/test_gpu_schedules.py holds every configuration to its counts, its status bits and the oracle's rule, scripts/epoch_fingerprint.py
prints a hash of the parameters per configuration (the record of a before / after comparison of the drivers)."""
import os

import datagen

N_ATTR = 20000
LR = 0.01
STDEV = 0.05
INIT_SEED = 7
FLAG_BIAS_LAG, FLAG_PIPELINE, FLAG_KEEP_WSIDE = 2, 4, 32
SEQUENTIAL, MINIBATCH, HOGWILD = 0, 1, 2
DEFAULT, ATOMIC, STORE, SEGMENTED, FUSED = 0, 1, 2, 3, 4
STAT_SCAN_PIT, STAT_SCAN_SERIAL, STAT_SCAN_FALLBACK, STAT_EVENT_SYNC, STAT_HANDOFF_TIMEOUT, STAT_SMALL_ONE = 4, 8, 16, 32, 64, 512
ROUTE_MASK = STAT_SCAN_PIT | STAT_SCAN_SERIAL | STAT_SMALL_ONE | STAT_EVENT_SYNC
KNOBS = ("FMX_SMALL_ONE", "FMX_SCAN", "FMX_GROUP_IN_STREAM")


def cfg(name, kind="single", mode=MINIBATCH, apply=FUSED, batch=512, rows=1300, nnz=4, k=8, chunk=0, flags=0, lag=0, env=None,
        epochs=2, deterministic=True, oracle=True, world=1):
    return dict(name=name, kind=kind, mode=mode, apply=apply, batch=batch, rows=rows, nnz=nnz, k=k, chunk=chunk, flags=flags, lag=lag,
                env=dict(env or {}), epochs=epochs, deterministic=deterministic, oracle=oracle and deterministic, world=world)


BIG = 2 * 32768 + 100
CONFIGS = [
    # one handle, the one-pass form
    cfg("fused_side_handoff_lag2", batch=32768, rows=BIG, lag=2),            # side stream, device-side hand-off (or events), PIT scan
    cfg("fused_side_events_lag1", batch=32768, rows=BIG, lag=1),             # side stream, events
    cfg("fused_two_launches_b2048", batch=2048, rows=5000, lag=2),           # in-stream, two launches per batch
    cfg("fused_small_one_b512", batch=512, rows=1300, lag=2),                # one launch per batch
    cfg("fused_small_one_off_b512", batch=512, rows=1300, lag=2, env={"FMX_SMALL_ONE": "0"}),
    cfg("fused_keep_wside_b512", batch=512, rows=1300, lag=2, flags=FLAG_KEEP_WSIDE),
    cfg("fused_chunk48_serial_scan", batch=32768, rows=BIG, lag=2, chunk=48),                                 # k_scan
    cfg("fused_chunk256_tiled_scan", batch=32768, rows=BIG, lag=2, chunk=256, env={"FMX_SCAN": "serial"}),    # k_scan1
    cfg("fused_small_one_k64", batch=512, rows=1300, lag=2, k=64),
    # one handle, the split step
    cfg("default_b2048", apply=DEFAULT, batch=2048, rows=5000),
    cfg("default_lag_b2048", apply=DEFAULT, batch=2048, rows=5000, flags=FLAG_BIAS_LAG),
    cfg("segmented_b2048", apply=SEGMENTED, batch=2048, rows=5000),
    cfg("segmented_lag_b2048", apply=SEGMENTED, batch=2048, rows=5000, flags=FLAG_BIAS_LAG),
    # FMX_APPLY_STORE loses updates where ids collide inside a batch (include/fmx.h: "exact when a batch has no repeated feature"; these
    # batches repeat most of theirs), so no oracle states its numbers: tests/test_gpu_parity.py holds it to one on collision-free rows only
    cfg("store_b2048", apply=STORE, batch=2048, rows=5000, oracle=False),
    cfg("store_lag_b2048", apply=STORE, batch=2048, rows=5000, flags=FLAG_BIAS_LAG, oracle=False),
    cfg("segmented_masked_nnz24", apply=SEGMENTED, batch=2048, rows=5000, nnz=24),                            # k_fused<FUSED_APPLY>
    cfg("default_lag_k64", apply=DEFAULT, batch=2048, rows=5000, k=64, flags=FLAG_BIAS_LAG),
    cfg("sgda_minibatch", kind="sgda", apply=DEFAULT, batch=2048, rows=5000, chunk=16, epochs=1),             # the dense segment list
    # loopback group of two shards (k = 64: k_apply_multi)
    cfg("group_in_stream_b512", kind="group", apply=DEFAULT, k=64, world=2, flags=FLAG_BIAS_LAG, lag=2),
    cfg("group_general_b512", kind="group", apply=DEFAULT, k=64, world=2, flags=FLAG_BIAS_LAG, lag=2, env={"FMX_GROUP_IN_STREAM": "0"}),
    cfg("group_pipeline_b512", kind="group", apply=DEFAULT, k=64, world=2, flags=FLAG_BIAS_LAG | FLAG_PIPELINE, lag=2),
    cfg("group_side_b40000_lag2", kind="group", apply=DEFAULT, k=64, world=2, batch=40000, rows=2 * 40000 + 100, flags=FLAG_BIAS_LAG, lag=2),
    cfg("group_exact_b512", kind="group", apply=DEFAULT, k=64, world=2),                                      # no lag: k_apply_multi<false>
    # asynchronous forms: counts only
    cfg("hogwild_store", mode=HOGWILD, apply=STORE, batch=512, rows=1300, deterministic=False),
    cfg("minibatch_atomic_b2048", apply=ATOMIC, batch=2048, rows=5000, deterministic=False),
]
BY_NAME = {c["name"]: c for c in CONFIGS}


def event_sync_masked(c):
    """FMX_STAT_EVENT_SYNC says whether the device ran the handle's two streams side by side when the epoch asked: not a property of the route"""
    return c["lag"] >= 2 and c["batch"] >= 32768


def route_bits(c, status):
    mask = ROUTE_MASK & ~(STAT_EVENT_SYNC if event_sync_masked(c) else 0)
    return int(status) & mask


_DATA = {}


def data(c):
    key = (c["rows"], c["nnz"])
    if key not in _DATA:
        _DATA[key] = datagen.onehot_fields(N_ATTR, c["nnz"], c["rows"], seed=1000 + c["nnz"])
    return _DATA[key]


def run(capi, c):
    """train `c` from init_params; returns (stats of the last epoch, (w0, w, v))"""
    ent, rp, y = data(c)
    saved = {kn: os.environ.get(kn) for kn in KNOBS}
    for kn in KNOBS:
        os.environ.pop(kn, None)
    os.environ.update(c["env"])
    hs, grp = [], None
    try:
        regw, regv = (0.0, 0.0) if c["kind"] == "sgda" else (0.001, 0.002)     # (SGDA learns its own regularisation)
        for r in range(c["world"]):
            hs.append(capi.Handle(N_ATTR, c["k"], True, True, capi.TASK_CLASSIFICATION, 0.0, regw, regv, LR, -1.0, 1.0,
                                  shard_rank=r, shard_world=c["world"], shard_hash=1 if c["world"] > 1 else 0))
        for h in hs:
            h.init_params(0.0, STDEV, INIT_SEED)
        if c["kind"] == "group":
            grp = capi.Group(hs)
            grp.upload_rows(0, ent, rp, y)
            for _ in range(c["epochs"]):
                st = grp.sgd_epoch(0, c["mode"], c["apply"], c["batch"], c["chunk"], c["flags"], c["lag"])
            params = grp.get_params()
        elif c["kind"] == "sgda":
            h = hs[0]
            h.upload_rows(0, ent, rp, y)
            h.upload_rows(1, ent[:int(rp[1000])], rp[:1001], y[:1000])
            h.sgda_begin()
            for i in range(c["epochs"]):
                st = h.sgda_epoch_minibatch(0, 1, i > 0, c["batch"], c["chunk"])
            params = h.get_params()
            h.sgda_end()
        else:
            h = hs[0]
            h.upload_rows(0, ent, rp, y)
            for _ in range(c["epochs"]):
                st = h.sgd_epoch(0, c["mode"], c["apply"], c["batch"], c["chunk"], c["flags"], c["lag"])
            params = h.get_params()
    finally:
        if grp is not None:
            grp.close()
        for h in hs:
            h.close()
        for kn, val in saved.items():
            os.environ.pop(kn, None)
            if val is not None:
                os.environ[kn] = val
    return st, params


def oracle_params(O, c, chunk_used):
    """the oracle call tests/test_gpu_parity.py (test_gpu_group.py, test_gpu_sgda.py) holds the same rule to"""
    ent, rp, y = data(c)
    d = O.Data(ent, rp, y)
    m = O.Model(N_ATTR, c["k"], True, True, 0.0, 0.001, 0.002)
    m.v[:] = O.init_values(INIT_SEED, N_ATTR, c["k"], STDEV)
    if c["kind"] == "sgda":
        m.reg0 = m.regw = m.regv = 0.0                                     # (the learner owns the regularisation)
        va = O.Data(ent[:int(rp[1000])], rp[:1001], y[:1000])
        O.sgda_learn(m, d, va, 1, LR, -1.0, 1.0, c["epochs"], None, batch=c["batch"], w0_chunk=c["chunk"])
        return m
    lag = (c["lag"] or 1) if (c["apply"] == FUSED or c["flags"] & FLAG_BIAS_LAG) else 0
    for _ in range(c["epochs"]):
        O.sgd_epoch_minibatch(m, d, 1, LR, -1.0, 1.0, c["batch"], chunk_used, bias_lag=lag, pipelined=bool(c["flags"] & FLAG_PIPELINE))
    return m
