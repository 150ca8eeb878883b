"""The id-only entry stream of unit-valued fixed-length slots (Slot::ids, load_entry in libfm_amd/csrc/fmx_kernels.h).

Where every value of a slot is 1.0f and every row has the same length, k_fused reads 4-byte ids and takes
the value as the constant.  The arithmetic sees the same operands, so a handle created with FMX_IDS=0 (entries) ends on the same bytes: row
lengths 1, 8, 32, 64 at k = 8, 64, 128, row counts that are no multiple of 4, a partial last batch; slots that miss the condition by ONE
value or ONE row; a unit-valued slot replaced by one that is not (a stale stream would read its values as 1); HOGWILD by counts and status,
as scripts/epoch_fingerprint.py holds the asynchronous forms."""
import os

import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

LR, STDEV, SEED = 0.01, 0.05, 7
SIDE = 32768                      # FMX_SIDE_STREAM_BATCH: the smallest batch whose recurrence gets the side stream
FUSED_B = 2048                    # two launches per batch: above the one-launch form's 1 024 rows, so the example pass is k_fused


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import capi as c
    if c.load().fmx_device_count() == 0:
        pytest.skip("no HIP device")
    return c


_DATA = {}


def rows(n, nnz, n_rows):
    key = (n, nnz, n_rows)
    if key not in _DATA:
        ent, rp, y = datagen.onehot_fields(n, nnz, n_rows, seed=300 + nnz)
        for a in (ent, rp, y):
            a.setflags(write=False)
        _DATA[key] = (ent, rp, y)
    return _DATA[key]


def handle(capi, n, k, env):
    """a handle created under `env` (the switches are read by fmx_create)"""
    knobs = ("FMX_IDS", "FMX_SCAN", "FMX_HANDOFF")
    saved = {kn: os.environ.pop(kn, None) for kn in knobs}
    os.environ.update(env)
    try:
        h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.001, 0.002, LR, -1.0, 1.0)
    finally:
        for kn in knobs:
            os.environ.pop(kn, None)
            if saved[kn] is not None:
                os.environ[kn] = saved[kn]
    h.init_params(0.0, STDEV, SEED)
    return h


def train(capi, n, k, data, env, epochs=2, mode=None, apply=None, batch=FUSED_B, flags=0, lag=2, uploads=None):
    """`epochs` epochs over `data`; uploads: further (entries, row_ptr, target) that REPLACE the slot, one more epoch each"""
    h = handle(capi, n, k, env)
    try:
        mode = capi.SGD_MINIBATCH if mode is None else mode
        apply = capi.APPLY_FUSED if apply is None else apply
        stats = []
        for d in [data] + list(uploads or []):
            h.upload_rows(0, *d)
            for _ in range(epochs if d is data else 1):
                stats.append(h.sgd_epoch(0, mode, apply, batch, 0, flags, lag))
        return stats, h.get_params()
    finally:
        h.close()


def same_bytes(a, b):
    (w0a, wa, va), (w0b, wb, vb) = a, b
    assert np.float64(w0a).tobytes() == np.float64(w0b).tobytes(), (w0a, w0b)
    assert wa.tobytes() == wb.tobytes(), "w: %d elements differ" % int((wa != wb).sum())
    assert va.tobytes() == vb.tobytes(), "V: %d elements differ" % int((va != vb).sum())


# ---- the large-batch launches of the headline's schedule --------------------------------------------------------------------------------
SIDE_ROWS = 3 * SIDE + 1000        # four batches, the last one partial


@pytest.mark.parametrize("k,nnz,n,lag,scan", [(8, 8, 50000, 2, None), (8, 8, 50000, 3, None), (64, 32, 200000, 2, None),
                                               (64, 32, 200000, 3, None), (8, 8, 50000, 2, "serial")])
def test_ids_stream_side_stream_both_orderings(capi, k, nnz, n, lag, scan):
    """batch 32 768 (the recurrence on the side stream): the id stream under the device-side hand-off ends on the bytes of the entry stream
    under events (FMX_FLAG_EVENT_SYNC) -- neither the stream k_fused reads nor the ordering of the two streams moves a number"""
    data = rows(n, nnz, SIDE_ROWS)
    env = {"FMX_SCAN": scan} if scan else {}
    stats, got = train(capi, n, k, data, env, batch=SIDE, lag=lag)
    for st in stats:
        assert not st.status & (capi.STAT_HANDOFF_TIMEOUT | capi.STAT_SCAN_FALLBACK), hex(int(st.status))
        assert st.status & (capi.STAT_SCAN_SERIAL if scan else capi.STAT_SCAN_PIT), hex(int(st.status))
        assert st.batches == 4
    ev_stats, want = train(capi, n, k, data, dict(env, FMX_IDS="0"), batch=SIDE, lag=lag, flags=capi.FLAG_EVENT_SYNC)
    assert all(st.status & capi.STAT_EVENT_SYNC for st in ev_stats)
    same_bytes(got, want)


# ---- the id-only stream -------------------------------------------------------------------------------------------------------------------
IDS_ROWS = 2 * FUSED_B + 1237      # three batches, the last one partial; 5 333 rows: no multiple of 4
IDS_N = 20000


def twin(capi, n, k, data, **kw):
    """the same training on a default handle and on one that keeps the entry stream (FMX_IDS=0)"""
    a = train(capi, n, k, data, {}, **kw)
    b = train(capi, n, k, data, {"FMX_IDS": "0"}, **kw)
    return a, b


@pytest.mark.parametrize("k", [8, 64, 128])
@pytest.mark.parametrize("nnz", [1, 8, 32, 64])
def test_ids_stream_same_bytes(capi, k, nnz):
    (sa, pa), (sb, pb) = twin(capi, IDS_N, k, rows(IDS_N, nnz, IDS_ROWS))
    assert [int(s.deferred_features) for s in sa] == [int(s.deferred_features) for s in sb]
    assert not sa[-1].status & capi.STAT_SMALL_ONE and sa[-1].batches == 3      # (k_fused, not the one-launch form, ran the examples)
    same_bytes(pa, pb)


def test_ids_stream_side_stream_batch(capi):
    """the large-batch launches of the headline's schedule: batch 32 768 with a partial second batch, k = 64, 32 entries per row"""
    (sa, pa), (sb, pb) = twin(capi, 200000, 64, rows(200000, 32, SIDE + 1001), batch=SIDE)
    assert not sa[-1].status & capi.STAT_HANDOFF_TIMEOUT
    same_bytes(pa, pb)


@pytest.mark.parametrize("k,nnz", [(8, 8), (64, 32)])
def test_one_value_or_one_row_off_takes_the_entries(capi, k, nnz):
    ent, rp, y = rows(IDS_N, nnz, IDS_ROWS)
    half = ent.copy()
    half["value"][len(half) // 2 + 3] = 0.5                               # ONE value that is not 1
    (_, pa), (_, pb) = twin(capi, IDS_N, k, (half, rp, y))
    same_bytes(pa, pb)
    # the same values read as 1 would give other numbers: the unit-valued rows do
    _, unit = train(capi, IDS_N, k, (ent, rp, y), {})
    assert unit[2].tobytes() != pa[2].tobytes()
    if nnz > 1:                                                            # ONE row one entry shorter: no fixed length
        r = IDS_ROWS // 3
        cut = int(rp[r + 1]) - 1
        ent2 = np.concatenate([ent[:cut], ent[cut + 1:]])
        rp2 = rp.copy()
        rp2[r + 1:] -= np.uint64(1)
        (_, pa), (_, pb) = twin(capi, IDS_N, k, (ent2, rp2, y))
        same_bytes(pa, pb)


def test_upload_replaces_the_stream(capi):
    """a unit-valued slot, an epoch, then fmx_upload_rows of rows with other values into the same slot: the next epoch reads THEIR values"""
    k, nnz = 64, 8
    ent, rp, y = rows(IDS_N, nnz, IDS_ROWS)
    other = ent.copy()
    other["value"] = (0.5 + np.arange(len(other)) % 4 * 0.25).astype(np.float32)
    (_, pa), (_, pb) = twin(capi, IDS_N, k, (ent, rp, y), epochs=1, uploads=[(other, rp, y), (ent, rp, y)])
    same_bytes(pa, pb)


def test_ids_stream_hogwild_counts(capi):
    """HOGWILD (k_fused<FUSED_STORE>): rows in flight race, so counts and status only, and every parameter a number"""
    (sa, pa), (sb, pb) = twin(capi, IDS_N, 64, rows(IDS_N, 32, IDS_ROWS), mode=capi.SGD_HOGWILD, apply=capi.APPLY_STORE, batch=512, lag=0)
    for x, y_ in zip(sa, sb):
        assert (int(x.batches), int(x.main_kernel_launches), int(x.status)) == (int(y_.batches), int(y_.main_kernel_launches), int(y_.status))
    for p in (pa, pb):
        assert np.isfinite(p[0]) and np.isfinite(p[1]).all() and np.isfinite(p[2]).all()
