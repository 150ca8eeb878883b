"""The training-side weight stream of the one-pass minibatch step (Slot::wtrain, WTrain in libfm_amd/csrc/fmx_kernels.h).

A feature that occurs in exactly one entry of a slot (a "single") has its linear weight read and written by one lane of one wavefront, epoch
after epoch; that lane keeps a copy in a packed stream and reads the copy instead of gathering w[j].  w[j] is written all the same and the
copy is bit for bit what w[j] holds, so a handle created with FMX_WTRAIN=0 -- the control: same seeds, same calls -- ends on the same bytes.
Here: both routes of k_fused<EXACT> (two launches per batch in the stream; the side stream with its hand-off), row widths 8 / 32 / 64 / 112
floats, rows of exactly 64 entries, rows of 65-70 (two-pass branch: no singles), empty rows, values != 1, a row that repeats an id, slots
of singles only and of none, everything that makes the stream stale, the predict-side stream next to it, and the paths that never build it.
The device's count of singles is held against numpy's."""
import os

import numpy as np
import pytest

from datagen import ENTRY_DTYPE

pytestmark = pytest.mark.gpu

LR, STDEV, SEED = 0.01, 0.05, 11
REGW, REGV = 0.001, 0.001
LAG = 2
SIDE = 32768                      # FMX_SIDE_STREAM_BATCH: the smallest batch whose recurrence gets the side stream
FUSED_B = 2048                    # two launches per batch: above the one-launch form's 1 024 rows, so the example pass is k_fused
ROWS = 2 * FUSED_B + 1237         # three batches, the last one partial; 5 333 rows: no multiple of 4
SIDE_ROWS = 2 * SIDE + 4500       # three batches, the last one short
KNOBS = ("FMX_WTRAIN", "FMX_IDS", "FMX_SCAN", "FMX_HANDOFF", "FMX_SMALL_ONE")


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import capi as c
    if c.load().fmx_device_count() == 0:
        pytest.skip("no HIP device")
    return c


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------
def _targets(rng, n_rows):
    return np.where(rng.random(n_rows) < 0.5, -1.0, 1.0).astype(np.float32)


def _entries(ids, values=None):
    ent = np.zeros(len(ids), dtype=ENTRY_DTYPE)
    ent["id"] = ids
    ent["value"] = 1.0 if values is None else values
    return ent


def fixed_rows(n_rows, nnz, seed):
    """unit-valued rows of one length (the id-only stream is on); ids uniform over n = rows * nnz / 1.3: about 27 % of the entries are singles"""
    rng = np.random.default_rng(seed)
    n = int(n_rows * nnz / 1.3)
    ids = rng.integers(0, n, n_rows * nnz).astype(np.uint32)
    rp = np.arange(n_rows + 1, dtype=np.uint64) * np.uint64(nnz)
    return n, (_entries(ids), rp, _targets(rng, n_rows))


def ragged_rows(n_rows, seed, long_rows=True):
    """rows of 1-40 entries with values != 1 (no id-only stream), an empty row in every 50, rows of exactly 64 entries, rows of 65-70
    (long_rows), and one row that repeats an id"""
    rng = np.random.default_rng(seed)
    r = np.arange(n_rows)
    sizes = rng.integers(1, 41, n_rows)
    sizes[r % 50 == 7] = 0
    sizes[r % 97 == 3] = 64
    if long_rows:
        sizes[r % 101 == 5] = 65 + r[r % 101 == 5] % 6
    sizes[11] = 12                                               # (the row that repeats an id)
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    nnz = int(rp[-1])
    n = int(nnz / 1.3)
    ids = rng.integers(0, n, nnz).astype(np.uint32)
    ids[int(rp[11]) + 5] = ids[int(rp[11]) + 2]
    vals = (0.25 + 0.25 * rng.integers(0, 3, nnz)).astype(np.float32)     # 0.25, 0.5, 0.75
    return n, (_entries(ids, vals), rp, _targets(rng, n_rows))


def permutation_rows(n_rows, nnz, seed):
    """every id exactly once: every entry is a single"""
    rng = np.random.default_rng(seed)
    n = n_rows * nnz
    rp = np.arange(n_rows + 1, dtype=np.uint64) * np.uint64(nnz)
    return n, (_entries(rng.permutation(n).astype(np.uint32)), rp, _targets(rng, n_rows))


def twice_rows(n_rows, nnz, seed):
    """every id exactly twice: no entry is a single"""
    rng = np.random.default_rng(seed)
    n = n_rows * nnz // 2
    ids = np.concatenate([rng.permutation(n), rng.permutation(n)]).astype(np.uint32)
    rp = np.arange(n_rows + 1, dtype=np.uint64) * np.uint64(nnz)
    return n, (_entries(ids), rp, _targets(rng, n_rows))


def row_cap(k, max_row):
    """longest row the k_fused instance of a slot keeps in registers (fmx_sgd.hip fused_row_cap_kp)"""
    kp = 1
    while kp < k:
        kp *= 2
    vec = kp // 64 if kp >= 64 else 1
    epi = 64 // (kp // vec)
    need = -(-max_row // epi)
    zr = next((z for z in (8, 16, 32, 40, 64) if vec * z <= 128 and need <= z), 8)
    return min(64, zr * epi)


def numpy_singles(data, k):
    ent, rp, _ = data
    sizes = np.diff(rp.astype(np.int64))
    cap = row_cap(k, int(sizes.max()))
    cnt = np.bincount(ent["id"])
    row_of = np.repeat(np.arange(len(sizes)), sizes)
    return int(((cnt[ent["id"]] == 1) & (sizes[row_of] <= cap)).sum())


# ---- handles ------------------------------------------------------------------------------------------------------------------------------
def handle(capi, n, k, streamed, k1=True, regw=REGW, regv=REGV, **cfg):
    """a handle created with the stream on (the default) or off (FMX_WTRAIN=0: the control); the switch is read by fmx_create"""
    saved = {kn: os.environ.pop(kn, None) for kn in KNOBS}
    if not streamed:
        os.environ["FMX_WTRAIN"] = "0"
    try:
        h = capi.Handle(n, k, True, k1, capi.TASK_CLASSIFICATION, 0.0, regw, regv, LR, -1.0, 1.0, **cfg)
    finally:
        for kn in KNOBS:
            os.environ.pop(kn, None)
            if saved[kn] is not None:
                os.environ[kn] = saved[kn]
    h.init_params(0.0, STDEV, SEED)
    return h


def epoch(capi, h, slot=0, batch=FUSED_B, flags=0):
    return h.sgd_epoch(slot, capi.SGD_MINIBATCH, capi.APPLY_FUSED, batch, 0, flags, LAG)


def same_bytes(a, b):
    (w0a, wa, va), (w0b, wb, vb) = a, b
    assert np.float64(w0a).tobytes() == np.float64(w0b).tobytes(), (w0a, w0b)
    assert wa.tobytes() == wb.tobytes(), "w: %d elements differ" % int((wa != wb).sum())
    assert va.tobytes() == vb.tobytes(), "V: %d elements differ" % int((va != vb).sum())


def twin(capi, n, k, data, script, **cfg):
    """`script(h)` -> list of the epochs' status words, on a streamed handle and on the control; ((bits, params, info), (bits, params, info))"""
    out = []
    for streamed in (True, False):
        h = handle(capi, n, k, streamed, **cfg)
        try:
            h.upload_rows(0, *data)
            status = script(h)
            out.append(([bool(int(s) & capi.STAT_WSTREAM) for s in status], h.get_params(), h.wtrain_info(0)))
        finally:
            h.close()
    return out


def three_epochs(capi, batch=FUSED_B, flags=0):
    return lambda h: [epoch(capi, h, 0, batch, flags).status for _ in range(3)]


def check_streamed(capi, n, k, data, batch=FUSED_B):
    (bits, got, (singles, kept)), (cbits, want, (csingles, ckept)) = twin(capi, n, k, data, three_epochs(capi, batch))
    assert singles == numpy_singles(data, k)
    assert 16 * singles >= len(data[0]) and kept
    assert bits == [False, True, True]                  # (the first epoch gathers and fills the stream)
    assert cbits == [False] * 3 and not ckept and csingles == 0
    same_bytes(got, want)
    return singles


# ---- both routes, every row width -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,nnz", [(8, 32), (32, 32), (64, 32), (100, 16)])
def test_in_stream_route(capi, k, nnz):
    """batch 2 048 over 5 333 unit-valued rows (id-only stream on): k_fused<EXACT> + k_apply_seg_scan, two launches per batch"""
    n, data = fixed_rows(ROWS, nnz, seed=500 + k)
    singles = check_streamed(capi, n, k, data)
    assert 0.2 * len(data[0]) <= singles <= 0.4 * len(data[0])


@pytest.mark.parametrize("k,nnz", [(8, 16), (64, 4)])
def test_side_stream_route(capi, k, nnz):
    """batch 32 768 over 70 036 rows: the recurrence on the side stream under the hand-off, a short last batch"""
    n, data = fixed_rows(SIDE_ROWS, nnz, seed=600 + k)
    singles = check_streamed(capi, n, k, data, batch=SIDE)
    assert 0.2 * len(data[0]) <= singles <= 0.4 * len(data[0])


@pytest.mark.parametrize("k,long_rows", [(8, True), (32, True), (64, False), (100, False)])
def test_ragged_rows(capi, k, long_rows):
    """variable lengths with values != 1, empty rows, rows of exactly 64 entries, a repeated id; below k = 64 rows of 65-70 next to them:
    the two-pass branch, no singles there (several entries share a row slot, so the register path still holds rows of 64)"""
    n, data = ragged_rows(ROWS, seed=700, long_rows=long_rows)
    check_streamed(capi, n, k, data)


def test_long_rows_leave_too_few_singles(capi):
    """k = 64 with rows of 65-70 in the slot: no instance holds the longest row, the register path ends at 8 entries, and the singles left
    on it are under 1/16 of the entries -- counted, not kept, no bit, the control's results"""
    n, data = ragged_rows(ROWS, seed=700)
    (bits, got, (singles, kept)), (cbits, want, _) = twin(capi, n, 64, data, three_epochs(capi))
    assert singles == numpy_singles(data, 64) and 0 < 16 * singles < len(data[0]) and not kept
    assert bits == [False] * 3 and cbits == [False] * 3
    same_bytes(got, want)


def test_full_rows_of_64(capi):
    """every row holds exactly 64 entries and every entry is a single: all 64 mask bits, ranks 0 .. 63"""
    rows = FUSED_B + 301
    n, data = permutation_rows(rows, 64, seed=710)
    assert check_streamed(capi, n, 64, data) == rows * 64


# ---- singles only, and none ---------------------------------------------------------------------------------------------------------------
def test_every_entry_a_single(capi):
    n, data = permutation_rows(ROWS, 8, seed=720)
    assert check_streamed(capi, n, 32, data) == ROWS * 8


def test_no_single_no_stream(capi):
    """every id twice: the stream is not built, no epoch carries the bit, the results are the control's"""
    n, data = twice_rows(ROWS + 1, 8, seed=730)
    (bits, got, (singles, kept)), (cbits, want, _) = twin(capi, n, 32, data, three_epochs(capi))
    assert singles == 0 and not kept
    assert bits == [False] * 3 and cbits == [False] * 3
    same_bytes(got, want)


# ---- staleness ----------------------------------------------------------------------------------------------------------------------------
def _touch_a_single(capi, h, data):
    ent = data[0]
    cnt = np.bincount(ent["id"])
    j = int(ent["id"][np.flatnonzero(cnt[ent["id"]] == 1)[3]])
    w0, w, v = h.get_params()
    w[j] = 0.125
    h.set_params(w0, w, v)


def _other_slot(capi, h, data):
    epoch(capi, h, 1)


def _hogwild(capi, h, data):
    h.sgd_epoch(0, capi.SGD_HOGWILD, capi.APPLY_STORE, 512, 0, 0, 0)


def _adagrad(capi, h, data):
    h.adapt_begin()
    h.adapt_epoch(0, FUSED_B)
    h.adapt_end()


@pytest.mark.parametrize("what", ["set_params", "other_slot", "hogwild", "adagrad", "save_load"])
def test_stale_stream_gathers_once(capi, what, tmp_path):
    """two epochs, something that changes linear weights, two more: the epoch after it gathers (no bit) and rewrites the stream, the next one
    reads it again; the parameters follow the control after every step"""
    k = 32
    if what == "hogwild":                                        # (rows that share no feature: the asynchronous step has nothing to race on)
        n, data = permutation_rows(ROWS, 8, seed=740)
    else:
        n, data = fixed_rows(ROWS, 8, seed=741)
    other = fixed_rows(ROWS, 8, seed=742)[1]

    def save_load(capi_, h, data_):
        path = str(tmp_path / "model.txt")
        h.save_model(path)
        h.load_model(path)
    disturb = {"set_params": _touch_a_single, "other_slot": _other_slot, "hogwild": _hogwild, "adagrad": _adagrad, "save_load": save_load}[what]
    trace = []

    def script(h):
        snaps, status = [], []
        if what == "other_slot":
            ids = other[0]["id"] % np.uint32(n)
            h.upload_rows(1, _entries(ids), other[1], other[2])
        for step in range(5):
            if step == 2:
                disturb(capi, h, data)
            else:
                status.append(epoch(capi, h).status)
            snaps.append(h.get_params())
        trace.append(snaps)
        return status
    (bits, got, (_, kept)), (cbits, want, _) = twin(capi, n, k, data, script)
    assert kept
    assert bits == [False, True, False, True]
    assert cbits == [False] * 4
    for a, b in zip(*trace):
        same_bytes(a, b)
    same_bytes(got, want)


# ---- next to the predict-side stream ------------------------------------------------------------------------------------------------------
def test_both_streams_at_once(capi):
    """FMX_FLAG_KEEP_WSIDE epochs with the training-side stream on: the predictions of a handle with neither, bit for bit; whether an
    evaluation reads the predict-side stream still follows the flag alone"""
    k = 64
    n, data = fixed_rows(ROWS, 16, seed=750)
    res = {}
    for name, streamed, flags in (("both", True, capi.FLAG_KEEP_WSIDE), ("train_only", True, 0), ("neither", False, 0)):
        h = handle(capi, n, k, streamed)
        try:
            h.upload_rows(0, *data)
            status = [epoch(capi, h, flags=flags).status for _ in range(3)]
            ev = h.evaluate(0)
            res[name] = (int(status[-1]), int(ev.flags), h.predict(0, ROWS), h.get_params())
        finally:
            h.close()
    assert res["both"][0] & capi.STAT_WSTREAM and res["train_only"][0] & capi.STAT_WSTREAM and not res["neither"][0] & capi.STAT_WSTREAM
    assert res["both"][1] & capi.EVAL_WSIDE
    assert not res["train_only"][1] & capi.EVAL_WSIDE and not res["neither"][1] & capi.EVAL_WSIDE
    for name in ("both", "train_only"):
        assert res[name][2].tobytes() == res["neither"][2].tobytes()
        same_bytes(res[name][3], res["neither"][3])


# ---- the paths that never build it ----------------------------------------------------------------------------------------------------------
def test_off_without_linear_weights(capi):
    n, data = fixed_rows(ROWS, 8, seed=760)
    (bits, got, (_, kept)), (cbits, want, _) = twin(capi, n, 32, data, three_epochs(capi), k1=False)
    assert not kept and bits == [False] * 3 and cbits == [False] * 3
    same_bytes(got, want)


def test_off_under_sgda(capi):
    n, data = fixed_rows(ROWS, 8, seed=761)
    ent, rp, y = data

    def script(h):
        h.upload_rows(1, ent[:int(rp[1000])], rp[:1001], y[:1000])
        h.sgda_begin()
        status = [h.sgda_epoch_minibatch(0, 1, i > 0, FUSED_B, 0).status for i in range(3)]
        h.sgda_end()
        return status
    (bits, got, (_, kept)), (cbits, want, _) = twin(capi, n, 32, data, script, regw=0.0, regv=0.0)
    assert not kept and bits == [False] * 3 and cbits == [False] * 3
    same_bytes(got, want)


def test_off_on_feature_shards(capi):
    """two feature shards on one device (the loopback exchange): the split step, no stream on either shard"""
    n, data = fixed_rows(ROWS, 8, seed=762)
    out = []
    for streamed in (True, False):
        hs = [handle(capi, n, 64, streamed, shard_rank=r, shard_world=2, shard_hash=1) for r in range(2)]
        grp = capi.Group(hs)
        try:
            grp.upload_rows(0, *data)
            status = [grp.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_DEFAULT, 512, 0, 0, 0).status for _ in range(3)]
            out.append(([bool(int(s) & capi.STAT_WSTREAM) for s in status], grp.get_params(), [h.wtrain_info(0)[1] for h in hs]))
        finally:
            grp.close()
            for h in hs:
                h.close()
    (bits, got, kept), (cbits, want, _) = out
    assert kept == [False, False] and bits == [False] * 3 and cbits == [False] * 3
    same_bytes(got, want)
