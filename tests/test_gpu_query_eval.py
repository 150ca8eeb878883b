"""GPU: fmx_set_row_queries / fmx_evaluate_by_query and their group forms -- the exact AUC inside every query (GAUC) reduced on the
device (include/fmx.h).

The oracle is libfm_amd.evalmetrics.query_metrics applied to THE DEVICE'S OWN fmx_predict output of the same slot and parameters:
every integer field and every per-query array is compared with ==, auc_within with == to the Python quotient, gauc and auc_macro
within the forward bound of an fp64 sum (mean_bound below); `pooled` is compared field for field with Handle.evaluate_ex on the
same handle.  n = 50 features, k = 2 (one case at k = 0, one at k = 17), 1 .. 3 entries per row, as tests/test_gpu_eval_ex.py.

n_queries = 2^31 - 1 (16 bytes per query = 32 GiB of scratch inside the call) is RUN, not refused: the library has no cap of its
own below the ABI's.  Where the device cannot give that much at the moment the call has to come back with FMX_E_HIP and leave the
handle usable; the test takes either outcome and says which on stdout."""
import ctypes as C
import math

import numpy as np
import pytest

from libfm_amd.evalmetrics import query_metrics

pytestmark = pytest.mark.gpu

N, K = 50, 2
SCORE_GRID_CAP = 2048        # EVALX_BLOCKS of libfm_amd/csrc/fmx_eval_kernels.h: blocks of 256 threads the grids are capped at
ONE_STRIDE_PLUS_A_WAVE = SCORE_GRID_CAP * 256 + 64      # one wavefront more than a single stride of the capped grid covers
ROW_COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 4097]
LAYOUTS = ["one", "rows", "7", "65", "sparse"]
POOLED_FIELDS = ("rows", "nan_rows", "pos", "neg", "correct", "auc_num2", "auc", "logloss", "rmse", "mae", "accuracy", "flags", "reserved")
INT_FIELDS = ("queries", "valid_queries", "one_class_queries", "empty_queries", "valid_rows", "num2_within", "den2_within")
MEANS = ("auc_within", "gauc", "auc_macro")
LINKS = {"logistic": 0, "probit": 1}


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


def make_rows(capi, rows, seed, dyadic, positive_values=False):
    """1 .. 3 entries per row with distinct ids; dyadic: values from a few multiples of 1/8 (every sum of the prediction is then
    exact in fp32 whatever its order), else seeded real values"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 4, rows)
    rp = np.zeros(rows + 1, dtype=np.uint64)
    rp[1:] = np.cumsum(sizes)
    ent = np.zeros(int(rp[-1]), dtype=capi.ENTRY_DTYPE)
    base = rng.integers(0, N, rows)
    step = rng.integers(1, N // 3, rows)                 # ids base, base + step, base + 2 step (mod N): distinct inside a row
    row_of = np.repeat(np.arange(rows), sizes)
    pos_in_row = np.arange(len(ent)) - np.repeat(rp[:-1].astype(np.int64), sizes)
    ent["id"] = ((base[row_of] + pos_in_row * step[row_of]) % N).astype(np.uint32)
    if dyadic:
        ent["value"] = rng.choice(np.array([1.0, 0.5, 2.0] if positive_values else [1.0, 0.5, -1.0, 2.0]), len(ent)).astype(np.float32)
    else:
        v = rng.normal(0.0, 1.0, len(ent))
        ent["value"] = (np.abs(v) if positive_values else v).astype(np.float32)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    return ent, rp, y


def make_params(seed, dyadic, k=K):
    rng = np.random.default_rng(1000 + seed)
    if dyadic:
        lv = np.array([-0.5, -0.125, 0.0, 0.125, 0.5, 1.0])
        return 0.125, rng.choice(lv, N), rng.choice(lv, (k, N))
    return 0.07, rng.normal(0, 0.6, N), rng.normal(0, 0.6, (k, N))


def make_queries(layout, rows, seed):
    """(qid uint32 [rows], n_queries).  one: a single query, whose segment spans every wavefront and block (all atomics hit one
    word); rows: every segment has length 1 and every query one class; 7 / 65: seeded draws; sparse: n_queries = rows + 70 with
    empty queries at both ends (no id below 35 or above rows + 34) and, the draws being with replacement, in between"""
    rng = np.random.default_rng(5000 + seed)
    if layout == "one":
        return np.zeros(rows, dtype=np.uint32), 1
    if layout == "rows":
        return rng.permutation(rows).astype(np.uint32), rows
    if layout == "sparse":
        return (35 + rng.integers(0, rows, rows)).astype(np.uint32), rows + 70
    return rng.integers(0, int(layout), rows).astype(np.uint32), int(layout)


def handle(capi, task=1, k=K, **kw):
    return capi.Handle(N, k, True, True, task, 0.0, 0.001, 0.002, 0.01, -1.0, 1.0, **kw)


def mean_bound(want, valid_queries):
    """|device - oracle| allowed for gauc and auc_macro: the device adds `valid_queries` non-negative fp64 terms in a fixed order;
    the forward error of such a sum is at most (V - 1) u |sum| with u = 2^-53, whatever the order; one rounding per product
    rows_q * auc_q and one for the final division come on top; the oracle's own sum (math.fsum) is correctly rounded."""
    return abs(want) * (valid_queries + 4) * 2.0 ** -53 * 2


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) if isinstance(a, float) and (math.isnan(a) or math.isnan(b)) else a == b


def check_struct(ev, want, pooled):
    """the struct against the oracle's dict and against fmx_evaluate_ex's struct of the same handle, slot and link"""
    got = {f: int(getattr(ev, f)) for f in INT_FIELDS}
    print(got, ev.auc_within, ev.gauc, ev.auc_macro, "oracle", want["num2_within"], want["auc_within"], want["gauc"], want["auc_macro"])
    assert got == {f: want[f] for f in INT_FIELDS}
    for f in POOLED_FIELDS:
        assert same(getattr(ev.pooled, f), getattr(pooled, f)), f
    if want["valid_queries"] == 0:
        assert all(math.isnan(getattr(ev, f)) for f in MEANS)
        return
    assert ev.auc_within == want["num2_within"] / want["den2_within"]
    for f in ("gauc", "auc_macro"):
        assert abs(getattr(ev, f) - want[f]) <= mean_bound(want[f], want["valid_queries"]), f
    assert ev.device_seconds >= ev.rank_seconds > 0.0


def check_against_oracle(h, slot, rows, y, qid, nq, links=("logistic",), per_query=True):
    p = h.predict(slot, rows)
    out = None
    for link in links:
        want = query_metrics(p, y, qid, nq, link, per_query=per_query)
        if per_query:
            ev, num2, pos, neg = h.evaluate_by_query(slot, LINKS[link], per_query=True)
            assert num2.dtype == np.uint64 and pos.dtype == np.uint32 and neg.dtype == np.uint32 and len(num2) == len(pos) == len(neg) == nq
            assert np.array_equal(pos, np.asarray(want["pos_q"], dtype=np.uint32))
            assert np.array_equal(neg, np.asarray(want["neg_q"], dtype=np.uint32))
            assert np.array_equal(num2, np.asarray(want["num2_q"], dtype=np.uint64))
        else:
            ev = h.evaluate_by_query(slot, LINKS[link])
        check_struct(ev, want, h.evaluate_ex(slot, LINKS[link]))
        out = out or (ev, want)
    return out


@pytest.fixture(scope="module")
def hc(capi):
    h = handle(capi)
    yield h
    h.close()


@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "real"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_every_field_and_array_equals_the_oracle(capi, hc, rows, layout, dyadic):
    ent, rp, y = make_rows(capi, rows, rows + 7 * dyadic, dyadic)
    qid, nq = make_queries(layout, rows, rows)
    hc.set_params(*make_params(rows, dyadic))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    ev, want = check_against_oracle(hc, 0, rows, y, qid, nq)
    if layout == "rows":
        assert (ev.valid_queries, ev.one_class_queries, ev.empty_queries) == (0, rows, 0)
    if layout == "one":
        assert ev.num2_within == ev.pooled.auc_num2 and (ev.valid_queries == 1) == bool(ev.pooled.pos and ev.pooled.neg)
    if layout == "sparse":
        assert ev.empty_queries >= 70
    if dyadic and rows >= 255:                             # ties dominate: far fewer distinct scores than rows
        assert len(np.unique(hc.predict(0, rows))) < rows // 2


def test_both_links(capi, hc):
    rows = 257
    ent, rp, y = make_rows(capi, rows, 3, False)
    qid, nq = make_queries("7", rows, 3)
    hc.set_params(*make_params(5, False))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid)                              # n_queries None = max + 1
    assert int(qid.max()) + 1 == nq
    check_against_oracle(hc, 0, rows, y, qid, nq, links=("logistic", "probit"))


def test_segment_boundaries_on_purpose(capi, hc):
    """one entry per row and a model of linear weights only, so that a row's score is w0 + w[its feature]: the sorted layout is
    known.  Query sizes 63, 1, 1, 63, 64, 63, 1, 1, 63, 100 put the query boundaries after the sorted positions 62, 63, 64, 127
    (a wavefront's last lane), 191 (another), 254, 255, 256 and 319.  Query 3 ends in a tie run at the score of feature 25 and
    query 4 begins with one at the same score, both labels on both sides: a run head that leaked across the boundary at 127 / 128
    would count query 3's negatives for query 4's positives."""
    sizes = [63, 1, 1, 63, 64, 63, 1, 1, 63, 100]
    assert np.cumsum(sizes).tolist() == [63, 64, 65, 128, 192, 255, 256, 257, 320, 420]
    rng = np.random.default_rng(17)
    qid = np.repeat(np.arange(len(sizes)), sizes).astype(np.uint32)
    feat = rng.integers(0, N, len(qid))
    y = np.where(rng.random(len(qid)) < 0.5, 1.0, -1.0).astype(np.float32)
    in3, in4 = np.flatnonzero(qid == 3), np.flatnonzero(qid == 4)
    feat[in3] = rng.integers(0, 25, len(in3))               # query 3: scores up to that of feature 25 ...
    feat[in4] = rng.integers(26, N, len(in4))               # ... query 4: from it upwards
    feat[in3[:6]] = feat[in4[:6]] = 25
    y[in3[:6]] = y[in4[:6]] = [1, -1, 1, -1, -1, 1]
    order = rng.permutation(len(qid))                       # the upload order says nothing about the sorted one
    qid, feat, y = qid[order], feat[order], y[order]
    ent = np.zeros(len(qid), dtype=capi.ENTRY_DTYPE)
    ent["id"], ent["value"] = feat, 1.0
    hc.set_params(0.125, (np.arange(N) - 25) / 8.0, np.zeros((K, N)))
    hc.upload_rows(0, ent, np.arange(len(qid) + 1, dtype=np.uint64), y)
    hc.set_row_queries(0, qid, len(sizes))
    p = hc.predict(0, len(qid))
    assert np.array_equal(p, 0.125 + (feat - 25) / 8.0)
    assert p[qid == 3].max() == p[qid == 4].min() == 0.125
    ev, want = check_against_oracle(hc, 0, len(qid), y, qid, len(sizes))
    assert ev.valid_queries >= 6 and want["num2_q"][3] > 0 and want["num2_q"][4] > 0


def test_high_id_bits(capi, hc):
    """n_queries = 2^24 + 3: 25 id bits above the 33 of the score and label, the sort runs over bits 0 .. 57; the per-query arrays
    (268 MB on the device, freed inside the call) come back for this one case"""
    rows, nq = 300, 2 ** 24 + 3
    ent, rp, y = make_rows(capi, rows, 23, True)
    ids = np.array([0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 2], dtype=np.uint32)
    qid = ids[np.random.default_rng(23).integers(0, len(ids), rows)]
    hc.set_params(*make_params(23, True))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    ev, want = check_against_oracle(hc, 0, rows, y, qid, nq)
    assert ev.empty_queries == nq - 5 and ev.valid_queries == 5


def test_largest_n_queries(capi, hc):
    """n_queries = 2^31 - 1 (31 id bits: all 64 key bits are sorted), 10 rows, no per-query arrays: see the module docstring"""
    rows, nq = 10, 2 ** 31 - 1
    ent, rp, y = make_rows(capi, rows, 29, True)
    y[:] = [1, -1, 1, -1, 1, -1, 1, -1, 1, -1]
    qid = np.array([0, 0, 2 ** 30, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 2, 2 ** 31 - 2, 5, 5, 7], dtype=np.uint32)
    hc.set_params(*make_params(29, True))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    try:
        ev, want = check_against_oracle(hc, 0, rows, y, qid, nq, per_query=False)
    except capi.FmxError as e:
        print("refused:", e)
        assert e.code == -2 and "memory" in e.text.lower()                                     # FMX_E_HIP, out of memory
    else:
        print("ran: rank_seconds", ev.rank_seconds)
        assert (ev.queries, ev.valid_queries, ev.one_class_queries, ev.empty_queries) == (nq, 4, 1, nq - 5)
    hc.set_row_queries(0, qid % 7, 7)                       # the handle works on, with the scratch given back
    check_against_oracle(hc, 0, rows, y, qid % 7, 7)


@pytest.mark.parametrize("nq", [4099, 3])
def test_one_long_case(capi, hc, nq):
    """more rows than one stride of the capped grid: every wavefront of the rank sum walks a chunk of two steps and carries the
    segment open at lane 63 into the second -- mostly on into lane 0 (3 queries), often not (4099 queries of about 128 rows)"""
    rows = ONE_STRIDE_PLUS_A_WAVE
    ent, rp, y = make_rows(capi, rows, 41, True)
    qid = np.random.default_rng(41).integers(0, nq, rows).astype(np.uint32)
    hc.set_params(*make_params(4, True))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    ev, want = check_against_oracle(hc, 0, rows, y, qid, nq)
    assert ev.valid_queries == nq


@pytest.mark.parametrize("k", [0, 17])
def test_other_factor_widths(capi, k):
    h = handle(capi, k=k)
    ent, rp, y = make_rows(capi, 257, 3, False)
    qid, nq = make_queries("7", 257, 9)
    w0, w, v = make_params(5, False, k)
    h.set_params(w0, w, v if k else None)
    h.upload_rows(0, ent, rp, y)
    h.set_row_queries(0, qid, nq)
    check_against_oracle(h, 0, 257, y, qid, nq, links=("logistic", "probit"))
    h.close()


def test_zero_model_and_empty_slot(capi, hc):
    rows = 300
    ent, rp, y = make_rows(capi, rows, 11, True)
    qid, nq = make_queries("7", rows, 11)
    hc.set_params(0.0, np.zeros(N), np.zeros((K, N)))      # a zero model: every score equal
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    ev, num2, pos, neg = hc.evaluate_by_query(0, per_query=True)
    assert ev.valid_queries == 7 and np.array_equal(num2, pos.astype(np.uint64) * neg)          # every auc_q == 0.5 exactly
    assert ev.auc_within == 0.5 and ev.gauc == 0.5 and ev.auc_macro == 0.5
    check_against_oracle(hc, 0, rows, y, qid, nq)
    hc.set_params(*make_params(1, False))
    for sign in (1.0, -1.0):                               # the whole slot of one class: pooled sorts nothing, the queries are still counted
        ys = np.full(rows, sign, dtype=np.float32)
        hc.upload_rows(0, ent, rp, ys)
        hc.set_row_queries(0, qid, nq + 2)
        ev, want = check_against_oracle(hc, 0, rows, ys, qid, nq + 2)
        assert (ev.valid_queries, ev.one_class_queries, ev.empty_queries, ev.valid_rows) == (0, 7, 2, 0)
        assert (ev.num2_within, ev.den2_within) == (0, 0) and math.isnan(ev.pooled.auc) and not math.isnan(ev.pooled.logloss)
    hc.upload_rows(0, ent[:0], np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.float32))     # an empty slot
    hc.set_row_queries(0, np.zeros(0, dtype=np.uint32), 4)
    ev, num2, pos, neg = hc.evaluate_by_query(0, per_query=True)
    assert (ev.queries, ev.empty_queries, ev.valid_queries, ev.one_class_queries, ev.valid_rows) == (4, 4, 0, 0, 0)
    assert all(math.isnan(getattr(ev, f)) for f in MEANS) and ev.pooled.rows == 0 and math.isnan(ev.pooled.auc)
    assert not num2.any() and not pos.any() and not neg.any() and len(num2) == 4


def test_nan_and_infinite_weights(capi, hc):
    rows, j = 4097, 17
    ent, rp, y = make_rows(capi, rows, 21, False, positive_values=True)
    qid, nq = make_queries("65", rows, 21)
    w0, w, v = make_params(2, False)
    w[j] = np.nan
    hc.set_params(w0, w, v)
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    ev, want = check_against_oracle(hc, 0, rows, y, qid, nq)
    assert ev.pooled.nan_rows > 0 and all(math.isnan(getattr(ev, f)) for f in MEANS) and ev.rank_seconds == 0.0
    assert {f: int(getattr(ev, f)) for f in INT_FIELDS} == {**dict.fromkeys(INT_FIELDS, 0), "queries": nq}
    _, num2, pos, neg = hc.evaluate_by_query(0, per_query=True)
    assert not num2.any() and not pos.any() and not neg.any()
    w[j] = np.inf                                          # (positive values: w_j x is +inf in every row that holds j)
    hc.set_params(w0, w, v)
    assert np.isposinf(hc.predict(0, rows)).any()
    ev, want = check_against_oracle(hc, 0, rows, y, qid, nq)
    assert ev.pooled.nan_rows == 0 and ev.valid_queries == 65 and ev.pooled.logloss == math.inf


def test_regression_handle(capi):
    rows = 257
    ent, rp, y = make_rows(capi, rows, 31, False)
    y = np.random.default_rng(5).normal(0.0, 0.8, rows).astype(np.float32)
    h = handle(capi, task=0)
    h.set_params(*make_params(3, False))
    h.upload_rows(0, ent, rp, y)
    h.set_row_queries(0, *make_queries("7", rows, 1))
    ev, num2, pos, neg = h.evaluate_by_query(0, per_query=True)
    ex = h.evaluate_ex(0)
    for f in POOLED_FIELDS:
        assert same(getattr(ev.pooled, f), getattr(ex, f)), f
    assert ev.pooled.rmse > 0 and ev.queries == 7 and ev.rank_seconds == 0.0
    assert (ev.valid_queries, ev.one_class_queries, ev.empty_queries, ev.valid_rows, ev.num2_within, ev.den2_within) == (0,) * 6
    assert all(math.isnan(getattr(ev, f)) for f in MEANS) and not num2.any() and not pos.any() and not neg.any()
    h.close()


def _bytes_outside_the_times(capi, ev):
    b = bytearray(bytes(ev))
    for off in (capi.EvalQuery.device_seconds.offset, capi.EvalQuery.rank_seconds.offset,
                capi.EvalQuery.pooled.offset + capi.EvalEx.device_seconds.offset, capi.EvalQuery.pooled.offset + capi.EvalEx.rank_seconds.offset):
        b[off:off + 8] = bytes(8)
    return bytes(b)


def test_two_calls_are_bit_identical(capi, hc):
    rows = 4097 * 8
    ent, rp, y = make_rows(capi, rows, 43, False)
    qid, nq = make_queries("sparse", rows, 43)
    hc.set_params(*make_params(4, False))
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    a, b = hc.evaluate_by_query(0, 1, per_query=True), hc.evaluate_by_query(0, 1, per_query=True)
    assert _bytes_outside_the_times(capi, a[0]) == _bytes_outside_the_times(capi, b[0]) and a[0].valid_queries > 1000
    for x, z in zip(a[1:], b[1:]):
        assert np.array_equal(x, z)


def test_state(capi):
    h = handle(capi)
    lib = capi.load()
    rows = 65
    ent, rp, y = make_rows(capi, rows, 3, True)
    qid, nq = make_queries("7", rows, 3)
    h.set_params(*make_params(3, True))

    def refused(fn, code, *needles):
        with pytest.raises(capi.FmxError) as ei:
            fn()
        assert ei.value.code == code
        for n in needles:
            assert n in ei.value.text, ei.value.text

    refused(lambda: h.set_row_queries(0, qid, nq), -3, "fmx_set_row_queries")                   # a slot never uploaded
    refused(lambda: h.evaluate_by_query(0), -3, "fmx_evaluate_by_query")
    h.upload_rows(0, ent, rp, y)
    refused(lambda: h.evaluate_by_query(0), -3, "no query ids")                                 # before set_row_queries
    refused(lambda: h.set_row_queries(0, qid, 0), -1, "n_queries")
    refused(lambda: h.set_row_queries(0, qid, 2 ** 31), -1, "n_queries")
    h.set_row_queries(0, qid, nq)
    first = h.evaluate_by_query(0, per_query=True)
    bad = qid.copy()
    bad[40], bad[50] = 7, 9
    refused(lambda: h.set_row_queries(0, bad, nq), -1, "row 40")                                # names the first offending row ...
    again = h.evaluate_by_query(0, per_query=True)                                              # ... and leaves the previous ids in force
    assert _bytes_outside_the_times(capi, first[0]) == _bytes_outside_the_times(capi, again[0])
    assert all(np.array_equal(x, z) for x, z in zip(first[1:], again[1:]))
    other = (qid + 3) % 11                                                                      # replacement by a second call
    h.set_row_queries(0, other, 11)
    check_against_oracle(h, 0, rows, y, other, 11)
    h.set_row_queries(0, None)                                                                  # NULL drops them
    refused(lambda: h.evaluate_by_query(0), -3, "no query ids")
    h.set_row_queries(0, qid, nq)
    h.upload_rows(0, ent, rp, y)                                                                # so does a new upload ...
    refused(lambda: h.evaluate_by_query(0), -3, "no query ids")
    h.set_row_queries(0, qid, nq)
    h.free_rows(0)                                                                              # ... and fmx_free_rows
    refused(lambda: h.evaluate_by_query(0), -3, "holds no rows")
    h.upload_rows(0, ent, rp, y)
    refused(lambda: h.evaluate_by_query(0), -3, "no query ids")
    h.upload_rows(2, ent, rp, None)                                                             # the refusals of fmx_evaluate_ex
    h.set_row_queries(2, qid, nq)
    refused(lambda: h.evaluate_by_query(2), -3, "without targets")
    h.set_row_queries(0, qid, nq)
    out = capi.EvalQuery()
    assert lib.fmx_evaluate_by_query(h.h, 0, None, None, None, None, None) == -1                # NULL out
    assert lib.fmx_evaluate_by_query(h.h, 0, C.byref(capi.EvalOpts(2, 0)), C.byref(out), None, None, None) == -1   # unknown link
    assert lib.fmx_evaluate_by_query(h.h, 0, C.byref(capi.EvalOpts(0, 1)), C.byref(out), None, None, None) == -1   # flags != 0
    assert b"fmx_evaluate_by_query" in lib.fmx_last_error(h.h)
    assert lib.fmx_evaluate_by_query(h.h, 0, None, C.byref(out), None, None, None) == 0 and out.queries == nq     # NULL opts = logistic
    assert out.pooled.logloss == h.evaluate_ex(0, capi.LINK_LOGISTIC).logloss
    h.close()


def test_weight_side_stream(capi):
    rows = 4097
    ent, rp, y = make_rows(capi, rows, 51, False)
    qid, nq = make_queries("65", rows, 51)
    h = handle(capi)
    h.set_params(*make_params(6, False))
    h.upload_rows(0, ent, rp, y)
    h.set_row_queries(0, qid, nq)
    h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_FUSED, 256, 32, capi.FLAG_KEEP_WSIDE, 2)
    ev, _ = check_against_oracle(h, 0, rows, y, qid, nq)
    assert ev.pooled.flags & capi.EVAL_WSIDE and ev.valid_queries == 65
    h.close()


def _relational(capi, rows, seed):
    """dyadic block-structured rows over the N attributes: main rows of one entry (ids 0 .. 9), one block of 7 rows with 1 .. 2
    entries over the block's 40 attributes (global ids 10 .. 49)"""
    rng = np.random.default_rng(seed)
    vals = np.array([1.0, 0.5, -1.0, 2.0])
    ent = np.zeros(rows, dtype=capi.ENTRY_DTYPE)
    ent["id"], ent["value"] = rng.integers(0, 10, rows), rng.choice(vals, rows)
    rp = np.arange(rows + 1, dtype=np.uint64)
    bsizes = rng.integers(1, 3, 7)
    brp = np.zeros(8, dtype=np.uint64)
    brp[1:] = np.cumsum(bsizes)
    bent = np.zeros(int(brp[-1]), dtype=capi.ENTRY_DTYPE)
    bent["id"] = np.concatenate([rng.choice(40, s, replace=False) for s in bsizes])
    bent["value"] = rng.choice(vals, len(bent))
    mp = rng.integers(0, 7, rows).astype(np.uint32)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    return ent, rp, y, [(bent, brp, mp, 10)]


def test_kept_relation_blocks(capi, hc):
    rows = 4097
    ent, rp, y, rel = _relational(capi, rows, 61)
    qid, nq = make_queries("65", rows, 61)
    hc.set_params(*make_params(7, True))
    hc.upload_block_rows(0, ent, rp, y, rel, keep=True)
    hc.upload_block_rows(1, ent, rp, y, rel, keep=False)
    hc.set_row_queries(0, qid, nq)
    hc.set_row_queries(1, qid, nq)
    a, b = hc.evaluate_by_query(0, per_query=True), hc.evaluate_by_query(1, per_query=True)
    assert {f: getattr(a[0], f) for f in INT_FIELDS} == {f: getattr(b[0], f) for f in INT_FIELDS} and a[0].num2_within > 0
    assert all(np.array_equal(x, z) for x, z in zip(a[1:], b[1:]))
    check_against_oracle(hc, 0, rows, y, qid, nq)
    hc.free_rows(1)


@pytest.mark.parametrize("world", [2, 3])
def test_loopback_groups(capi, hc, world):
    rows = 4097
    ent, rp, y = make_rows(capi, rows, 71, True)             # dyadic: the shards' y-hat does not differ in rounding
    qid, nq = make_queries("sparse", rows, 71)
    params = make_params(8, True)
    hc.set_params(*params)
    hc.upload_rows(0, ent, rp, y)
    hc.set_row_queries(0, qid, nq)
    hs = [handle(capi, device=0, shard_rank=r, shard_world=world, shard_hash=1) for r in range(world)]
    g = capi.Group(hs)
    g.set_params(*params)
    g.upload_rows(0, ent, rp, y)
    with pytest.raises(capi.FmxError) as ei:
        g.evaluate_by_query(0)
    assert ei.value.code == -3 and "no query ids" in ei.value.text
    g.set_row_queries(0, qid, nq)
    for link in LINKS.values():
        one, grp = hc.evaluate_by_query(0, link, per_query=True), g.evaluate_by_query(0, link, per_query=True)
        assert {f: getattr(grp[0], f) for f in INT_FIELDS} == {f: getattr(one[0], f) for f in INT_FIELDS} and one[0].valid_queries > 100
        assert all(np.array_equal(x, z) for x, z in zip(one[1:], grp[1:]))
        assert grp[0].auc_within == one[0].auc_within
        for f in ("gauc", "auc_macro"):
            assert abs(getattr(grp[0], f) - getattr(one[0], f)) <= mean_bound(getattr(one[0], f), one[0].valid_queries)
        gex = g.evaluate_ex(0, link)
        for f in POOLED_FIELDS:
            assert same(getattr(grp[0].pooled, f), getattr(gex, f)), f
    with pytest.raises(capi.FmxError) as ei:                 # a shard handle passed to fmx_evaluate_by_query itself
        hs[0].evaluate_by_query(0)
    assert ei.value.code == -4 and "fmx_evaluate_by_query" in ei.value.text
    g.upload_rows(0, ent, rp, y)                             # a new upload drops the ids on the first shard too
    with pytest.raises(capi.FmxError) as ei:
        g.evaluate_by_query(0)
    assert ei.value.code == -3
    g.close()
    for h in hs:
        h.close()


def test_one_handle_group_forwards(capi):
    rows = 257
    ent, rp, y = make_rows(capi, rows, 91, False)
    qid, nq = make_queries("7", rows, 91)
    h = handle(capi)
    g = capi.Group([h])
    h.set_params(*make_params(10, False))
    h.upload_rows(0, ent, rp, y)
    g.set_row_queries(0, qid, nq)
    assert _bytes_outside_the_times(capi, g.evaluate_by_query(0, 1)) == _bytes_outside_the_times(capi, h.evaluate_by_query(0, 1))
    assert g.evaluate_by_query(0).valid_queries == 7
    g.close()
    h.close()


def _separable(capi, rows, seed):
    """a toy set a linear model separates: feature 0 .. 24 in positive rows, 25 .. 49 in negative rows, plus one shared feature"""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    ent = np.zeros(2 * rows, dtype=capi.ENTRY_DTYPE)
    ent["id"][0::2] = np.where(y > 0, rng.integers(0, 24, rows), rng.integers(25, 49, rows))
    ent["id"][1::2] = 49
    ent["value"] = 1.0
    return ent, np.arange(0, 2 * rows + 1, 2, dtype=np.uint64), y


def _learner(L, cls):
    l = cls()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor = N, K
    l.fm.init(np.random.default_rng(3))
    l.task, l.num_iter, l.min_target, l.max_target = L.TASK_CLASSIFICATION, 5, -1.0, 1.0
    return l


def test_sgd_learner(capi, capsys):
    from libfm_amd import learner as L
    tr, te = L.Data(*_separable(capi, 200, 1)), L.Data(*_separable(capi, 200, 2))
    qid = np.random.default_rng(4).integers(0, 9, 200)
    l = _learner(L, L.FMLearnSGD)
    l.learn_rate = 0.05
    l.init()
    l.set_queries(te, qid)                                   # the test set only: Train prints nan
    l.learn(tr, te)
    want = query_metrics(l.predict_raw(te), te.target, qid, 9)
    ev = l.evaluate_by_query(te)
    assert ev.num2_within == want["num2_within"] and ev.valid_queries == want["valid_queries"] == 9
    assert l.log[-1]["auc_within_test"] == want["auc_within"] and want["gauc"] > 0.7
    assert abs(l.log[-1]["gauc_test"] - want["gauc"]) <= mean_bound(want["gauc"], 9)
    assert math.isnan(l.log[-1]["gauc_train"]) and math.isnan(l.log[-1]["auc_within_train"])
    cap = capsys.readouterr()
    assert cap.err.count("\tgauc: Train=nan\tTest=") == 5 and "gauc" not in cap.out
    with pytest.raises(ValueError):
        l.evaluate_by_query(tr)
    with pytest.raises(ValueError):
        l.set_queries(tr, qid[:10])
    l.close()
    m = L.FMLearnMCMC()
    with pytest.raises(NotImplementedError):
        m.set_queries(te, qid)


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-handle", "two-shards"])
def test_als_learner(capi, capsys, devices):
    from libfm_amd import learner as L
    tr, te = L.Data(*_separable(capi, 200, 1)), L.Data(*_separable(capi, 200, 2))
    qtr, qte = np.random.default_rng(5).integers(0, 9, 200), np.random.default_rng(6).integers(0, 5, 200)
    l = _learner(L, L.FMLearnALS)
    l.num_iter, l.w_lambda, l.v_lambda, l.devices = 2, 1.0, 1.0, devices
    l.init()
    l.set_queries(tr, qtr)
    l.set_queries(te, qte, 6)
    l.learn(tr, te)
    want = query_metrics(l._h.predict(1, te.num_cases), te.target, qte, 6, "probit")
    ev = l.evaluate_by_query(te)
    assert (ev.num2_within, ev.queries, ev.empty_queries) == (want["num2_within"], 6, 1)
    assert l.log[-1]["auc_within_test"] == want["auc_within"] and not math.isnan(l.log[-1]["gauc_train"])
    assert capsys.readouterr().err.count("\tgauc: Train=") == 2
    l.close()


def _write_libfm(path, ent, rp, y):
    with open(path, "w") as f:
        for r in range(len(y)):
            f.write("%g %s\n" % (y[r], " ".join("%d:%g" % (e["id"], e["value"]) for e in ent[int(rp[r]):int(rp[r + 1])])))


def test_cli_query_flags(capi, tmp_path, capsys):
    from libfm_amd import cli
    trf, tef = str(tmp_path / "tr.libfm"), str(tmp_path / "te.libfm")
    _write_libfm(trf, *_separable(capi, 200, 1))
    _write_libfm(tef, *_separable(capi, 200, 2))
    qtr, qte = str(tmp_path / "qtr.txt"), str(tmp_path / "qte.txt")
    np.savetxt(qtr, np.random.default_rng(7).integers(0, 9, 200), fmt="%d")
    np.savetxt(qte, np.random.default_rng(8).integers(0, 9, 200), fmt="%d")
    rlog = str(tmp_path / "rlog.tsv")
    argv = ["-task", "c", "-train", trf, "-test", tef, "-dim", "1,1,2", "-iter", "3", "-method", "sgd", "-learn_rate", "0.05",
            "-init_stdev", "0.1", "-seed", "42"]
    assert cli.main(argv) == 0
    plain = capsys.readouterr()
    assert cli.main(argv + ["-test_queries", qte]) == 0
    test_only = capsys.readouterr()
    assert cli.main(argv + ["-test_queries", qte, "-train_queries", qtr, "-rlog", rlog]) == 0
    both = capsys.readouterr()
    assert test_only.out == plain.out == both.out and plain.out.count("#Iter=") == 3
    assert "gauc" not in plain.err
    assert test_only.err.count("\tgauc: Train=nan\tTest=") == 3
    assert both.err.count("\tgauc: Train=") == 3 and "nan" not in both.err
    header = open(rlog).readline().split("\t")
    assert {"gauc_train", "gauc_test", "auc_within_train", "auc_within_test"} <= {c.strip() for c in header}
