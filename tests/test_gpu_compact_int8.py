"""GPU: the int8 row-wise serving snapshot (FMX_COMPACT_INT8: k_compact_quant8, k_rowsums and k_fetch_rows over RowsI8; include/fmx.h,
DESIGN.md section 21) against libfm_amd/compact.py (pinned on the CPU in tests/test_compact_int8_cpu.py).  Rows, models and tolerances
are those of tests/test_gpu_compact.py.

Shapes.  k in {0, 1, 2, 8, 9, 24, 25, 56, 57, 64, 100, 120, 121, 128, 256}: both sides of every block size P(k) = 8, 16, 32, 64, 128,
192, 320 and every lane map of RowsI8 with 8-byte loads (2, 4, 8, 16, 32, 64 lanes per row), among them the widths whose block is
smaller than the lane map covers (k = 24 under KP = 32, k = 56 under KP = 64: whole lanes at or beyond P hold zeros).  n in {1, 200,
4099}, k1 on and off, both tasks.  One case in the regime the format is for: n = 3e6 with ids up to n - 1 and 40 000 rows, more than
resident wavefronts, so the loops of k_rowsums and k_compact_quant8 run; bf16 and int8 snapshots replace one another three times.

Tolerances.  Snapshot rows, max_abs_err, nonfinite, bytes: exact.  sum_sq_err rtol 1e-12.  Scores against the restatement: the
project's predict tolerance (RTOL, ATOL of test_gpu_compact).  int8 against fp32: a factor moves by at most
delta_i = step_i (0.5 + EPS) (test_compact_int8_cpu: EPS and the absolute term of subnormal scales, which these models never reach),
so a pair's product v_if x_i v_jf x_j moves by at most (delta_i |v_jf| + |v_if| delta_j + delta_i delta_j) |x_i x_j|; summed over
i < j and f in fp64 that is the bound, on top of the predict tolerance.

Measured on an MI355X (largest over the cases; every test prints its own figures): snapshot rows, max_abs_err, nonfinite and bytes
equal; sum_sq_err 3.1e-16 relative; compact_predict against the restatement 1.3e-6 absolute; |compact - fmx_predict|
0.0151 absolute, at most 0.151 of its bound; counts and AUC numerators equal, log loss to the last digit or one ulp."""
import ctypes as C
import io
import math

import numpy as np
import pytest

import topk_oracle as T
from libfm_amd import compact
from libfm_amd.evalmetrics import classification_metrics
from test_compact_cpu import planted
from test_compact_int8_cpu import EPS, ROW_BYTES
from test_gpu_compact import (ATOL, ROWS, RTOL, bits, compact_dtype, handle, make_params, make_rows, row_stride, same_bits,
                              tiny_regression, trained_learner, write_libfm)
from test_gpu_eval_ex import INT_FIELDS, logloss_bound
from test_gpu_topk import check_lists

pytestmark = pytest.mark.gpu

# (k, n, k1, task): every k, every n, k1 on and off, both tasks
CASES = [(0, 200, True, 0), (1, 4099, True, 1), (2, 200, False, 0), (8, 4099, True, 1), (9, 200, True, 0), (24, 200, False, 1),
         (25, 4099, True, 0), (56, 200, True, 1), (57, 200, False, 0), (64, 4099, True, 1), (64, 200, False, 0), (100, 4099, True, 0),
         (120, 200, True, 1), (121, 200, False, 0), (128, 200, True, 1), (256, 200, False, 1), (8, 1, True, 0), (64, 1, True, 1),
         (0, 1, False, 1)]
IDS = ["k%d-n%d-%s-%s" % (k, n, "k1" if k1 else "nok1", "cr"[1 - t]) for k, n, k1, t in CASES]
INT8 = 3


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    assert capi.COMPACT_INT8 == INT8
    return capi


def int8_bound(ent, rp, v):
    """sum_{i<j} sum_f (delta_i |v_jf| + |v_if| delta_j + delta_i delta_j) |x_i x_j| per row, fp64 (v: [k][n]), delta_i = step_i (0.5 + EPS):
    with A_i = |v_if x_i| and D_i = delta_i |x_i| that is (sum D)(sum A) - sum D_i A_i + ((sum D)^2 - sum D_i^2) / 2 per factor"""
    rp = np.asarray(rp, dtype=np.int64)
    n = len(rp) - 1
    out = np.zeros(n)
    if v.shape[0] == 0:
        return out
    row = np.repeat(np.arange(n), np.diff(rp))
    ids, xs = ent["id"].astype(np.int64), np.abs(ent["value"].astype(np.float64))
    delta = np.abs(v).max(axis=0) / 127.0 * (0.5 + EPS)
    d = delta[ids] * xs
    sd, sdd = np.bincount(row, weights=d, minlength=n), np.bincount(row, weights=d * d, minlength=n)
    for f in range(v.shape[0]):
        a = np.abs(v[f, ids]) * xs
        out += sd * np.bincount(row, weights=a, minlength=n) - np.bincount(row, weights=d * a, minlength=n)
    return out + v.shape[0] * 0.5 * (sd * sd - sdd)


def model_of(w0, w, v, k1=True):
    return compact.CompactModel(w0, w, v, True, k1, format="int8")


# ---- 1. the quantiser -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, n, k1, task", CASES, ids=IDS)
def test_quantiser_bit_exact_and_report(capi, k, n, k1, task):
    w0, w, v = make_params(n, k, k)
    px, _ = planted()
    special = np.concatenate([px, np.array([np.nan], dtype=np.float32)]).astype(np.float64)
    if k >= 1 and n >= 2 * len(special) + 8:               # the planted values of the CPU test, through fmx_set_params
        v[0, :len(special)] = special
        v[k - 1, n - len(special):] = special[::-1]
        v[:, len(special)] = 0.0                           # an all-zero row
        v[:, len(special) + 1] = 1e-42                     # a subnormal row
        v[:, len(special) + 2] = 0.0
        v[0, len(special) + 2] = 1e-44                     # a / 127 underflows
        v[k // 2, len(special) + 3:len(special) + 8] = 0.0  # planted zeros in ordinary rows
    h = handle(capi, n, k, k1, task, (w0, w, v))
    try:
        _, w_dev, v_dev = h.get_params()
        info = h.compact_begin(capi.COMPACT_INT8)
        cw, cv = h.compact_rows(np.arange(n, dtype=np.uint32))
        info2 = h.compact_begin(capi.COMPACT_INT8)
        cw2, cv2 = h.compact_rows(np.arange(n, dtype=np.uint32))
        _, w_after, v_after = h.get_params()
        v32 = v_dev.astype(np.float32).reshape(k, n)
        want = compact.int8_dequant(*compact.int8_quant(v32))
        got = cv.astype(np.float32).reshape(k, n)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(nan, np.broadcast_to(nan.any(axis=0), nan.shape))          # NaN for a whole row, or not at all
        assert np.array_equal(bits(got)[~nan], bits(want)[~nan])
        assert np.array_equal(cv.reshape(k, n)[~nan], got[~nan].astype(np.float64))       # (widened to double exactly)
        assert np.array_equal(cw, w_dev)                                                  # w_j unchanged
        assert same_bits(w_after, w_dev) and same_bits(v_after[~np.isnan(v_dev)], v_dev[~np.isnan(v_dev)])   # the model is not written
        assert np.all(got[v32 == 0][~nan[v32 == 0]] == 0)                                 # exact zeros stay zero
        mx, ss, nf = compact.quant_report(v32, format="int8")
        print("k %d n %d: max_abs_err %.17g (want %.17g) sum_sq_err %.17g (want %.17g) nonfinite %d (want %d) bytes %d / %d" % (
            k, n, info.max_abs_err, mx, info.sum_sq_err, ss, info.nonfinite, nf, info.bytes_compact, info.bytes_params))
        assert info.max_abs_err == mx and info.nonfinite == nf
        assert abs(info.sum_sq_err - ss) <= 1e-12 * ss
        p = compact.row_bytes("int8", k)
        assert p == ROW_BYTES.get(k, p) == capi.load().fmx_compact_row_bytes(capi.COMPACT_INT8, k)
        assert info.features == n and info.bytes_compact == n * p
        assert info.bytes_params == h.info().bytes_params == n * (4 * row_stride(k) + 4)
        if k >= 1 and n >= 2 * len(special) + 8:
            assert nf == 6 * k and mx > 0                                                 # +inf, -inf, NaN: three whole rows at each end
        # two calls agree bit for bit
        assert (info2.max_abs_err, info2.nonfinite, info2.bytes_compact) == (info.max_abs_err, info.nonfinite, info.bytes_compact)
        assert np.float64(info2.sum_sq_err).tobytes() == np.float64(info.sum_sq_err).tobytes()
        assert same_bits(cw2, cw) and np.asarray(cv2).tobytes() == np.asarray(cv).tobytes()
        # w0: an empty row scores the bias alone
        ent, rp, y = make_rows(n, 3, task)
        h.upload_rows(0, ent, rp, y)
        assert h.compact_predict(0, ROWS)[0] == float(np.float32(w0))
    finally:
        h.close()


# ---- 2. predict -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, n, k1, task", CASES, ids=IDS)
def test_predict_matches_the_restatement_and_the_bound(capi, k, n, k1, task):
    ent, rp, y = make_rows(n, 10 + k, task)
    params = make_params(n, k, k + 1)
    h = handle(capi, n, k, k1, task, params)
    try:
        h.upload_rows(0, ent, rp, y)
        w0, w_dev, v_dev = h.get_params()
        v_dev = np.asarray(v_dev).reshape(k, n)
        fp32 = h.predict(0, ROWS)
        h.compact_begin(capi.COMPACT_INT8)
        got = h.compact_predict(0, ROWS)
        again = h.compact_predict(0, ROWS)
        want = model_of(w0, w_dev, v_dev, k1).predict(ent, rp)
        bound = int8_bound(ent, rp, v_dev) + RTOL * np.abs(fp32) + ATOL
        print("k %d n %d: |compact - restatement| max %.3g (allowed %.3g at that row); |compact - fp32| max %.3g, largest share of its "
              "bound %.3g" % (k, n, np.abs(got - want).max(), (RTOL * np.abs(want) + ATOL)[np.argmax(np.abs(got - want))],
                              np.abs(got - fp32).max(), (np.abs(got - fp32) / bound).max()))
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
        assert same_bits(got, again)
        assert np.all(np.abs(got - fp32) <= bound)
        assert same_bits(h.predict(0, ROWS), fp32)
        # a model that int8 holds exactly (requantising the dequantised table is the identity): the snapshot scores what the model scores
        if k:
            vq = compact.int8_round(v_dev.astype(np.float32)).astype(np.float64)
            h.set_params(w0, w_dev, vq)
            info = h.compact_begin(capi.COMPACT_INT8)
            assert info.max_abs_err == 0.0 and info.sum_sq_err == 0.0
            np.testing.assert_allclose(h.compact_predict(0, ROWS), h.predict(0, ROWS), rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(h.compact_predict(0, ROWS), want, rtol=RTOL, atol=ATOL)
    finally:
        h.close()


def test_a_nonfinite_row_scores_nan_and_no_other_row_does(capi):
    k, n = 64, 200
    ent, rp, y = make_rows(n, 99, 1)
    w0, w, v = make_params(n, k, 3)
    j = int(ent["id"][int(rp[5])])                          # a feature of row 5
    v[17, j] = np.inf
    h = handle(capi, n, k, True, 1, (w0, w, v))
    try:
        h.upload_rows(0, ent, rp, y)
        info = h.compact_begin(capi.COMPACT_INT8)
        got, fp32 = h.compact_predict(0, ROWS), h.predict(0, ROWS)
        touched = np.array([j in ent["id"][int(rp[r]):int(rp[r + 1])] for r in range(ROWS)])
        assert info.nonfinite == k and touched[5]
        assert np.array_equal(np.isnan(got), touched) and np.all(~np.isfinite(fp32[touched]))
    finally:
        h.close()


def test_more_rows_than_resident_waves_and_ids_beyond_2_16(capi):
    """the regime the format is for: k_rowsums' loop over several examples per wavefront, k_compact_quant8's loop over several features
    per wavefront, feature ids in the millions; and the snapshot taken in turns with a bf16 one, as scripts/compact_rate.py takes it"""
    n, k, rows, nnz = 3_000_000, 64, 40_000, 8
    rng = np.random.default_rng(123)
    ent = np.zeros(rows * nnz, dtype=compact_dtype())
    ent["id"] = rng.integers(0, n, rows * nnz)
    ent["id"][:nnz] = np.arange(n - nnz, n)                                     # the last features of the table
    ent["value"] = np.round(rng.normal(0.0, 1.0, rows * nnz), 3)
    rp = (np.arange(rows + 1) * nnz).astype(np.uint64)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    h = capi.Handle(n, k, True, True, 1, 0.0, 0.001, 0.002, 0.01, -1.0, 1.0)
    try:
        h.init_params(0.0, 0.05, 7)
        h.upload_rows(0, ent, rp, y)
        fp32 = h.predict(0, rows)
        ids, inv = np.unique(ent["id"], return_inverse=True)
        assert ids.max() == n - 1 and ids.max() > 2 ** 16
        wr, vr = h.get_param_rows(ids.astype(np.uint32))
        local = ent.copy()
        local["id"] = inv
        want = compact.CompactModel(0.0, wr, vr, True, True, format="int8").predict(local, rp)
        want_v = compact.int8_round(np.asarray(vr, dtype=np.float32))
        bound = int8_bound(local, rp, np.asarray(vr)) + RTOL * np.abs(fp32) + ATOL
        for turn in range(3):
            h.compact_begin(capi.COMPACT_BF16)
            pb = h.compact_predict(0, rows)
            info = h.compact_begin(capi.COMPACT_INT8)
            got = h.compact_predict(0, rows)
            cw, cv = h.compact_rows(ids.astype(np.uint32))
            print("turn %d: |compact - restatement| max %.3g, |compact - fp32| largest share of its bound %.3g, |bf16 - fp32| max %.3g" % (
                turn, np.abs(got - want).max(), (np.abs(got - fp32) / bound).max(), np.abs(pb - fp32).max()))
            assert info.nonfinite == 0 and info.bytes_compact == n * 128
            assert np.array_equal(bits(cv), bits(want_v)) and np.array_equal(cw, wr)
            np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
            assert np.all(np.abs(got - fp32) <= bound)
            np.testing.assert_allclose(pb, compact.CompactModel(0.0, wr, vr).predict(local, rp), rtol=RTOL, atol=ATOL)
    finally:
        h.close()


# ---- 3. the snapshot is frozen, the model is never written -----------------------------------------------------------------------
@pytest.mark.parametrize("k, n, k1, task", [(64, 4099, True, 1), (8, 200, True, 0), (100, 200, False, 1)], ids=["k64", "k8", "k100"])
def test_frozen_snapshot(capi, k, n, k1, task):
    ent, rp, y = make_rows(n, 20 + k, task)
    params = make_params(n, k, k + 2)
    h = handle(capi, n, k, k1, task, params, lr=0.05)
    all_ids = np.arange(n, dtype=np.uint32)
    try:
        h.upload_rows(0, ent, rp, y)
        h.upload_rows(1, ent, rp, y)
        p0 = h.predict(0, ROWS)
        t0 = h.topk(0, 1, 5)
        h.compact_begin(capi.COMPACT_INT8)
        c0 = h.compact_predict(0, ROWS)
        r0 = h.compact_rows(all_ids)
        assert same_bits(h.predict(0, ROWS), p0)                                # taking the snapshot wrote nothing
        h.sgd_epoch(0, capi.SGD_MINIBATCH, batch=16)
        p1 = h.predict(0, ROWS)
        assert not same_bits(p1, p0)
        assert same_bits(h.compact_predict(0, ROWS), c0)
        w0, w, v = params
        h.set_params(w0 + 1.0, w * 0.5, v * 2.0)
        p2 = h.predict(0, ROWS)
        assert not same_bits(p2, p1)
        assert same_bits(h.compact_predict(0, ROWS), c0)
        r1 = h.compact_rows(all_ids)
        assert same_bits(r1[0], r0[0]) and same_bits(r1[1], r0[1])
        h.compact_begin(capi.COMPACT_INT8)                                      # a second begin follows the model
        c2 = h.compact_predict(0, ROWS)
        assert not same_bits(c2, c0)
        w0d, wd, vd = h.get_params()
        np.testing.assert_allclose(c2, model_of(w0d, wd, np.asarray(vd).reshape(k, n), k1).predict(ent, rp), rtol=RTOL, atol=ATOL)
        assert same_bits(h.compact_predict(0, ROWS), c2)
        # a begin of the other format replaces the snapshot, and back
        ib = h.compact_begin(capi.COMPACT_BF16)
        assert ib.bytes_compact == n * (2 * row_stride(k) + 4)
        cb = h.compact_predict(0, ROWS)
        np.testing.assert_allclose(cb, compact.CompactModel(w0d, wd, vd, True, k1).predict(ent, rp), rtol=RTOL, atol=ATOL)
        assert not same_bits(cb, c2)
        assert np.array_equal(bits(h.compact_rows(all_ids)[1]), bits(compact.bf16_round(np.asarray(vd, dtype=np.float32))))
        i8 = h.compact_begin(capi.COMPACT_INT8)
        assert i8.bytes_compact == n * compact.row_bytes("int8", k)
        assert same_bits(h.compact_predict(0, ROWS), c2)
        h.compact_end()
        assert same_bits(h.predict(0, ROWS), p2)                                # begin .. end never wrote the model
        h.set_params(*params)
        t1 = h.topk(0, 1, 5)
        assert same_bits(h.predict(0, ROWS), p0) and np.array_equal(t0[0], t1[0]) and same_bits(t0[1], t1[1])
        with pytest.raises(capi.FmxError) as ei:
            h.compact_predict(0, ROWS)
        assert ei.value.code == -3
    finally:
        h.close()


def test_snapshot_inside_an_open_ftrl_session(capi):
    k, n, task = 16, 200, 1
    ent, rp, y = make_rows(n, 77, task)
    params = make_params(n, k, 9)
    finals = []
    for with_snapshot in (False, True):
        h = handle(capi, n, k, True, task, params, lr=0.05)
        try:
            h.upload_rows(0, ent, rp, y)
            h.ftrl_begin(0.05, 1.0, 0.001, 0.001, 0.01, 0.01, 0.0)
            h.ftrl_epoch(0, 16, 4)
            if with_snapshot:
                info = h.compact_begin(capi.COMPACT_INT8)
                w0d, wd, vd = h.get_params()
                vd = np.asarray(vd).reshape(k, n)
                c = h.compact_predict(0, ROWS)
                np.testing.assert_allclose(c, model_of(w0d, wd, vd).predict(ent, rp), rtol=RTOL, atol=ATOL)
                assert info.features == n
            h.ftrl_epoch(0, 16, 4)
            if with_snapshot:
                assert same_bits(h.compact_predict(0, ROWS), c)
            finals.append(h.get_params())
            zs = h.ftrl_state_rows(np.arange(n, dtype=np.uint32))
            finals[-1] = finals[-1] + tuple(zs)
        finally:
            h.close()
    for a, b in zip(*finals):
        assert same_bits(a, b)


def test_ftrl_zeros_are_still_zero_in_the_snapshot(capi):
    k, n, task = 16, 200, 1
    ent, rp, y = make_rows(n, 78, task)
    h = handle(capi, n, k, True, task, make_params(n, k, 10), lr=0.05)
    try:
        h.upload_rows(0, ent, rp, y)
        h.ftrl_begin(0.05, 1.0, 0.0, 5.0, 0.01, 0.01, 0.0)              # an L1 on the factors that no touched coordinate survives
        h.ftrl_epoch(0, 16, 4)
        h.compact_begin(capi.COMPACT_INT8)
        _, _, vd = h.get_params()
        _, cv = h.compact_rows(np.arange(n, dtype=np.uint32))
        zeros = np.asarray(vd) == 0
        print("ftrl: %d of %d factors are zero, %d rows are all zero" % (zeros.sum(), zeros.size, zeros.all(axis=0).sum()))
        assert zeros.any() and not zeros.all() and np.all(cv[zeros] == 0)
    finally:
        h.close()


# ---- 4. metrics -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, n, k1, task", [c for c in CASES if c[1] > 1][:10], ids=[i for c, i in zip(CASES, IDS) if c[1] > 1][:10])
def test_metrics_equal_the_formulas_on_the_snapshots_own_scores(capi, k, n, k1, task):
    ent, rp, y = make_rows(n, 30 + k, task)
    h = handle(capi, n, k, k1, task, make_params(n, k, k + 3))
    try:
        h.upload_rows(0, ent, rp, y)
        h.compact_begin(capi.COMPACT_INT8)
        p = h.compact_predict(0, ROWS)
        ev = h.compact_evaluate(0)
        assert ev.rows == ROWS and ev.device_seconds > 0 and (ev.flags & capi.EVAL_WSIDE) == 0
        if task == 0:
            err = np.maximum(-1.0, np.minimum(1.0, p)) - y.astype(np.float64)
            rmse, mae = math.sqrt(float(np.mean(err * err))), float(np.mean(np.abs(err)))
            ex = h.compact_evaluate_ex(0)
            print("k %d: rmse %.17g / %.17g / %.17g  mae %.17g / %.17g / %.17g" % (k, ev.rmse, ex.rmse, rmse, ev.mae, ex.mae, mae))
            for got in (ev, ex):
                assert abs(got.rmse - rmse) <= 1e-12 and abs(got.mae - mae) <= 1e-12
            assert ex.rows == ROWS and math.isnan(ex.auc) and math.isnan(ex.logloss)
        else:
            for link_name, link in (("logistic", capi.LINK_LOGISTIC), ("probit", capi.LINK_PROBIT)):
                ex = h.compact_evaluate_ex(0, link)
                want = classification_metrics(p, y, link_name)
                print("k %d %s: auc_num2 %d / %d  logloss %.17g / %.17g" % (k, link_name, ex.auc_num2, want["auc_num2"], ex.logloss,
                                                                             want["logloss"]))
                assert {f: int(getattr(ex, f)) for f in INT_FIELDS} == {f: want[f] for f in INT_FIELDS}
                assert ex.auc == want["auc_num2"] / (2 * want["pos"] * want["neg"])
                assert abs(ex.logloss - want["logloss"]) <= logloss_bound(want["logloss"], ROWS)
                assert ex.accuracy == want["correct"] / ROWS and ex.device_seconds > 0
            assert ev.accuracy == want["correct"] / ROWS
    finally:
        h.close()


# ---- 5. top-K -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, K", [(0, 5), (1, 10), (8, 100), (24, 7), (57, 10), (64, 10), (100, 33), (121, 10), (256, 10)])
def test_topk_from_the_snapshot(capi, oracle, k, K):
    n, nq, nc = 200, 20, 130
    rng = np.random.default_rng(40 + k)
    qe, qr, _ = make_rows(n, 41 + k, 0)
    qe, qr = qe[:int(qr[nq])], qr[:nq + 1]
    sizes = rng.integers(0, 9, nc)
    cr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ce = np.zeros(int(cr[-1]), dtype=compact_dtype())
    ce["id"], ce["value"] = rng.integers(0, n, len(ce)), np.round(rng.normal(0, 1, len(ce)), 3)
    exclude = [rng.choice(nc, size=int(rng.integers(0, 6)), replace=False) for _ in range(nq)]
    h = handle(capi, n, k, True, 0, make_params(n, k, k + 4))
    try:
        h.upload_rows(0, qe, qr, np.zeros(nq, np.float32))
        h.upload_rows(1, ce, cr, np.zeros(nc, np.float32))
        before = h.topk(0, 1, K, exclude=exclude)
        h.compact_begin(capi.COMPACT_INT8)
        idx, sc, st = h.compact_topk(0, 1, K, exclude=exclude, stats=True)
        idx2, sc2 = h.compact_topk(0, 1, K, exclude=exclude)
        after = h.topk(0, 1, K, exclude=exclude)
        w0, _, _ = h.get_params()
        cw, cv = h.compact_rows(np.arange(n, dtype=np.uint32))
        h.compact_end()
        ended = h.topk(0, 1, K, exclude=exclude)
    finally:
        h.close()
    assert np.array_equal(before[0], after[0]) and same_bits(before[1], after[1])
    assert np.array_equal(before[0], ended[0]) and same_bits(before[1], ended[1])
    assert np.array_equal(idx, idx2) and same_bits(sc, sc2)
    assert st.scores == nq * nc and st.device_seconds > 0
    m = oracle.Model(n, k)
    m.w0, m.w[:], m.v[:] = w0, cw, cv
    ref = T.scores_decomposed(m, qe, qr, ce, cr)
    check_lists(idx, sc, ref, K, exclude)
    if k >= 8:                                                                  # (the snapshot's lists are its own, not the model's)
        assert not same_bits(sc, before[1])


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(capi):
    lib = capi.load()
    k, n = 8, 200
    ent, rp, y = make_rows(n, 50, 1)
    h = handle(capi, n, k, True, 1, make_params(n, k, 5))
    out_p = np.zeros(ROWS)
    ev, ex, info = capi.Eval(), capi.EvalEx(), capi.CompactInfo()
    idx, sc = np.zeros((ROWS, 3), dtype=np.uint32), np.zeros((ROWS, 3))
    ids, wv = np.arange(4, dtype=np.uint32), np.zeros(4 * (k + 1))
    topts = capi.TopkOpts(3, 0, 0, ROWS, 0, None, None)
    good = capi.CompactOpts(capi.COMPACT_INT8, 0)

    def refused(rc, code, name):
        assert rc == code, (name, rc)
        assert name.encode() in lib.fmx_last_error(h.h), lib.fmx_last_error(h.h)

    def usable():
        assert lib.fmx_compact_begin(h.h, C.byref(good), C.byref(info)) == 0 and info.features == n and info.bytes_compact == n * 16
        assert np.all(np.isfinite(h.compact_predict(0, ROWS)))

    try:
        h.upload_rows(0, ent, rp, y)
        h.upload_rows(2, ent, rp, None)                                          # a slot without targets
        refused(lib.fmx_compact_predict(h.h, 0, out_p.ctypes.data), -3, "fmx_compact_predict")      # no snapshot yet
        # _begin's own arguments
        refused(lib.fmx_compact_begin(h.h, None, C.byref(info)), -1, "fmx_compact_begin")
        for fmt in (0, 2, 4):
            refused(lib.fmx_compact_begin(h.h, C.byref(capi.CompactOpts(fmt, 0)), C.byref(info)), -1, "fmx_compact_begin")
        refused(lib.fmx_compact_begin(h.h, C.byref(capi.CompactOpts(capi.COMPACT_INT8, 1)), C.byref(info)), -1, "fmx_compact_begin")
        refused(lib.fmx_compact_end(h.h), -3, "fmx_compact_end")                 # (none of them left a snapshot behind)
        usable()
        assert lib.fmx_compact_begin(h.h, C.byref(good), None) == 0             # info may be NULL
        refused(lib.fmx_compact_begin(h.h, C.byref(capi.CompactOpts(2, 0)), C.byref(info)), -1, "fmx_compact_begin")
        assert np.all(np.isfinite(h.compact_predict(0, ROWS)))                   # (a refused begin keeps the snapshot there was)
        # NULL outputs
        refused(lib.fmx_compact_predict(h.h, 0, None), -1, "fmx_compact_predict")
        refused(lib.fmx_compact_evaluate(h.h, 0, None), -1, "fmx_compact_evaluate")
        refused(lib.fmx_compact_evaluate_ex(h.h, 0, None, None), -1, "fmx_compact_evaluate_ex")
        refused(lib.fmx_compact_topk(h.h, 0, 0, C.byref(topts), None, sc.ctypes.data, None), -1, "fmx_compact_topk")
        refused(lib.fmx_compact_get_rows(h.h, None, 4, wv.ctypes.data, wv.ctypes.data), -1, "fmx_compact_get_rows")
        refused(lib.fmx_compact_get_rows(h.h, ids.ctypes.data, 4, wv.ctypes.data, None), -1, "fmx_compact_get_rows")
        bad = np.array([0, n], dtype=np.uint32)                                  # an id >= num_attribute
        refused(lib.fmx_compact_get_rows(h.h, bad.ctypes.data, 2, wv.ctypes.data, wv.ctypes.data), -1, "fmx_compact_get_rows")
        refused(lib.fmx_compact_evaluate_ex(h.h, 0, C.byref(capi.EvalOpts(2, 0)), C.byref(ex)), -1, "fmx_compact_evaluate_ex")
        refused(lib.fmx_compact_topk(h.h, 0, 0, None, idx.ctypes.data, sc.ctypes.data, None), -1, "fmx_compact_topk")
        usable()
        # slots: out of range, never uploaded, without targets where targets are needed
        refused(lib.fmx_compact_predict(h.h, 99, out_p.ctypes.data), -1, "fmx_compact_predict")
        refused(lib.fmx_compact_predict(h.h, 5, out_p.ctypes.data), -3, "fmx_compact_predict")
        refused(lib.fmx_compact_evaluate(h.h, 2, C.byref(ev)), -3, "fmx_compact_evaluate")
        refused(lib.fmx_compact_evaluate_ex(h.h, 2, None, C.byref(ex)), -3, "fmx_compact_evaluate_ex")
        assert lib.fmx_compact_predict(h.h, 2, out_p.ctypes.data) == 0          # (predict needs no targets)
        usable()
        # kept `-relation` blocks
        main = np.zeros(6, dtype=capi.ENTRY_DTYPE)
        main["id"], main["value"] = np.arange(6), 1.0
        bent = np.zeros(3, dtype=capi.ENTRY_DTYPE)
        bent["id"], bent["value"] = np.arange(3), 0.5
        rel = [(bent, np.arange(4, dtype=np.uint64), np.array([0, 1, 2, 0, 1, 2], dtype=np.uint32), 10)]
        h.upload_block_rows(3, main, np.arange(7, dtype=np.uint64), np.ones(6, np.float32), rel, keep=True)
        refused(lib.fmx_compact_predict(h.h, 3, out_p.ctypes.data), -4, "fmx_compact_predict")
        refused(lib.fmx_compact_evaluate(h.h, 3, C.byref(ev)), -4, "fmx_compact_evaluate")
        refused(lib.fmx_compact_topk(h.h, 3, 0, C.byref(capi.TopkOpts(3, 0, 0, 6, 0, None, None)), idx.ctypes.data, sc.ctypes.data, None),
                -4, "fmx_compact_topk")
        usable()
        assert lib.fmx_compact_end(h.h) == 0
        assert np.all(np.isfinite(h.predict(0, ROWS)))
    finally:
        h.close()
    # a feature shard
    hs = handle(capi, n, k, True, 1, None, shard_rank=0, shard_world=2)
    try:
        assert lib.fmx_compact_begin(hs.h, C.byref(good), C.byref(info)) == -4
        assert b"fmx_compact_begin" in lib.fmx_last_error(hs.h)
        hs.upload_rows(0, ent, rp, y)                                           # (still usable)
    finally:
        hs.close()


# ---- 7. learners and CLI --------------------------------------------------------------------------------------------------------
def test_learner_view_and_cli_serve_int8(capi, tmp_path, capsys):
    from libfm_amd import cli
    from libfm_amd import data as D
    from libfm_amd import learner as L
    k, iters = 8, 3
    tr_raw, te_raw = tiny_regression(1), tiny_regression(2)
    trf, tef, outp, outs, outb = (str(tmp_path / f) for f in ("tr.libfm", "te.libfm", "plain.txt", "serve.txt", "bf16.txt"))
    write_libfm(trf, *tr_raw)
    write_libfm(tef, *te_raw)
    tr, te = L.Data(*D.load(trf)), L.Data(*D.load(tef))
    l = trained_learner(L, tr, te, k, iters)
    try:
        fp32_metric = l.evaluate(te)
        view = l.compact(format="int8")
        assert view.format == "int8"
        v_dev = np.asarray(l.fm.v, dtype=np.float64).reshape(k, -1)
        raw = l.predict_raw(te)
        bound = int8_bound(te.entries, te.row_ptr, v_dev) + RTOL * np.abs(raw) + ATOL
        got = view.evaluate(te)
        print("learner: rmse fp32 %.9g int8 %.9g, allowed difference %.3g; max_abs_err %.3g" % (fp32_metric, got, bound.max(),
                                                                                                view.info.max_abs_err))
        assert abs(got - fp32_metric) <= bound.max()                            # (rmse and the clamp are 1-Lipschitz in the scores)
        assert np.all(np.abs(view.predict_raw(te) - raw) <= bound)
        want_out = view.predict(te)
        assert np.all(want_out >= l.min_target) and np.all(want_out <= l.max_target)
        assert view.info.bytes_compact == l.fm.num_attribute * 16 and view.info.nonfinite == 0
        bytes_compact = int(view.info.bytes_compact)
        idx, sc = view.recommend(te, tr, 5)
        assert idx.shape == (te.num_cases, 5) and np.all(np.diff(sc, axis=1) <= 0)
        view.close()
        with pytest.raises(capi.FmxError):
            l._h.compact_predict(l._slot(te), te.num_cases)
    finally:
        l.close()
    capsys.readouterr()
    argv = ["-task", "r", "-train", trf, "-test", tef, "-dim", "1,1,%d" % k, "-iter", str(iters), "-method", "sgd", "-learn_rate", "0.02",
            "-init_stdev", "0.1", "-seed", "42"]
    assert cli.main(argv + ["-out", outp]) == 0
    plain = capsys.readouterr()
    assert cli.main(argv + ["-out", outs, "-serve", "int8"]) == 0
    served = capsys.readouterr()
    assert served.out == plain.out and plain.out.count("#Iter=") == iters
    extra = served.err[len(plain.err):]
    assert served.err.startswith(plain.err) and extra.count("\n") == 1 and extra.startswith("compact\tformat=int8\tbytes=")
    fields = dict(f.split("=") for f in extra.strip().split("\t")[1:])
    assert int(fields["bytes"]) == bytes_compact and int(fields["bytes_fp32"]) > bytes_compact
    assert int(fields["nonfinite"]) == 0 and float(fields["max_abs_err"]) > 0
    assert float(fields["Test(fp32)"]) == pytest.approx(fp32_metric, rel=1e-5)
    assert float(fields["Test(int8)"]) == pytest.approx(got, rel=1e-5)
    p_plain = np.array([float(x) for x in open(outp).read().split()])
    p_serve = np.array([float(x) for x in open(outs).read().split()])
    np.testing.assert_allclose(p_serve, want_out, rtol=1e-5, atol=1e-9)          # (%g keeps 6 digits)
    assert not np.array_equal(p_serve, p_plain)
    assert cli.main(argv + ["-out", outb, "-serve", "bf16"]) == 0                # bf16 still says bf16
    assert "compact\tformat=bf16\tbytes=" in capsys.readouterr().err
    assert cli.main(argv + ["-serve", "int8", "-method", "mcmc"]) == 0
    assert "ERROR: -serve is not supported with -method mcmc" in capsys.readouterr().err


def test_als_learner_view_int8(capi):
    from libfm_amd import learner as L
    tr, te = L.Data(*tiny_regression(3)), L.Data(*tiny_regression(4))
    l = L.FMLearnALS()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor = 60, 4
    l.fm.init(np.random.default_rng(3))
    l.task, l.num_iter, l.min_target, l.max_target = L.TASK_REGRESSION, 2, tr.min_target, tr.max_target
    l.w_lambda = l.v_lambda = 1.0
    l.out = io.StringIO()
    l.init()
    try:
        l.learn(tr, te)
        view = l.compact("int8")
        raw = l._h.predict(1, te.num_cases)
        bound = int8_bound(te.entries, te.row_ptr, np.asarray(l.fm.v).reshape(4, -1)) + RTOL * np.abs(raw) + ATOL
        assert view.info.bytes_compact == 60 * 16
        assert np.all(np.abs(view.predict_raw(te) - raw) <= bound)
        assert abs(view.evaluate(te) - l.evaluate(te)) <= bound.max()
        assert np.array_equal(view.predict(te), np.maximum(l.min_target, np.minimum(l.max_target, view.predict_raw(te))))
        view.close()
    finally:
        l.close()
