"""GPU: the bf16 serving snapshot (fmx_compact_*, k_compact_quant, k_rowsums and k_fetch_rows over RowsBf16; include/fmx.h)
against libfm_amd/compact.py (itself pinned to torch's bfloat16 conversion and to the fp64 oracle in tests/test_compact_cpu.py).

Shapes.  k in {0, 1, 2, 4, 8, 16, 32, 64, 100, 128, 256, 300, 512, 1000}: every lane map of the bf16 row source (MapC: 2-byte loads,
4-byte loads on 1 .. 32 lanes per row, one row per wavefront with 4 / 8 / 16 / 2 x 16-byte loads) and row strides that are not the
padded power of two (k = 100: 112 elements; k = 300: 304 of 512, whole lanes past the row read zeros; k = 1000: 1008 of 1024, lane
63 is empty).  n in {1, 200, 4099}.  Slots of 47 rows whose lengths include 0, 1, 2, 33, 64, 65 and 130: the second 64-entry block and every tail of
the round loop; one row repeats an id; values are seeded reals.

Tolerances.  Scores: the project's predict tolerance rtol 1e-4 / atol 2e-5 (tests/test_gpu_parity.py::test_predict_matches_reference)
-- the arithmetic is k_rowsums', only the load differs.  bf16 against fp32: round to nearest changes every factor by at most
u = 2^-8 relative, a product v_if x_i v_jf x_j by at most 2u + u^2, so |compact - fmx_predict| <= (2u + u^2) A_e on top of that
tolerance, A_e = sum_{i<j} sum_f |v_if x_i| |v_jf x_j| in fp64.  Quantiser: bit patterns and the maximum are exact (v - q(v) is exact
in fp32), sum_sq_err rtol 1e-12 (an fp64 sum of at most 1e6 terms in another order).  Metrics: integer fields exact, log loss within
test_gpu_eval_ex.logloss_bound, rmse / mae 1e-12 as there.

Measured on an MI355X (largest over the cases; every test prints its own figures): snapshot rows, max_abs_err and nonfinite equal;
sum_sq_err 4e-16 relative; compact_predict against the restatement 3.3e-6 absolute where 1.8e-3 is allowed; |compact - fmx_predict|
0.0108 absolute, at most 0.144 of its bound; counts and AUC numerators equal, log loss 2e-16 relative, rmse / mae to the last digit."""
import ctypes as C
import io
import math

import numpy as np
import pytest

import topk_oracle as T
from libfm_amd import compact
from libfm_amd.evalmetrics import classification_metrics
from test_compact_cpu import planted
from test_gpu_eval_ex import INT_FIELDS, logloss_bound
from test_gpu_topk import check_lists

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
U = 2.0 ** -8
ROWS = 47
LENGTHS = (0, 1, 2, 33, 64, 65, 130)
# (k, n, k1, task): every k, every n, k1 on and off, both tasks
CASES = [(0, 200, True, 0), (1, 4099, True, 1), (2, 200, False, 0), (8, 4099, True, 1), (16, 200, True, 0), (64, 4099, True, 1),
         (64, 200, False, 0), (100, 4099, True, 0), (128, 200, True, 1), (256, 200, False, 1), (8, 1, True, 0), (64, 1, True, 1),
         (0, 1, False, 1),
         # the widths whose lane maps nothing else runs: 2 and 16 lanes per row, and row_ld_c's 16-byte loads with lanes past the row
         (4, 200, True, 1), (32, 200, False, 0), (300, 200, True, 0), (512, 200, False, 1), (1000, 200, True, 1)]
IDS = ["k%d-n%d-%s-%s" % (k, n, "k1" if k1 else "nok1", "cr"[1 - t]) for k, n, k1, t in CASES]


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


def row_stride(k):
    """Tab::rs of fmx_create: the lane map's power of two, cut to k rounded up to 16 from 32 on"""
    kp = 1
    while kp < max(k, 1):
        kp *= 2
    return kp if kp < 32 else min(kp, (k + 15) // 16 * 16)


def make_rows(n, seed, task):
    """ROWS rows over n features: LENGTHS first, then seeded lengths up to 40; ids distinct inside a row where n allows, row 7 repeats
    an id; real values; targets +-1 or real"""
    rng = np.random.default_rng(seed)
    sizes = list(LENGTHS) + [int(x) for x in rng.integers(2, 41, ROWS - len(LENGTHS))]
    ids, vals = [], []
    for z in sizes:
        ids.append(rng.choice(n, size=z, replace=False) if z <= n else rng.integers(0, n, z))
        x = np.round(rng.normal(0.0, 1.0, z), 3)
        x[x == 0] = 0.5
        vals.append(x)
    ids[7][1] = ids[7][0]
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ent = np.zeros(int(rp[-1]), dtype=compact_dtype())
    ent["id"], ent["value"] = np.concatenate(ids), np.concatenate(vals)
    y = np.where(rng.random(ROWS) < 0.4, 1.0, -1.0) if task == 1 else np.round(rng.normal(0.0, 1.0, ROWS), 3)
    return ent, rp, y.astype(np.float32)


def compact_dtype():
    return np.dtype([("id", np.uint32), ("value", np.float32)])


def make_params(n, k, seed):
    """w0, w, v with |v| ~ 0.3 / sqrt(k): a row's sum of squares does not grow with k, so the fp32 error of a score stays far
    inside the tolerance at every width"""
    rng = np.random.default_rng(500 + seed)
    return 0.3, rng.normal(0.0, 0.3, n), rng.normal(0.0, 0.3 / math.sqrt(max(k, 1)), (k, n))


def handle(capi, n, k, k1, task, params=None, lr=0.01, **kw):
    h = capi.Handle(n, k, True, k1, task, 0.0, 0.001, 0.002, lr, -1.0, 1.0, **kw)
    if params is not None:
        h.set_params(*params)
    return h


def pair_mass(ent, rp, v):
    """A_e = sum_{i<j} sum_f |v_if x_i| |v_jf x_j| per row, fp64 (v: [k][n])"""
    rp = np.asarray(rp, dtype=np.int64)
    n = len(rp) - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    ids, xs = ent["id"].astype(np.int64), np.abs(ent["value"].astype(np.float64))
    out = np.zeros(n)
    for f in range(v.shape[0]):
        a = np.abs(v[f, ids]) * xs
        s = np.bincount(row, weights=a, minlength=n)
        out += 0.5 * (s * s - np.bincount(row, weights=a * a, minlength=n))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


# ---- 1. the quantiser -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, n, k1, task", CASES, ids=IDS)
def test_quantiser_bit_exact_and_report(capi, k, n, k1, task):
    w0, w, v = make_params(n, k, k)
    px, _ = planted()
    special = np.concatenate([px, np.array([np.nan], dtype=np.float32)]).astype(np.float64)
    if k >= 1 and n >= len(special):                       # the planted values of the CPU test, through fmx_set_params
        v[0, :len(special)] = special
        v[k - 1, n - len(special):] = special[::-1]
    h = handle(capi, n, k, k1, task, (w0, w, v))
    try:
        _, w_dev, v_dev = h.get_params()
        info = h.compact_begin()
        cw, cv = h.compact_rows(np.arange(n, dtype=np.uint32))
        _, w_after, v_after = h.get_params()
        rs = row_stride(k)
        want = compact.bf16_round(v_dev.astype(np.float32))
        got = cv.astype(np.float32)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(bits(got)[~nan], bits(want)[~nan])
        assert np.array_equal(cv[~nan], got[~nan].astype(np.float64))          # (the dequantised values are exact in fp64)
        assert np.array_equal(cw, w_dev)                                        # w is a plain copy
        assert same_bits(w_after, w_dev) and same_bits(v_after[~np.isnan(v_dev)], v_dev[~np.isnan(v_dev)])   # the model is not written
        mx, ss, nf = compact.quant_report(v_dev)
        print("k %d n %d: max_abs_err %.6g (want %.6g) sum_sq_err %.17g (want %.17g) nonfinite %d (want %d) bytes %d / %d" % (
            k, n, info.max_abs_err, mx, info.sum_sq_err, ss, info.nonfinite, nf, info.bytes_compact, info.bytes_params))
        assert info.max_abs_err == mx and info.nonfinite == nf
        assert abs(info.sum_sq_err - ss) <= 1e-12 * ss
        assert info.features == n and info.bytes_compact == n * (2 * rs + 4)
        assert info.bytes_params == h.info().bytes_params == n * (4 * rs + 4)
        if k >= 1 and n >= len(special):
            assert nf == 2 * 5 and mx > 0                                       # 3.4e38 -> inf twice, +-inf, NaN; in both rows
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
        fp32 = h.predict(0, ROWS)
        h.compact_begin()
        got = h.compact_predict(0, ROWS)
        again = h.compact_predict(0, ROWS)
        cm = compact.CompactModel(w0, w_dev, v_dev, True, k1)
        want = cm.predict(ent, rp)
        bound = (2 * U + U * U) * pair_mass(ent, rp, v_dev) + RTOL * np.abs(fp32) + ATOL
        print("k %d n %d: |compact - restatement| max %.3g (allowed %.3g at that row); |compact - fp32| max %.3g, largest share of its "
              "bound %.3g" % (k, n, np.abs(got - want).max(), (RTOL * np.abs(want) + ATOL)[np.argmax(np.abs(got - want))],
                              np.abs(got - fp32).max(), (np.abs(got - fp32) / bound).max()))
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
        assert same_bits(got, again)
        assert np.all(np.abs(got - fp32) <= bound)
        # a model that bf16 holds exactly: the snapshot scores what the model scores
        vq = compact.bf16_round(v_dev.astype(np.float32)).astype(np.float64)
        h.set_params(w0, w_dev, vq)
        h.compact_begin()
        np.testing.assert_allclose(h.compact_predict(0, ROWS), h.predict(0, ROWS), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(h.compact_predict(0, ROWS), want, rtol=RTOL, atol=ATOL)
    finally:
        h.close()


# ---- 3. the snapshot is frozen, the model is never written -----------------------------------------------------------------------
@pytest.mark.parametrize("k, n, k1, task", [(64, 4099, True, 1), (8, 200, True, 0), (100, 200, False, 1)], ids=["k64", "k8", "k100"])
def test_frozen_snapshot(capi, k, n, k1, task):
    ent, rp, y = make_rows(n, 20 + k, task)
    params = make_params(n, k, k + 2)
    h = handle(capi, n, k, k1, task, params, lr=0.05)
    try:
        h.upload_rows(0, ent, rp, y)
        p0 = h.predict(0, ROWS)
        h.compact_begin()
        c0 = h.compact_predict(0, ROWS)
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
        h.compact_begin()                                                       # a second begin follows the model
        c2 = h.compact_predict(0, ROWS)
        assert not same_bits(c2, c0)
        w0d, wd, vd = h.get_params()
        np.testing.assert_allclose(c2, compact.CompactModel(w0d, wd, vd, True, k1).predict(ent, rp), rtol=RTOL, atol=ATOL)
        assert same_bits(h.compact_predict(0, ROWS), c2)
        h.compact_end()
        assert same_bits(h.predict(0, ROWS), p2)                                # begin .. end never wrote the model
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
                info = h.compact_begin()
                w0d, wd, vd = h.get_params()
                c = h.compact_predict(0, ROWS)
                np.testing.assert_allclose(c, compact.CompactModel(w0d, wd, vd).predict(ent, rp), rtol=RTOL, atol=ATOL)
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


# ---- 4. metrics -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, n, k1, task", [c for c in CASES if c[1] > 1][:10], ids=[i for c, i in zip(CASES, IDS) if c[1] > 1][:10])
def test_metrics_equal_the_formulas_on_the_snapshots_own_scores(capi, k, n, k1, task):
    ent, rp, y = make_rows(n, 30 + k, task)
    h = handle(capi, n, k, k1, task, make_params(n, k, k + 3))
    try:
        h.upload_rows(0, ent, rp, y)
        h.compact_begin()
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
@pytest.mark.parametrize("k, K", [(0, 5), (1, 10), (8, 100), (64, 10), (100, 33), (256, 10), (512, 10), (1000, 10)])
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
        h.compact_begin()
        idx, sc, st = h.compact_topk(0, 1, K, exclude=exclude, stats=True)
        after = h.topk(0, 1, K, exclude=exclude)
        w0, _, _ = h.get_params()
        cw, cv = h.compact_rows(np.arange(n, dtype=np.uint32))
    finally:
        h.close()
    assert np.array_equal(before[0], after[0]) and same_bits(before[1], after[1])
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
    good = capi.CompactOpts(capi.COMPACT_BF16, 0)

    def refused(rc, code, name):
        assert rc == code, (name, rc)
        assert name.encode() in lib.fmx_last_error(h.h), lib.fmx_last_error(h.h)

    def usable():
        assert lib.fmx_compact_begin(h.h, C.byref(good), C.byref(info)) == 0 and info.features == n
        assert np.all(np.isfinite(h.compact_predict(0, ROWS)))

    try:
        h.upload_rows(0, ent, rp, y)
        h.upload_rows(2, ent, rp, None)                                          # a slot without targets
        # no snapshot yet: every call but _begin
        refused(lib.fmx_compact_predict(h.h, 0, out_p.ctypes.data), -3, "fmx_compact_predict")
        refused(lib.fmx_compact_evaluate(h.h, 0, C.byref(ev)), -3, "fmx_compact_evaluate")
        refused(lib.fmx_compact_evaluate_ex(h.h, 0, None, C.byref(ex)), -3, "fmx_compact_evaluate_ex")
        refused(lib.fmx_compact_topk(h.h, 0, 0, C.byref(topts), idx.ctypes.data, sc.ctypes.data, None), -3, "fmx_compact_topk")
        refused(lib.fmx_compact_get_rows(h.h, ids.ctypes.data, 4, wv.ctypes.data, wv.ctypes.data), -3, "fmx_compact_get_rows")
        refused(lib.fmx_compact_end(h.h), -3, "fmx_compact_end")
        # _begin's own arguments
        refused(lib.fmx_compact_begin(h.h, None, C.byref(info)), -1, "fmx_compact_begin")
        refused(lib.fmx_compact_begin(h.h, C.byref(capi.CompactOpts(2, 0)), C.byref(info)), -1, "fmx_compact_begin")
        refused(lib.fmx_compact_begin(h.h, C.byref(capi.CompactOpts(0, 0)), C.byref(info)), -1, "fmx_compact_begin")
        refused(lib.fmx_compact_begin(h.h, C.byref(capi.CompactOpts(capi.COMPACT_BF16, 1)), C.byref(info)), -1, "fmx_compact_begin")
        usable()
        assert lib.fmx_compact_begin(h.h, C.byref(good), None) == 0             # info may be NULL
        # NULL outputs
        refused(lib.fmx_compact_predict(h.h, 0, None), -1, "fmx_compact_predict")
        refused(lib.fmx_compact_evaluate(h.h, 0, None), -1, "fmx_compact_evaluate")
        refused(lib.fmx_compact_evaluate_ex(h.h, 0, None, None), -1, "fmx_compact_evaluate_ex")
        refused(lib.fmx_compact_topk(h.h, 0, 0, C.byref(topts), None, sc.ctypes.data, None), -1, "fmx_compact_topk")
        refused(lib.fmx_compact_topk(h.h, 0, 0, C.byref(topts), idx.ctypes.data, None, None), -1, "fmx_compact_topk")
        refused(lib.fmx_compact_get_rows(h.h, None, 4, wv.ctypes.data, wv.ctypes.data), -1, "fmx_compact_get_rows")
        refused(lib.fmx_compact_get_rows(h.h, ids.ctypes.data, 4, None, wv.ctypes.data), -1, "fmx_compact_get_rows")
        refused(lib.fmx_compact_get_rows(h.h, ids.ctypes.data, 4, wv.ctypes.data, None), -1, "fmx_compact_get_rows")
        usable()
        # an id >= num_attribute
        bad = np.array([0, n], dtype=np.uint32)
        refused(lib.fmx_compact_get_rows(h.h, bad.ctypes.data, 2, wv.ctypes.data, wv.ctypes.data), -1, "fmx_compact_get_rows")
        # what fmx_evaluate_ex / fmx_topk refuse in their own arguments
        refused(lib.fmx_compact_evaluate_ex(h.h, 0, C.byref(capi.EvalOpts(2, 0)), C.byref(ex)), -1, "fmx_compact_evaluate_ex")
        refused(lib.fmx_compact_evaluate_ex(h.h, 0, C.byref(capi.EvalOpts(0, 1)), C.byref(ex)), -1, "fmx_compact_evaluate_ex")
        refused(lib.fmx_compact_topk(h.h, 0, 0, None, idx.ctypes.data, sc.ctypes.data, None), -1, "fmx_compact_topk")
        for o in (capi.TopkOpts(0, 0, 0, ROWS, 0, None, None), capi.TopkOpts(1025, 0, 0, ROWS, 0, None, None),
                  capi.TopkOpts(3, 1, 0, ROWS, 0, None, None), capi.TopkOpts(3, 0, 1, ROWS, 0, None, None)):
            refused(lib.fmx_compact_topk(h.h, 0, 0, C.byref(o), idx.ctypes.data, sc.ctypes.data, None), -1, "fmx_compact_topk")
        ex_ptr, ex_idx = np.zeros(ROWS + 1, dtype=np.uint64), np.array([ROWS], dtype=np.uint32)
        ex_ptr[1:] = 1
        o = capi.TopkOpts(3, 0, 0, ROWS, 0, ex_ptr.ctypes.data, ex_idx.ctypes.data)
        refused(lib.fmx_compact_topk(h.h, 0, 0, C.byref(o), idx.ctypes.data, sc.ctypes.data, None), -1, "fmx_compact_topk")
        usable()
        # slots: out of range, never uploaded, without targets where targets are needed
        refused(lib.fmx_compact_predict(h.h, 99, out_p.ctypes.data), -1, "fmx_compact_predict")
        refused(lib.fmx_compact_predict(h.h, 5, out_p.ctypes.data), -3, "fmx_compact_predict")
        refused(lib.fmx_compact_evaluate(h.h, 5, C.byref(ev)), -3, "fmx_compact_evaluate")
        refused(lib.fmx_compact_evaluate(h.h, 2, C.byref(ev)), -3, "fmx_compact_evaluate")
        refused(lib.fmx_compact_evaluate_ex(h.h, 5, None, C.byref(ex)), -3, "fmx_compact_evaluate_ex")
        refused(lib.fmx_compact_evaluate_ex(h.h, 2, None, C.byref(ex)), -3, "fmx_compact_evaluate_ex")
        assert lib.fmx_compact_topk(h.h, 0, 5, C.byref(topts), idx.ctypes.data, sc.ctypes.data, None) == -3
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
        refused(lib.fmx_compact_evaluate_ex(h.h, 3, None, C.byref(ex)), -4, "fmx_compact_evaluate_ex")
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
        assert lib.fmx_compact_predict(hs.h, 0, out_p.ctypes.data) == -4
        hs.upload_rows(0, ent, rp, y)                                           # (still usable)
    finally:
        hs.close()


# ---- 7. learner and CLI ---------------------------------------------------------------------------------------------------------
def write_libfm(path, ent, rp, y):
    with open(path, "w") as f:
        for r in range(len(y)):
            f.write("%g %s\n" % (y[r], " ".join("%d:%g" % (e["id"], e["value"]) for e in ent[int(rp[r]):int(rp[r + 1])])))


def tiny_regression(seed, rows=120, n=60):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 7, rows)
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ent = np.zeros(int(rp[-1]), dtype=compact_dtype())
    ent["id"] = np.concatenate([rng.choice(n, size=z, replace=False) for z in sizes])
    ent["value"] = np.round(rng.uniform(0.25, 1.5, len(ent)), 2)
    wtrue = rng.normal(0, 1, n)
    row = np.repeat(np.arange(rows), sizes)
    y = np.round(np.bincount(row, weights=wtrue[ent["id"]] * ent["value"], minlength=rows), 2)
    return ent, rp, y.astype(np.float32)


def trained_learner(L, tr, te, k, iters):
    """what `-task r -dim 1,1,k -iter iters -method sgd -learn_rate 0.02 -init_stdev 0.1 -seed 42` sets up and trains"""
    from libfm_amd import refrand as R
    fm = L.FMModel()
    fm.num_attribute, fm.num_factor, fm.init_stdev = max(tr.num_feature, te.num_feature), k, 0.1
    R.srand(42)
    fm.w0, fm.w = 0.0, np.zeros(fm.num_attribute)
    fm.v = R.init_v(k, fm.num_attribute, 0.0, 0.1)
    l = L.FMLearnSGD()
    l.fm, l.num_iter, l.task, l.learn_rate = fm, iters, L.TASK_REGRESSION, 0.02
    l.min_target, l.max_target = tr.min_target, tr.max_target
    l.out = io.StringIO()
    l.init()
    l.learn(tr, te)
    return l


def test_learner_view_and_cli_serve(capi, tmp_path, capsys):
    from libfm_amd import cli
    from libfm_amd import learner as L
    k, iters = 8, 3
    tr_raw, te_raw = tiny_regression(1), tiny_regression(2)
    trf, tef, outp, outs = (str(tmp_path / f) for f in ("tr.libfm", "te.libfm", "plain.txt", "serve.txt"))
    write_libfm(trf, *tr_raw)
    write_libfm(tef, *te_raw)
    from libfm_amd import data as D
    tr, te = L.Data(*D.load(trf)), L.Data(*D.load(tef))
    l = trained_learner(L, tr, te, k, iters)
    try:
        fp32_metric, fp32_pred = l.evaluate(te), l.predict(te)
        view = l.compact()
        v_dev = np.asarray(l.fm.v, dtype=np.float64).reshape(k, -1)
        raw = l.predict_raw(te)
        bound = (2 * U + U * U) * pair_mass(te.entries, te.row_ptr, v_dev) + RTOL * np.abs(raw) + ATOL
        got = view.evaluate(te)
        print("learner: rmse fp32 %.9g bf16 %.9g, allowed difference %.3g; max_abs_err %.3g" % (fp32_metric, got, bound.max(),
                                                                                                view.info.max_abs_err))
        assert abs(got - fp32_metric) <= bound.max()                            # (rmse and the clamp are 1-Lipschitz in the scores)
        assert np.all(np.abs(view.predict_raw(te) - raw) <= bound)
        want_out = view.predict(te)
        assert np.all(want_out >= l.min_target) and np.all(want_out <= l.max_target)
        assert view.info.bytes_compact == l.fm.num_attribute * (2 * row_stride(k) + 4) and view.info.nonfinite == 0
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
    assert cli.main(argv + ["-out", outs, "-serve", "bf16"]) == 0
    served = capsys.readouterr()
    assert served.out == plain.out and plain.out.count("#Iter=") == iters
    assert "compact" not in plain.err
    extra = served.err[len(plain.err):]
    assert served.err.startswith(plain.err) and extra.count("\n") == 1 and extra.startswith("compact\tformat=bf16\tbytes=")
    fields = dict(f.split("=") for f in extra.strip().split("\t")[1:])
    assert int(fields["bytes"]) == bytes_compact and int(fields["bytes_fp32"]) > bytes_compact
    assert int(fields["nonfinite"]) == 0 and float(fields["max_abs_err"]) > 0
    assert float(fields["Test(fp32)"]) == pytest.approx(fp32_metric, rel=1e-5)
    assert float(fields["Test(bf16)"]) == pytest.approx(got, rel=1e-5)
    p_plain = np.array([float(x) for x in open(outp).read().split()])
    p_serve = np.array([float(x) for x in open(outs).read().split()])
    np.testing.assert_allclose(p_plain, fp32_pred, rtol=1e-5, atol=1e-9)         # (%g keeps 6 digits)
    np.testing.assert_allclose(p_serve, want_out, rtol=1e-5, atol=1e-9)
    assert not np.array_equal(p_serve, p_plain)                                 # (and the two files are not the same numbers)
    # MCMC has no single model to freeze
    assert cli.main(argv + ["-serve", "bf16", "-method", "mcmc"]) == 0
    assert "ERROR: -serve is not supported with -method mcmc" in capsys.readouterr().err


def test_als_learner_view(capi):
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
        view = l.compact()
        raw = l._h.predict(1, te.num_cases)
        bound = (2 * U + U * U) * pair_mass(te.entries, te.row_ptr, np.asarray(l.fm.v).reshape(4, -1)) + RTOL * np.abs(raw) + ATOL
        assert np.all(np.abs(view.predict_raw(te) - raw) <= bound)
        assert abs(view.evaluate(te) - l.evaluate(te)) <= bound.max()
        assert np.array_equal(view.predict(te), np.maximum(l.min_target, np.minimum(l.max_target, view.predict_raw(te))))
        with pytest.raises(ValueError):
            view.predict(L.Data(*tiny_regression(5)))
        view.close()
    finally:
        l.close()
