"""GPU: the third-order FM (fmx_hofm_*, k_hofm_rows / k_hofm_apply_seg) against its float64 restatement libfm_amd/hofm.py.
Tolerances: tests/test_gpu_adagrad.py's -- w0, w, v, predictions: rtol 1e-4 / atol 2e-5; accumulators: rtol 1e-4."""
import numpy as np
import pytest

import hofm_cases

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
LR, ETA, ROWS_T = 0.01, 0.05, 503


def open_handle(capi, m, k3, task=0, adagrad=False):
    h = capi.Handle(m.n, m.k, m.k0, m.k1, task, m.reg0, m.regw, m.regv, LR, -1.0, 1.0)
    h.set_params(m.w0, m.w, m.v)
    if adagrad:
        h.adapt_begin("adagrad", 1.0, ETA)
    if k3 is not None:
        h.hofm_begin(k3)
    return h


def state_of(h, n):
    return h.get_params() + h.adapt_state_rows(np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("k2, k3", [(0, 1), (4, 4), (3, 5), (16, 16), (17, 47), (64, 64), (0, 1024)])
def test_predict(oracle, k2, k3):
    """one column, several rows per wave-wide load, a row off the 16-float padding, lanes of 1, 2 and 16 floats, the widest row, no pair part"""
    from libfm_amd import capi, hofm
    m, d = hofm_cases.make(oracle, k2, k3)
    h = open_handle(capi, m, k3)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        ref = hofm.predict(m, k3, d)
        np.testing.assert_allclose(h.hofm_predict(0, d.n_rows), ref, rtol=RTOL, atol=ATOL)
        assert abs(h.hofm_evaluate(0).rmse - np.sqrt(np.mean((np.clip(ref, -1, 1) - d.target) ** 2))) < 1e-4
    finally:
        h.close()


@pytest.mark.parametrize("task", [0, 1])
@pytest.mark.parametrize("batch", [1, 7, 0, 202])
@pytest.mark.parametrize("k2, k3", [(4, 4), (3, 5), (17, 47)])
def test_training(oracle, k2, k3, batch, task):
    """batch 202 of 503 rows: a feature's segment holds several occurrences with different values"""
    from libfm_amd import adaptive, capi, hofm
    m, d = hofm_cases.make(oracle, k2, k3, task, ROWS_T)
    before = m.copy()
    st = adaptive.AdaptState(m.n, m.k, 1.0)
    h = open_handle(capi, m, k3, task, adagrad=True)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        for _ in range(3):
            es = h.hofm_epoch(0, batch, 16)
            hofm.epoch(m, st, k3, d, task, LR, -1.0, 1.0, batch, 16, eta=ETA)
        assert es.rows == ROWS_T and es.batches == (1 if batch == 0 else -(-ROWS_T // batch))
        w0, w, v, nw, nv = state_of(h, m.n)
        pred = h.hofm_predict(0, ROWS_T)
    finally:
        h.close()
    for got, ref, atol in ((v, m.v, ATOL), (w, m.w, ATOL), (w0, m.w0, ATOL), (pred, hofm.predict(m, k3, d), ATOL), (nv, st.n_v, 0), (nw, st.n_w, 0)):
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=atol)
    assert np.abs(m.v - before.v)[k2:].max() > 1e-3                # (the third-order factors moved far beyond the tolerances)


@pytest.mark.parametrize("k2, k3, first", [(31, 54, "hofm"), (20, 0, "adapt"), (85, 0, "adapt")])
def test_identical_bits_untouched_features_and_padding(oracle, k2, k3, first):
    """two runs, the first of them fmx_adapt_epoch where k3 = 0; V's padding (rows of 96 and 32 floats) stays zero: fmx_predict sums over it"""
    from libfm_amd import capi
    m, d = hofm_cases.make(oracle, k2, k3, 1, ROWS_T)
    touched = np.isin(np.arange(m.n), d.entries["id"])
    res = []
    for which in (first, "hofm"):
        h = open_handle(capi, m, k3 if which == "hofm" else None, 1, adagrad=True)
        try:
            h.upload_rows(0, d.entries, d.row_ptr, d.target)
            start = state_of(h, m.n)
            for _ in range(2):
                (h.hofm_epoch if which == "hofm" else h.adapt_epoch)(0, 202, 16)
            res.append(state_of(h, m.n))
            plain = h.predict(0, d.n_rows)
        finally:
            h.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    w0, w, v, nw, nv = res[0]
    assert not touched.all() and not np.array_equal(v[:, touched], start[2][:, touched])
    for got, was in ((w, start[1]), (nw, start[3]), (v.T, start[2].T), (nv.T, start[4].T)):
        assert np.array_equal(got[~touched], was[~touched])
    after = m.copy()
    after.w0, after.w[:], after.v[:] = w0, w, v
    np.testing.assert_allclose(plain, oracle.predict_raw(after, d), rtol=RTOL, atol=ATOL)


BEGIN, OPEN = ["h.hofm_begin(3)"], "h.hofm_begin(3); "
REFUSALS = {
    "too_many": ("", ["h.hofm_begin(9)", "h.lib.fmx_hofm_begin(h.h, None)", "h.lib.fmx_hofm_begin(h.h, C.byref(capi.HofmOpts(3, 1)))"], -1, ""),
    "no_adagrad": (OPEN, ["h.hofm_epoch(0)"], -3, ""),
    **{s + "_open": ("h.%s_begin(%s)" % (s, a), BEGIN, -3, "h.%s_end()" % s) for s, a in (("sgda", ""), ("als", "0"), ("fwfm", ""), ("ffm", "8"), ("fmfm", ""))},
    "hofm_open": (OPEN, ["h.fwfm_begin()", "h.ffm_begin(8)", "h.fmfm_begin()"], -3, ""),
    "shard": ("", BEGIN, -4, ""),
    "comm": ("h.comm_init_rank(capi.comm_unique_id(), 0, 1)", BEGIN, -4, ""),
    "blocks": (OPEN + "h.upload_block_rows(4, d.entries, d.row_ptr, d.target, [datagen.ragged_real(20, 4, 3, seed=62)[:2] + "
                      "(np.arange(ROWS) % 4, 680)], keep=True); h.adapt_begin()", ["h.hofm_epoch(4)", "h.hofm_predict(4, ROWS)"], -4, ""),
    "weights": (OPEN + "h.set_row_weights(0, np.ones(ROWS)); h.adapt_begin()", ["h.hofm_epoch(0)"], -4, "h.set_row_weights(0, None)"),
}


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(oracle, what):
    """every refusal of include/fmx.h "fmx_hofm_*", once: (set-up, the refused calls, their code, what undoes the set-up); the handle predicts afterwards"""
    import ctypes as C
    import datagen
    from libfm_amd import capi
    setup, calls, code, undo = REFUSALS[what]
    _, d = hofm_cases.make(oracle, 5, 3)
    h = capi.Handle(hofm_cases.N, 8, learn_rate=LR, **(dict(shard_rank=0, shard_world=2) if what == "shard" else {}))
    scope = dict(h=h, d=d, C=C, capi=capi, np=np, datagen=datagen, ROWS=d.n_rows)
    try:
        if what not in ("shard", "comm"):
            h.upload_rows(0, d.entries, d.row_ptr, d.target)
        exec(setup, scope)
        for call in calls:
            try:
                got = eval(call, scope)
                got = got if isinstance(got, int) else 0
            except capi.FmxError as e:
                got = e.code
            assert got == code, call
        exec(undo, scope)
        assert what in ("shard", "comm") or np.isfinite(h.predict(0, d.n_rows)).all()       # the handle is usable
    finally:
        h.close()


def test_learner_and_cli(oracle, tmp_path):
    """three iterations of `-model hofm -dim 1,1,4,3` and of the learner end at the restatement's model; -save_model carries k2 + k3 columns"""
    from libfm_amd import adaptive, cli, hofm, learner as L, refrand as R
    (_, d), k2, k3, reg = hofm_cases.make(oracle, 4, 3, 1), 4, 3, (0.01, 0.002, 0.001)
    trf, mout, n = str(tmp_path / "tr.libfm"), str(tmp_path / "model.txt"), d.num_feature
    d.write_libsvm(trf)
    assert cli.main(["-task", "c", "-train", trf, "-test", trf, "-dim", "1,1,%d,%d" % (k2, k3), "-iter", "3", "-method", "sgd", "-learn_rate", "0.05",
                     "-regular", "%g,%g,%g" % reg, "-init_stdev", "0.1", "-seed", "42", "-optimizer", "adagrad", "-batch", "64",
                     "-w0_chunk", "16", "-model", "hofm", "-save_model", mout]) == 0
    m = oracle.Model(n, k2 + k3, True, True, *reg)
    R.srand(42)
    m.v[:] = R.init_v(k2 + k3, n, 0.0, 0.1)
    l, saved = L.FMLearnSGD(), L.FMModel()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor, (l.fm.reg0, l.fm.regw, l.fm.regv) = n, k2, reg
    l.fm.w0, l.fm.w, l.fm.v = 0.0, np.zeros(n), m.v.copy()
    l.task, l.num_iter, l.learn_rate, l.batch, l.w0_chunk, l.min_target, l.max_target = 1, 3, 0.05, 64, 16, -1.0, 1.0
    l.optimizer, l.model, l.num_factor3, l.out = "adagrad", "hofm", k3, open(str(tmp_path / "log"), "w")
    st = adaptive.AdaptState(n, k2 + k3, 1.0)
    for _ in range(3):
        hofm.epoch(m, st, k3, d, 1, 0.05, -1.0, 1.0, 64, 16)
    saved.num_attribute, saved.num_factor, saved.v = n, k2, np.zeros((k2 + k3, n))
    assert saved.load_model(mout)
    np.testing.assert_allclose(saved.v, m.v, rtol=1e-5, atol=ATOL)  # (the file holds 6 significant digits)
    data = L.Data(d.entries, d.row_ptr, d.target)
    try:
        l.init()
        l.learn(data, data)
        np.testing.assert_allclose(l.predict_raw(data), hofm.predict(m, k3, d), rtol=RTOL, atol=ATOL)
    finally:
        l.close()
