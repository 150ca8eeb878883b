"""GPU: the field-aware FM (fmx_ffm_*, k_ffm_rows / k_ffm_apply_seg) against its float64 restatement libfm_amd/ffm.py.
Tolerances: tests/test_gpu_adagrad.py's -- w0, w, v and predictions at rtol 1e-4 / atol 2e-5, the accumulators at rtol 1e-4.  The
restatement run in fp32 (numpy) on the training cases below sits at most 2.0e-7 (w0, w, v: absolute), 1.9e-6 (accumulators:
relative) and 2.2e-6 (predictions after training: absolute) from the fp64 one: the tolerances are more than
4x that."""
import numpy as np
import pytest

import fwfm_cases

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
LR, ETA, ROWS = 0.01, 0.05, 203


def open_handle(capi, m, groups, kf, task=0, adagrad=False):
    h = capi.Handle(m.n, m.k, m.k0, m.k1, task, m.reg0, m.regw, m.regv, LR, -1.0, 1.0)
    h.set_params(m.w0, m.w, m.v)
    h.set_groups(groups)
    if adagrad:
        h.adapt_begin("adagrad", 1.0, ETA)
    h.ffm_begin(kf)
    return h


@pytest.mark.parametrize("kf, F", [(1, 1), (4, 2), (4, 5), (8, 8), (5, 17), (3, 33), (4, 39), (4, 64)])
def test_predict(oracle, kf, F):
    """W = 1, several rows per wave-wide load, W no power of two, W = 64, every lane-map width up to 256, a tile beyond 64 KiB"""
    from libfm_amd import capi, ffm
    m, groups, _, d = fwfm_cases.make(oracle, F * kf, F)
    h = open_handle(capi, m, groups, kf)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        got = h.ffm_predict(0, d.n_rows)
        ref = ffm.predict(m, groups, kf, d)
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
        assert abs(h.ffm_evaluate(0).rmse - np.sqrt(np.mean((np.clip(ref, -1, 1) - d.target) ** 2))) < 1e-4
        if F == 1:                                                  # one field is the plain FM: fmx_predict of the same handle
            np.testing.assert_allclose(got, h.predict(0, d.n_rows), rtol=RTOL, atol=ATOL)
    finally:
        h.close()


def state_of(h, n):
    return h.get_params() + h.adapt_state_rows(np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("task", [0, 1])
@pytest.mark.parametrize("batch", [1, 7, 0, ROWS - 1])
@pytest.mark.parametrize("kf, F", [(4, 3), (5, 17), (4, 39)])
def test_training(oracle, kf, F, batch, task):
    from libfm_amd import adaptive, capi, ffm
    m, groups, _, d = fwfm_cases.make(oracle, F * kf, F, task)
    before = m.copy()
    st = adaptive.AdaptState(m.n, m.k, 1.0)
    h = open_handle(capi, m, groups, kf, task, adagrad=True)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        for _ in range(3):
            es = h.ffm_epoch(0, batch, 16)
            ffm.epoch(m, st, groups, kf, d, task, LR, -1.0, 1.0, batch, 16, eta=ETA)
        assert es.rows == ROWS and es.batches == (1 if batch == 0 else -(-ROWS // batch))
        w0, w, v, nw, nv = state_of(h, m.n)
    finally:
        h.close()
    np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=ATOL)
    assert abs(w0 - m.w0) <= RTOL * abs(m.w0) + ATOL
    np.testing.assert_allclose(nv, st.n_v, rtol=RTOL)
    np.testing.assert_allclose(nw, st.n_w, rtol=RTOL)
    assert np.abs(m.v - before.v).max() > 1e-3                     # (moved far beyond the tolerances)


def test_bit_reproducible_untouched_features_and_padding(oracle):
    """... and V's padding columns (W = 85 in rows of 96 floats) stay zero: fmx_predict's sums run over the whole row"""
    from libfm_amd import capi
    m, groups, _, d = fwfm_cases.make(oracle, 85, 17, 1)
    touched = np.zeros(m.n, dtype=bool)
    touched[d.entries["id"]] = True
    res = []
    for _ in range(2):
        h = open_handle(capi, m, groups, 5, 1, adagrad=True)
        try:
            h.upload_rows(0, d.entries, d.row_ptr, d.target)
            start = state_of(h, m.n)
            for _ in range(2):
                h.ffm_epoch(0, 48, 16)
            res.append(state_of(h, m.n))
            plain = h.predict(0, ROWS)
        finally:
            h.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    for i in (1, 3):                                                # w, n_w
        assert np.array_equal(res[0][i][~touched], start[i][~touched]) and not np.array_equal(res[0][i][touched], start[i][touched])
    for i in (2, 4):                                                # v, n_v
        assert np.array_equal(res[0][i][:, ~touched], start[i][:, ~touched])
    after = m.copy()
    after.w0, after.w[:], after.v[:] = res[0][:3]
    np.testing.assert_allclose(plain, oracle.predict_raw(after, d), rtol=RTOL, atol=ATOL)


REFUSALS = ["wrong_num_factor", "no_adagrad", "exclusive", "groups_changed", "weights", "tile_too_large"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(oracle, what):
    """the refusals of include/fmx.h "fmx_ffm_*" that are its own; the handle predicts afterwards"""
    from libfm_amd import capi
    m, groups, _, d = fwfm_cases.make(oracle, 15, 5)
    big = what == "tile_too_large"                                  # 64 fields x 16: rows of 1040 floats, 260 KiB
    h = capi.Handle(m.n, 1024 if big else 15, learn_rate=LR)

    def code(fn, *a):
        with pytest.raises(capi.FmxError) as ei:
            fn(*a)
        return ei.value.code
    try:
        h.set_groups(np.arange(m.n) % 64 if big else groups)
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        if what == "wrong_num_factor":
            assert code(h.ffm_begin, 4) == -1 and code(h.ffm_begin, 0) == -1
        elif big:
            assert code(h.ffm_begin, 16) == -4
        elif what == "exclusive":                                   # an open FwFM session refuses the FFM's, and the reverse
            h.fwfm_begin()
            assert code(h.ffm_begin, 3) == -3
            h.fwfm_end()
            h.ffm_begin(3)
            assert code(h.fwfm_begin) == -3
        else:
            h.ffm_begin(3)
            if what == "no_adagrad":
                assert code(h.ffm_epoch, 0) == -3
            elif what == "groups_changed":
                h.set_groups(np.arange(m.n) % 3)
                assert code(h.ffm_predict, 0, ROWS) == -3
                h.set_groups(groups)
            elif what == "weights":
                h.set_row_weights(0, np.ones(ROWS))
                h.adapt_begin()
                assert code(h.ffm_epoch, 0) == -4
                h.set_row_weights(0, None)
        assert np.isfinite(h.predict(0, ROWS)).all()               # the handle is usable
    finally:
        h.close()


def test_learner_and_cli(oracle, tmp_path):
    """three iterations of `-model ffm` and of the learner with model="ffm" end at the model the restatement, driven the same way, ends at"""
    from libfm_amd import adaptive, cli, ffm, learner as L
    from libfm_amd import refrand as R
    (_, groups, _, d), kf, F = fwfm_cases.make(oracle, 20, 5, 1), 4, 5
    trf, meta, mout = str(tmp_path / "tr.libfm"), str(tmp_path / "meta"), str(tmp_path / "model.txt")
    d.write_libsvm(trf)
    n, reg = d.num_feature, (0.01, 0.002, 0.001)
    np.savetxt(meta, groups[:n], fmt="%d")
    assert cli.main(["-task", "c", "-train", trf, "-test", trf, "-dim", "1,1,%d" % kf, "-iter", "3", "-method", "sgd", "-learn_rate", "0.05",
                     "-regular", "%g,%g,%g" % reg, "-init_stdev", "0.1", "-seed", "42", "-optimizer", "adagrad", "-batch", "64",
                     "-w0_chunk", "16", "-model", "ffm", "-meta", meta, "-save_model", mout]) == 0
    m = oracle.Model(n, F * kf, True, True, *reg)
    R.srand(42)
    m.v[:] = R.init_v(F * kf, n, 0.0, 0.1)
    l = L.FMLearnSGD()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor, (l.fm.reg0, l.fm.regw, l.fm.regv) = n, kf, reg
    l.fm.w0, l.fm.w, l.fm.v = 0.0, np.zeros(n), m.v.copy()
    l.task, l.num_iter, l.learn_rate, l.batch, l.w0_chunk, l.min_target, l.max_target = 1, 3, 0.05, 64, 16, -1.0, 1.0
    l.optimizer, l.model, l.groups, l.out = "adagrad", "ffm", groups[:n], open(str(tmp_path / "log"), "w")
    st = adaptive.AdaptState(n, F * kf, 1.0)
    for _ in range(3):
        ffm.epoch(m, st, groups[:n], kf, d, 1, 0.05, -1.0, 1.0, 64, 16)
    saved = L.FMModel()
    saved.num_attribute, saved.num_factor, saved.v = n, kf, np.zeros((F * kf, n))
    assert saved.load_model(mout)                                   # F kf columns per feature
    np.testing.assert_allclose(saved.v, m.v, rtol=1e-5, atol=ATOL)  # (the file holds 6 significant digits)
    data = L.Data(d.entries, d.row_ptr, d.target)
    try:
        l.init()
        l.learn(data, data)
        np.testing.assert_allclose(l.fm.v, m.v, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(l.predict_raw(data), ffm.predict(m, groups[:n], kf, d), rtol=RTOL, atol=ATOL)
    finally:
        l.close()
