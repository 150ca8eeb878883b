"""GPU: the field-weighted FM (fmx_fwfm_*, k_fwfm_rows / k_fwfm_apply_seg / k_fwfm_rgrad / k_fwfm_rstep) against its float64
restatement libfm_amd/fwfm.py (itself pinned to a brute-force double loop and to finite differences in tests/test_fwfm_cpu.py).

Tolerances: tests/test_gpu_adagrad.py's -- w0, w, v, r and predictions at rtol 1e-4 / atol 2e-5, the accumulators at rtol 1e-4.  The
restatement run in fp32 (numpy) on the training cases below sits at most 4.6e-7 (w0, w, v, r: absolute) and 2.1e-5 (accumulators:
relative) from the fp64 one: the tolerances are more than 4x that."""
import numpy as np
import pytest

import fwfm_cases

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
LR, ETA = 0.01, 0.05
ROWS = 203
CHUNK = 64                                                        # FWFM_RCHUNK of k_fwfm_rgrad


def open_handle(capi, m, groups, task=0, r=None, adagrad=False):
    h = capi.Handle(m.n, m.k, m.k0, m.k1, task, m.reg0, m.regw, m.regv, LR, -1.0, 1.0)
    h.set_params(m.w0, m.w, m.v)
    h.set_groups(groups)
    if adagrad:
        h.adapt_begin("adagrad", 1.0, ETA)
    h.fwfm_begin()
    if r is not None:
        h.fwfm_set_r(r)
    return h


@pytest.mark.parametrize("F", [1, 2, 5, 17, 33, 64])
@pytest.mark.parametrize("k", [1, 8, 20, 64, 128])
def test_predict(oracle, k, F):
    """the padding and tile boundaries of the MFMA shapes; fwfm_cases' rows reach the kernel's edges; 203 rows = 50 blocks of 4 + 3"""
    from libfm_amd import capi, fwfm
    m, groups, r, d = fwfm_cases.make(oracle, k, F)
    h = open_handle(capi, m, groups, r=r)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        got = h.fwfm_predict(0, d.n_rows)
        ref = fwfm.predict(m, r, groups, d)
        print("k %d F %d: largest gap %.3g" % (k, F, np.abs(got - ref).max()))
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
        assert abs(h.fwfm_evaluate(0).rmse - np.sqrt(np.mean((np.clip(ref, -1, 1) - d.target) ** 2))) < 1e-4
        h.fwfm_set_r(np.ones((F, F)))                               # r == 1 is the plain FM: fmx_predict of the same handle
        np.testing.assert_allclose(h.fwfm_predict(0, d.n_rows), h.predict(0, d.n_rows), rtol=RTOL, atol=ATOL)
    finally:
        h.close()


def state_of(h, n):
    return h.get_params() + h.adapt_state_rows(np.arange(n, dtype=np.uint32)) + h.fwfm_get_r()


@pytest.mark.parametrize("task", [0, 1])
@pytest.mark.parametrize("batch", [1, 7, 0, ROWS - 1, CHUNK - 1, CHUNK, CHUNK + 1])
@pytest.mark.parametrize("k, F", [(8, 3), (20, 17), (64, 33)])
def test_training(oracle, k, F, batch, task):
    from libfm_amd import adaptive, capi, fwfm
    m, groups, r, d = fwfm_cases.make(oracle, k, F, task)
    assert d.n_rows == ROWS
    before, r0 = m.copy(), r.copy()
    st, nr = adaptive.AdaptState(m.n, k, 1.0), np.ones((F, F))
    h = open_handle(capi, m, groups, task, r, adagrad=True)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        for _ in range(3):
            es = h.fwfm_epoch(0, batch, 16)
            fwfm.epoch(m, st, r, nr, groups, d, task, LR, -1.0, 1.0, batch, 16, eta=ETA)
        assert es.rows == ROWS and es.batches == (1 if batch == 0 else -(-ROWS // batch))
        w0, w, v, nw, nv, gr, gnr = state_of(h, m.n)
    finally:
        h.close()
    print("gaps: v %.3g w %.3g w0 %.3g r %.3g" % (np.abs(v - m.v).max(), np.abs(w - m.w).max(), abs(w0 - m.w0), np.abs(gr - r).max()))
    np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=ATOL)
    assert abs(w0 - m.w0) <= RTOL * abs(m.w0) + ATOL
    np.testing.assert_allclose(gr, r, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(nv, st.n_v, rtol=RTOL)
    np.testing.assert_allclose(nw, st.n_w, rtol=RTOL)
    np.testing.assert_allclose(gnr, nr, rtol=RTOL)
    assert np.array_equal(gr, gr.T) and np.array_equal(gnr, gnr.T)              # exactly symmetric
    assert np.abs(m.v - before.v).max() > 1e-3 and np.abs(r - r0).max() > 1e-3  # (moved far beyond the tolerances)


def test_bit_reproducible_and_untouched_features(oracle):
    from libfm_amd import capi
    m, groups, r, d = fwfm_cases.make(oracle, 64, 33, 1)
    touched = np.zeros(m.n, dtype=bool)
    touched[d.entries["id"]] = True
    res = []
    for _ in range(2):
        h = open_handle(capi, m, groups, 1, r, adagrad=True)
        try:
            h.upload_rows(0, d.entries, d.row_ptr, d.target)
            start = state_of(h, m.n)
            for _ in range(2):
                h.fwfm_epoch(0, 48, 16)
            res.append(state_of(h, m.n))
        finally:
            h.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    for i in (1, 3):                                                # w, n_w
        assert np.array_equal(res[0][i][~touched], start[i][~touched]) and not np.array_equal(res[0][i][touched], start[i][touched])
    for i in (2, 4):                                                # v, n_v
        assert np.array_equal(res[0][i][:, ~touched], start[i][:, ~touched])


def test_learner_and_cli(oracle, tmp_path):
    """three iterations of `-model fwfm` and of the learner with model="fwfm" end at the matrix the restatement, driven the same way, ends at"""
    from libfm_amd import adaptive, cli, fwfm, learner as L
    from libfm_amd import refrand as R
    (_, groups, _, d), k, F = fwfm_cases.make(oracle, 8, 5, 1), 8, 5
    trf, meta, rout = str(tmp_path / "tr.libfm"), str(tmp_path / "meta"), str(tmp_path / "r.txt")
    d.write_libsvm(trf)
    n, reg = d.num_feature, (0.01, 0.002, 0.001)
    np.savetxt(meta, groups[:n], fmt="%d")
    assert cli.main(["-task", "c", "-train", trf, "-test", trf, "-dim", "1,1,%d" % k, "-iter", "3", "-method", "sgd", "-learn_rate", "0.05",
                     "-regular", "%g,%g,%g" % reg, "-init_stdev", "0.1", "-seed", "42", "-optimizer", "adagrad", "-batch", "64",
                     "-w0_chunk", "16", "-model", "fwfm", "-meta", meta, "-r_out", rout]) == 0
    m = oracle.Model(n, k, True, True, *reg)
    R.srand(42)
    m.v[:] = R.init_v(k, n, 0.0, 0.1)
    l = L.FMLearnSGD()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor, (l.fm.reg0, l.fm.regw, l.fm.regv) = n, k, reg
    l.fm.w0, l.fm.w, l.fm.v = 0.0, np.zeros(n), m.v.copy()
    l.task, l.num_iter, l.learn_rate, l.batch, l.w0_chunk, l.min_target, l.max_target = 1, 3, 0.05, 64, 16, -1.0, 1.0
    l.optimizer, l.model, l.groups, l.out = "adagrad", "fwfm", groups[:n], open(str(tmp_path / "log"), "w")
    st, r, nr = adaptive.AdaptState(n, k, 1.0), np.ones((F, F)), np.ones((F, F))
    for _ in range(3):
        fwfm.epoch(m, st, r, nr, groups[:n], d, 1, 0.05, -1.0, 1.0, 64, 16)
    np.testing.assert_allclose(np.loadtxt(rout), r, rtol=RTOL, atol=ATOL)      # (the file holds 6 significant digits)
    data = L.Data(d.entries, d.row_ptr, d.target)
    try:
        l.init()
        l.learn(data, data)
        np.testing.assert_allclose(l.r, r, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(l.predict_raw(data), fwfm.predict(m, r, groups[:n], d), rtol=RTOL, atol=ATOL)
        with pytest.raises(NotImplementedError):
            l.evaluate_ex(data)
    finally:
        l.close()


REFUSALS = ["no_session", "no_adagrad", "null_opts", "flags", "bad_option", "bad_r", "groups_changed", "slot_unused", "slot_no_target",
            "sgda", "als", "shard", "comm", "blocks", "weights", "too_many_fields", "too_many_factors"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(oracle, what):
    """every refusal of include/fmx.h "fmx_fwfm_*"; the handle predicts afterwards"""
    import ctypes as C
    import datagen
    from libfm_amd import capi
    m, groups, r, d = fwfm_cases.make(oracle, 8, 5)
    kw = {"shard": dict(shard_rank=0, shard_world=2)}.get(what, {})
    k = 256 if what == "too_many_factors" else 8
    h = capi.Handle(m.n, k, learn_rate=LR, **kw)

    def code(fn, *a):
        with pytest.raises(capi.FmxError) as ei:
            fn(*a)
        return ei.value.code
    try:
        if what in ("shard", "too_many_factors"):
            assert code(h.fwfm_begin) == -4
            return
        if what == "comm":
            h.comm_init_rank(capi.comm_unique_id(), 0, 1)
            assert code(h.fwfm_begin) == -4
            return
        h.set_groups(np.arange(m.n) % 65 if what == "too_many_fields" else groups)
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        h.upload_rows(1, d.entries, d.row_ptr, None)
        if what == "too_many_fields":
            assert code(h.fwfm_begin) == -4
        elif what == "no_session":
            assert [code(f, *a) for f, a in ((h.fwfm_epoch, (0,)), (h.fwfm_predict, (0, ROWS)), (h.fwfm_evaluate, (0,)), (h.fwfm_get_r, ()),
                                             (h.fwfm_set_r, (r,)), (h.fwfm_end, ()))] == [-3] * 6
        elif what == "null_opts":
            assert h.lib.fmx_fwfm_begin(h.h, None) == -1
        elif what == "flags":
            assert h.lib.fmx_fwfm_begin(h.h, C.byref(capi.FwfmOpts(1, 0, 0.0, 0.0, 0.0))) == -1
        elif what == "bad_option":
            for bad in (-1.0, float("nan"), float("inf")):
                for i in range(3):
                    o = [0.0, 0.0, 0.0]
                    o[i] = bad
                    assert h.lib.fmx_fwfm_begin(h.h, C.byref(capi.FwfmOpts(0, 0, *o))) == -1
        elif what == "sgda":
            h.sgda_begin()
            assert code(h.fwfm_begin) == -3
            h.sgda_end()
        elif what == "als":
            h.als_begin(0)
            assert code(h.fwfm_begin) == -3
            h.als_end()
        else:
            h.fwfm_begin()
            if what == "no_adagrad":
                assert code(h.fwfm_epoch, 0) == -3
            elif what == "bad_r":
                bad = r.copy()
                bad[0, 1] += 1.0
                assert code(h.fwfm_set_r, bad) == -1
                bad = r.copy()
                bad[2, 2] = float("nan")
                assert code(h.fwfm_set_r, bad) == -1
                assert h.lib.fmx_fwfm_set_r(h.h, None) == -1 and h.lib.fmx_fwfm_get_r(h.h, None, None) == -1
                assert h.lib.fmx_fwfm_predict(h.h, 0, None) == -1 and h.lib.fmx_fwfm_evaluate(h.h, 0, None) == -1
            elif what == "groups_changed":
                h.set_groups(np.arange(m.n) % 7)
                assert code(h.fwfm_predict, 0, ROWS) == -3
                h.set_groups(groups)
            elif what == "slot_unused":
                h.adapt_begin()
                assert code(h.fwfm_epoch, 5) == -3 and code(h.fwfm_evaluate, 5) == -3 and code(h.fwfm_predict, 5, ROWS) == -3
            elif what == "slot_no_target":
                h.adapt_begin()
                assert code(h.fwfm_epoch, 1) == -3 and code(h.fwfm_evaluate, 1) == -3
            elif what == "blocks":
                be, br, _ = datagen.ragged_real(20, 4, 3, seed=62)
                h.upload_block_rows(4, d.entries, d.row_ptr, d.target, [(be, br, np.arange(ROWS) % 4, 580)], keep=True)
                h.adapt_begin()
                assert code(h.fwfm_epoch, 4) == -4 and code(h.fwfm_predict, 4, ROWS) == -4
            elif what == "weights":
                h.set_row_weights(0, np.ones(ROWS))
                h.adapt_begin()
                assert code(h.fwfm_epoch, 0) == -4
                h.set_row_weights(0, None)
        assert np.isfinite(h.predict(0, ROWS)).all()               # the handle is usable
        if what != "too_many_fields":
            h.fwfm_begin()
            assert np.isfinite(h.fwfm_predict(0, ROWS)).all()
    finally:
        h.close()
