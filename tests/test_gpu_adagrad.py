"""GPU: AdaGrad on the minibatch rule (fmx_adapt_*, k_adapt_apply_seg) against its float64 restatement libfm_amd/adaptive.py (itself
pinned to the oracle's batch rule and to hand-worked literals in tests/test_adagrad_cpu.py).

Tolerances: w0, w, v at rtol 1e-4 / atol 2e-5 (the SGDA batch form's, tests/test_gpu_sgda.py), the accumulators at rtol 1e-4.  They hold
because d(step)/dg <= eta / sqrt(init_acc): a gradient error is amplified no more than under plain SGD; the restatement run in fp32
sits 5e-7 (accumulators) and 5e-8 (parameters) from the fp64 one at the parity shape, 1.4e-6 on the long segments."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import datagen
from test_adagrad_cpu import hot_case

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
N, ROWS, NNZ = 6400, 512, 32
LR, ETA = 0.01, 0.05


def start_model(O, n, k, k0=True, k1=True, reg=(0.01, 0.002, 0.001)):
    m = O.Model(n, k, k0, k1, *reg)
    m.v[:] = O.init_values(1, n, k, 0.05)
    if k1:
        m.w[:] = O.init_values(2, n, 1, 0.02)[0]
    m.w0 = 0.03 if k0 else 0.0
    return m


def handle_for(capi, m, task, lr, lo=-1.0, hi=1.0, **kw):
    h = capi.Handle(m.n, m.k, m.k0, m.k1, task, m.reg0, m.regw, m.regv, lr, lo, hi, **kw)
    h.set_params(m.w0, m.w, m.v)
    return h


def check_against(h, m, st):
    """parameters and every accumulator of the handle against the restatement's"""
    w0, w, v = h.get_params()
    nw, nv = h.adapt_state_rows(np.arange(m.n, dtype=np.uint32))
    gaps = [float(np.abs(v - m.v).max()) if m.k else 0.0, float(np.abs(w - m.w).max()), abs(w0 - m.w0),
            float((np.abs(nv - st.n_v) / st.n_v).max()) if m.k else 0.0, float((np.abs(nw - st.n_w) / st.n_w).max())]
    print("gaps: v %.3g  w %.3g  w0 %.3g  n_v (rel) %.3g  n_w (rel) %.3g" % tuple(gaps))
    np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=ATOL)
    assert abs(w0 - m.w0) <= RTOL * abs(m.w0) + ATOL
    np.testing.assert_allclose(nv, st.n_v, rtol=RTOL)
    np.testing.assert_allclose(nw, st.n_w, rtol=RTOL)


def run_parity(oracle, k, task, k0=True, k1=True):
    from libfm_amd import adaptive, capi
    d = oracle.synth_rows(7, 0, ROWS, NNZ, N)
    m = start_model(oracle, N, k, k0, k1)
    before = m.copy()
    st = adaptive.AdaptState(N, k, 1.0)
    h = handle_for(capi, m, task, LR)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        h.adapt_begin("adagrad", 1.0, ETA)
        for _ in range(3):
            es = h.adapt_epoch(0, 64, 16)
            adaptive.epoch(m, d, task, LR, -1.0, 1.0, 64, 16, st, eta=ETA)
        assert es.rows == ROWS and es.batches == 8 and es.batch_used == 64 and es.w0_chunk_used == 16
        assert es.main_kernel_launches == 8 and es.device_seconds > 0 and es.max_feature_count >= 1
        check_against(h, m, st)
    finally:
        h.close()
    if k:
        assert np.abs(m.v - before.v).max() > 1e-3               # (three epochs moved the parameters far beyond the tolerances)
    if not k1:
        assert np.all(m.w == before.w) and np.all(st.n_w == 1.0)


# every width the owner kernel is instantiated for: six of them under both tasks, the other six once (regression 2, 16, 512; classification 4, 32, 1024)
PARITY_WIDTHS = [(k, task) for k in (1, 8, 64, 100, 128, 256) for task in (0, 1)] + [(2, 0), (16, 0), (512, 0), (4, 1), (32, 1), (1024, 1)]


@pytest.mark.parametrize("k, task", PARITY_WIDTHS)
def test_parity(oracle, k, task):
    """several rows per wave-wide load (k 1, 8), VEC 1, 2 and 4 (k 64, 128, 256), a row shorter than KP (k 100: 112 floats under KP 128);
    the remaining widths once each (k 2, 4, 16, 32; VEC 8 and 16 with fewer segment groups per round: k 512, 1024)"""
    run_parity(oracle, k, task)


def test_parity_without_linear_weights(oracle):
    run_parity(oracle, 8, 1, k1=False)


def test_parity_without_bias(oracle):
    run_parity(oracle, 8, 0, k0=False)


@pytest.mark.parametrize("k", [64, 8])
def test_long_segments(oracle, k):
    """the hot-feature case: id 0 in every row (one segment of 512 occurrences: the tail loop past 64) and a tail batch of 88 rows"""
    from libfm_amd import adaptive, capi
    d, m8 = hot_case()
    m = oracle.Model(m8.n, k, True, True, 0.0, 0.002, 0.001)
    m.v[:] = oracle.init_values(1, m.n, k, 0.05)
    st = adaptive.AdaptState(m.n, k, 1.0)
    h = handle_for(capi, m, 0, 0.05)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        h.adapt_begin("adagrad", 1.0, 0.05)
        for _ in range(3):
            es = h.adapt_epoch(0, 512, 8)
            adaptive.epoch(m, d, 0, 0.05, -1.0, 1.0, 512, 8, st, eta=0.05)
        assert es.batches == 2 and es.max_feature_count == 512
        check_against(h, m, st)
    finally:
        h.close()


def test_bit_reproducible(oracle):
    from libfm_amd import capi
    d = oracle.synth_rows(7, 0, ROWS, NNZ, N)
    m = start_model(oracle, N, 64)
    res = []
    for _ in range(2):
        h = handle_for(capi, m, 1, LR)
        try:
            h.upload_rows(0, d.entries, d.row_ptr, d.target)
            h.adapt_begin("adagrad", 0.5, ETA)
            for _ in range(2):
                h.adapt_epoch(0, 64, 16)
            res.append(h.get_params() + h.adapt_state_rows(np.arange(N, dtype=np.uint32)))
        finally:
            h.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_state(oracle):
    from libfm_amd import adaptive, capi
    k = 8
    d = oracle.synth_rows(7, 0, ROWS, NNZ, N)
    m = start_model(oracle, N, k)
    ids = np.arange(N, dtype=np.uint32)
    touched = np.zeros(N, dtype=bool)
    touched[d.entries["id"]] = True
    assert touched.any() and not touched.all()
    h = handle_for(capi, m, 1, LR)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        _, w_before, v_before = h.get_params()                   # (as the device holds them: fp32)
        h.adapt_begin("adagrad", 0.25, ETA)
        nw, nv = h.adapt_state_rows(ids)
        assert np.all(nw == 0.25) and np.all(nv == 0.25)
        es = h.adapt_epoch(0)                                     # batch 0 / micro-chunk 0: the library's choices
        assert es.batch_used >= 32 and es.w0_chunk_used == capi.default_w0_chunk(LR, 1) and es.rows == ROWS
        _, w, v = h.get_params()
        nw, nv = h.adapt_state_rows(ids)
        # untouched features: bit-unchanged, accumulators == init_acc; touched ones moved
        assert np.array_equal(w[~touched], w_before[~touched]) and np.array_equal(v[:, ~touched], v_before[:, ~touched])
        assert np.all(nw[~touched] == 0.25) and np.all(nv[:, ~touched] == 0.25)
        # (fp32: a gradient sum below 1e-4 leaves an accumulator of 0.25 where it is, so "moved" is a statement about nearly all of them)
        assert np.all(nw[touched] >= 0.25) and (nw[touched] > 0.25).mean() > 0.99 and (w[touched] != w_before[touched]).mean() > 0.99
        # a subset of rows, in the caller's order
        sub = np.array([5, 0, 6399, 17], dtype=np.uint32)
        snw, snv = h.adapt_state_rows(sub)
        assert np.array_equal(snw, nw[sub]) and np.array_equal(snv, nv[:, sub])
        # fmx_sgd_epoch and fmx_set_params inside a session leave the accumulators alone
        h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, 64, 16)
        h.set_params(m.w0, m.w, m.v)
        nw2, nv2 = h.adapt_state_rows(ids)
        assert np.array_equal(nw2, nw) and np.array_equal(nv2, nv)
        # begin again resets (and nothing in the model changes)
        p0 = h.get_params()
        h.adapt_begin("adagrad", 2.0, ETA)
        nw, nv = h.adapt_state_rows(ids)
        assert np.all(nw == 2.0) and np.all(nv == 2.0)
        for a, b in zip(p0, h.get_params()):
            assert np.array_equal(a, b)
        # init_acc 0 = 1.0, learn_rate 0 = the handle's: one epoch equals the restatement's with those values
        h.adapt_begin()
        ref, st = m.copy(), adaptive.AdaptState(N, k, 1.0)
        h.adapt_epoch(0, 64, 16)
        adaptive.epoch(ref, d, 1, LR, -1.0, 1.0, 64, 16, st, eta=LR)
        check_against(h, ref, st)
        # an empty slot
        h.upload_rows(1, np.zeros(0, dtype=capi.ENTRY_DTYPE), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.float32))
        es = h.adapt_epoch(1, 64, 16)
        assert es.rows == 0 and es.batches == 0
        h.adapt_end()
        h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, 64, 16)     # the handle trains on without a session
    finally:
        h.close()


def test_refusals(oracle):
    from libfm_amd import capi
    k = 8
    d = oracle.synth_rows(7, 0, 64, 8, 100)
    m = start_model(oracle, 100, k)
    h = handle_for(capi, m, 0, LR)

    def code(fn, *a, **kw):
        with pytest.raises(capi.FmxError) as ei:
            fn(*a, **kw)
        return ei.value.code

    def begin_raw(opts):
        return h.lib.fmx_adapt_begin(h.h, C.byref(opts) if opts is not None else None)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        h.upload_rows(1, d.entries, d.row_ptr, None)              # no targets
        ids = np.arange(4, dtype=np.uint32)
        # without a session
        assert code(h.adapt_epoch, 0, 16, 4) == -3 and code(h.adapt_state_rows, ids) == -3 and code(h.adapt_end) == -3
        # FMX_E_ARG of begin
        assert begin_raw(None) == -1
        assert begin_raw(capi.AdaptOpts(2, 0, 0.0, 0.0)) == -1 and begin_raw(capi.AdaptOpts(0, 0, 0.0, 0.0)) == -1
        assert begin_raw(capi.AdaptOpts(1, 1, 0.0, 0.0)) == -1
        for bad in (-1.0, float("nan"), float("inf")):
            assert begin_raw(capi.AdaptOpts(1, 0, bad, 0.0)) == -1
        for bad in (-0.01, float("nan")):
            assert begin_raw(capi.AdaptOpts(1, 0, 0.0, bad)) == -1
        assert code(h.adapt_epoch, 0, 16, 4) == -3                # (none of them opened a session)
        # an open SGDA session, both ways round
        h.sgda_begin()
        assert code(h.adapt_begin) == -3
        h.sgda_end()
        h.set_params(m.w0, m.w, m.v)                              # (fmx_sgda_begin zeroed w)
        h.adapt_begin("adagrad", 1.0, ETA)
        assert code(h.sgda_begin) == -3
        # slots
        assert code(h.adapt_epoch, 5, 16, 4) == -3                # never uploaded
        assert code(h.adapt_epoch, 1, 16, 4) == -3                # without targets
        # outputs and ids of _get_state_rows
        nw, nv = np.zeros(4), np.zeros((4, k))
        assert h.lib.fmx_adapt_get_state_rows(h.h, ids.ctypes.data, 4, None, nv.ctypes.data) == -1
        assert h.lib.fmx_adapt_get_state_rows(h.h, ids.ctypes.data, 4, nw.ctypes.data, None) == -1
        assert h.lib.fmx_adapt_get_state_rows(h.h, None, 4, nw.ctypes.data, nv.ctypes.data) == -1
        assert code(h.adapt_state_rows, np.array([3, 100], dtype=np.uint32)) == -1
        # an open ALS / MCMC session on the slot
        h.als_begin(0)
        assert code(h.adapt_epoch, 0, 16, 4) == -3
        h.als_end()
        # kept `-relation` blocks
        be, br, _ = datagen.ragged_real(20, 4, 3, seed=62)
        h.upload_block_rows(4, d.entries, d.row_ptr, d.target, [(be, br, np.arange(64) % 4, 80)], keep=True)
        with pytest.raises(capi.FmxError) as ei:
            h.adapt_epoch(4, 16, 4)
        assert ei.value.code == -4 and "relations are not supported with SGD" in ei.value.text
        # the handle and the session work afterwards
        es = h.adapt_epoch(0, 16, 4)
        assert es.rows == 64 and es.batches == 4
        h.adapt_end()
    finally:
        h.close()
    # a feature shard, a communicator rank
    hs = capi.Handle(100, k, shard_rank=0, shard_world=2, learn_rate=LR)
    try:
        with pytest.raises(capi.FmxError) as ei:
            hs.adapt_begin()
        assert ei.value.code == -4
    finally:
        hs.close()
    hc = capi.Handle(100, k, learn_rate=LR)
    try:
        hc.comm_init_rank(capi.comm_unique_id(), 0, 1)
        with pytest.raises(capi.FmxError) as ei:
            hc.adapt_begin()
        assert ei.value.code == -4
    finally:
        hc.close()


def test_epoch_invalidates_a_kept_weight_side_stream(oracle):
    """a fused epoch with FMX_FLAG_KEEP_WSIDE leaves the slot's weight side stream valid; an AdaGrad epoch changes the linear weights, so
    fmx_evaluate afterwards must not read it: it equals fmx_evaluate on a fresh handle given the same parameters"""
    from libfm_amd import capi
    d = oracle.synth_rows(7, 0, ROWS, NNZ, N)
    m = start_model(oracle, N, 8)
    h = handle_for(capi, m, 0, LR)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_FUSED, 64, 16, capi.FLAG_KEEP_WSIDE, 2)
        assert h.evaluate(0).flags & capi.EVAL_WSIDE             # (the stream is there and current)
        h.adapt_begin("adagrad", 1.0, ETA)
        h.adapt_epoch(0, 64, 16)
        ev = h.evaluate(0)
        assert not (ev.flags & capi.EVAL_WSIDE)
        w0, w, v = h.get_params()
    finally:
        h.close()
    f = capi.Handle(N, 8, True, True, 0, m.reg0, m.regw, m.regv, LR, -1.0, 1.0)
    try:
        f.set_params(w0, w, v)
        f.upload_rows(0, d.entries, d.row_ptr, d.target)
        ef = f.evaluate(0)
    finally:
        f.close()
    assert not (ef.flags & capi.EVAL_WSIDE)
    # (a stale stream would be off by the epoch's steps of up to eta = 0.05 per weight; two handles agree to the order of their sums)
    assert ev.rmse == pytest.approx(ef.rmse, rel=1e-6) and ev.mae == pytest.approx(ef.mae, rel=1e-6)


def test_learner_and_cli(oracle, tmp_path):
    """`-optimizer adagrad` for five iterations ends at the parameters the restatement, driven the same way, ends at"""
    from libfm_amd import adaptive, cli
    from libfm_amd import refrand as R
    n, k, rows = 800, 8, 300
    d = oracle.synth_rows(21, 0, rows, 8, n)
    y = np.where(d.target <= 0.0, -1.0, 1.0).astype(np.float32)
    tr = oracle.Data(d.entries, d.row_ptr, y)
    te = oracle.synth_rows(21, rows, 100, 8, n)
    trf, tef, model = str(tmp_path / "tr.libfm"), str(tmp_path / "te.libfm"), str(tmp_path / "model")
    tr.write_libsvm(trf)
    te.write_libsvm(tef)
    argv = ["-task", "c", "-train", trf, "-test", tef, "-dim", "1,1,%d" % k, "-iter", "5", "-method", "sgd", "-learn_rate", "0.05",
            "-regular", "0.01,0.002,0.001", "-init_stdev", "0.1", "-seed", "42", "-save_model", model, "-optimizer", "adagrad",
            "-init_acc", "0.5", "-batch", "64", "-w0_chunk", "16"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(argv) == 0
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("#Iter=")]
    assert len(lines) == 5 and "Final\tTrain=" in buf.getvalue()
    n_attr = max(int(tr.entries["id"].max()), int(te.entries["id"].max())) + 1
    m = oracle.Model(n_attr, k, True, True, 0.01, 0.002, 0.001)
    R.srand(42)
    m.v[:] = R.init_v(k, n_attr, 0.0, 0.1)
    st = adaptive.AdaptState(n_attr, k, 0.5)
    for _ in range(5):
        adaptive.epoch(m, tr, 1, 0.05, -1.0, 1.0, 64, 16, st)
    txt = open(model).read().splitlines()
    assert txt[0] == "#global bias W0" and txt[2] == "#unary interactions Wj"
    w0 = float(txt[1])
    w = np.array([float(x) for x in txt[3:3 + n_attr]])
    v = np.array([[float(x) for x in ln.split()] for ln in txt[4 + n_attr:4 + 2 * n_attr]]).T
    # (the model file holds 6 significant digits: 5e-7 relative, inside the tolerances)
    assert abs(w0 - m.w0) <= RTOL * abs(m.w0) + ATOL
    np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=ATOL)
    assert float(lines[-1].split("\t")[1].split("=")[1]) == pytest.approx(oracle.evaluate(m, tr, 1, -1.0, 1.0)[0], abs=0.02)
