"""GPU: FTRL-proximal with L1 on the minibatch rule (fmx_ftrl_*, k_ftrl_apply_seg, k_ftrl_init) and the zero count of the model
(fmx_param_sparsity, k_param_sparsity) against the float64 restatement libfm_amd/ftrl.py (itself pinned to the AdaGrad restatement and
to hand-worked literals in tests/test_ftrl_cpu.py).

Tolerances.  Parameters: the project's rtol 1e-4 / atol 2e-5 (tests/test_gpu_adagrad.py).  z and n: rtol 1e-4 plus an absolute term,
because n starts at 0 and a gradient sum that cancels leaves an n with an unbounded relative gap (1.8 between the fp32 and the fp64
restatement).  The absolute term is 8 x the largest gap between the restatement run in fp32 and in fp64 at the test's own shape
(test_ftrl_cpu.ftrl_gaps, computed in the test): z 1.5e-6 .. 3.7e-6 and n 0.9e-6 .. 9.3e-6 at the parity shapes, z 1.1e-5 / 1.8e-5 and
n 2.5e-4 / 1.5e-4 on the long segments (k = 64 / 8, max n 846); x 8 for the device's different association of the sums.  Zero pattern:
theta == 0 agrees with the fp64 restatement on every coordinate except those with ||z64| - l1| <= 1e-4 (1 + l1), of which there may be
at most 0.1 % per table.

Measured on an MI355X (device against the fp64 restatement, largest over the cases; every test prints its own figures): parity shapes
parameters 2.4e-7, z 6.5e-6, n 1.2e-5 (absolute terms in force: z >= 1.2e-5, n >= 3.2e-6, the relative part on top); long segments z 1.3e-5,
n 1.3e-4 (terms 8.6e-5 / 1.5e-4 and 2.0e-3 / 1.2e-3); the AdaGrad identity 4.3e-7 on parameters, 1.2e-5 relative on n; 3.9 - 7.5 % of V and
12 - 21 % of w exactly zero; excluded near the threshold at most 0.05 % of a table (3 of 6400 linear weights, <= 0.008 % of V); no
mismatch of the zero pattern anywhere."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import datagen
from test_adagrad_cpu import hot_case
from test_ftrl_cpu import PARITY, ftrl_gaps, parity_case

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
N, ROWS, NNZ = 6400, 512, 32
LR = 0.01
ASSOC = 8.0                 # the device sums in another association than the fp32 restatement


def handle_for(capi, m, task, lr, lo=-1.0, hi=1.0, **kw):
    h = capi.Handle(m.n, m.k, m.k0, m.k1, task, m.reg0, m.regw, m.regv, lr, lo, hi, **kw)
    h.set_params(m.w0, m.w, m.v)
    return h


def check_zero_pattern(name, dev, ref, z64, l1):
    """theta == 0 on the device where the fp64 restatement has it, except within 1e-4 (1 + l1) of the threshold; at most 0.1 % excluded"""
    if dev.size == 0:
        return
    near = np.abs(np.abs(z64) - l1) <= 1e-4 * (1.0 + l1)
    wrong = ((dev == 0) != (ref == 0)) & ~near
    print("zeros %s: device %.4f  fp64 %.4f of %d; excluded near the threshold %.5f %%; mismatches %d" % (
        name, (dev == 0).mean(), (ref == 0).mean(), dev.size, 100.0 * near.mean(), int(wrong.sum())))
    assert near.mean() <= 1e-3
    assert not wrong.any()


def check_against(h, m, st, atol_z, atol_n):
    """parameters, every z and n and the zero pattern of the handle against the restatement's"""
    w0, w, v = h.get_params()
    zw, zv, nw, nv = h.ftrl_state_rows(np.arange(m.n, dtype=np.uint32))

    def gap(a, b):
        return float(np.abs(a - b).max()) if a.size else 0.0
    print("gaps: v %.3g  w %.3g  w0 %.3g  z_v %.3g  z_w %.3g  n_v %.3g  n_w %.3g  (absolute terms: z %.3g  n %.3g)" % (
        gap(v, m.v), gap(w, m.w), abs(w0 - m.w0), gap(zv, st.z_v), gap(zw, st.z_w), gap(nv, st.n_v), gap(nw, st.n_w), atol_z, atol_n))
    np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=ATOL)
    assert abs(w0 - m.w0) <= RTOL * abs(m.w0) + ATOL
    np.testing.assert_allclose(zv, st.z_v, rtol=RTOL, atol=atol_z)
    np.testing.assert_allclose(zw, st.z_w, rtol=RTOL, atol=atol_z)
    np.testing.assert_allclose(nv, st.n_v, rtol=RTOL, atol=atol_n)
    np.testing.assert_allclose(nw, st.n_w, rtol=RTOL, atol=atol_n)
    check_zero_pattern("v", v, m.v, st.z_v, st.l1_v)
    if m.k1:
        check_zero_pattern("w", w, m.w, st.z_w, st.l1_w)
    return w, v


def run_case(d, m, task, lr, batch, chunk, opts, epochs=3):
    """`epochs` epochs on the device and in the fp64 restatement from the same start; returns (handle's final w, v, restatement m, st)"""
    from libfm_amd import capi, ftrl
    _, gz, gn = ftrl_gaps(d, m, task, lr, batch, chunk, epochs, opts)
    m = m.copy()
    st = ftrl.FtrlState(m, **opts)
    h = handle_for(capi, m, task, lr)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        h.ftrl_begin(**opts)
        for _ in range(epochs):
            es = h.ftrl_epoch(0, batch, chunk)
            ftrl.epoch(m, d, task, lr, -1.0, 1.0, batch, chunk, st)
        w, v = check_against(h, m, st, ASSOC * gz, ASSOC * gn)
        sp = h.param_sparsity()
    finally:
        h.close()
    assert (sp.features, sp.v_coords) == (m.n, m.n * m.k)
    assert sp.w_zero == int((w == 0).sum()) and sp.v_zero == int((v == 0).sum())
    assert sp.v_zero_rows == int((v == 0).all(axis=0).sum())
    assert sp.dead_features == int(((v == 0).all(axis=0) & ((w == 0) | (not m.k1))).sum())
    return es, w, v, m, st


def run_parity(k, task, k0=True, k1=True, opts=PARITY):
    d, m0 = parity_case(k, k0, k1)
    es, w, v, m, st = run_case(d, m0, task, LR, 64, 16, opts)
    assert es.rows == ROWS and es.batches == 8 and es.batch_used == 64 and es.w0_chunk_used == 16
    assert es.main_kernel_launches == 8 and es.device_seconds > 0 and es.max_feature_count >= 1
    assert np.abs(m.v - m0.v).max() > 1e-3                       # (three epochs moved the parameters far beyond the tolerances)
    if opts["l1_v"] > 0:
        assert 0.01 < (v == 0).mean() < 0.5                      # (and L1 produced zeros, not only zeros)
    if not k1:
        assert np.all(w == m0.w) and np.all(st.n_w == 0.0)
    elif opts["l1_w"] > 0:
        assert 0.05 < (w == 0).mean() < 0.5


# every width the owner kernel is instantiated for: six of them under both tasks, the other six once (regression 2, 16, 512; classification 4, 32, 1024)
PARITY_WIDTHS = [(k, task) for k in (1, 8, 64, 100, 128, 256) for task in (0, 1)] + [(2, 0), (16, 0), (512, 0), (4, 1), (32, 1), (1024, 1)]


@pytest.mark.parametrize("k, task", PARITY_WIDTHS)
def test_parity(k, task):
    """several rows per wave-wide load (k 1, 8), VEC 1, 2 and 4 (k 64, 128, 256), a row shorter than KP (k 100: 112 floats under KP 128);
    the remaining widths once each (k 2, 4, 16, 32; VEC 8 and 16 with fewer segment groups per round: k 512, 1024)"""
    run_parity(k, task)


def test_parity_without_linear_weights():
    run_parity(8, 1, k1=False)


def test_parity_without_bias():
    run_parity(8, 0, k0=False)


def test_parity_beta_zero_with_init_acc():
    run_parity(8, 1, opts=dict(PARITY, beta=0.0, init_acc=1.0))


@pytest.mark.parametrize("task", [0, 1])
def test_adagrad_identity_on_the_device(task):
    """l1 = l2 = beta = 0, init_acc = a, alpha = eta on a handle with regw = regv = 0 is AdaGrad: against fmx_adapt_epoch's own result"""
    from libfm_amd import capi
    eta, a0 = 0.05, 0.5
    d, m = parity_case(64)
    m.regw = m.regv = 0.0
    ids = np.arange(N, dtype=np.uint32)
    res = []
    for rule in ("adagrad", "ftrl"):
        h = handle_for(capi, m, task, LR)
        try:
            h.upload_rows(0, d.entries, d.row_ptr, d.target)
            if rule == "adagrad":
                h.adapt_begin("adagrad", a0, eta)
            else:
                h.ftrl_begin(eta, 0.0, init_acc=a0)
            for _ in range(3):
                (h.adapt_epoch if rule == "adagrad" else h.ftrl_epoch)(0, 64, 16)
            res.append(h.get_params() + (h.adapt_state_rows(ids) if rule == "adagrad" else h.ftrl_state_rows(ids)[2:]))
        finally:
            h.close()
    (w0a, wa, va, nwa, nva), (w0f, wf, vf, nwf, nvf) = res
    print("gaps: v %.3g  w %.3g  w0 %.3g  n_v (rel) %.3g  n_w (rel) %.3g" % (
        np.abs(va - vf).max(), np.abs(wa - wf).max(), abs(w0a - w0f), (np.abs(nva - nvf) / nva).max(), (np.abs(nwa - nwf) / nwa).max()))
    np.testing.assert_allclose(vf, va, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(wf, wa, rtol=RTOL, atol=ATOL)
    assert abs(w0f - w0a) <= RTOL * abs(w0a) + ATOL
    np.testing.assert_allclose(nvf, nva, rtol=RTOL)              # (n starts at 0.5: a relative bound holds here)
    np.testing.assert_allclose(nwf, nwa, rtol=RTOL)
    assert np.abs(va - m.v).max() > 1e-3


@pytest.mark.parametrize("k", [64, 8])
def test_long_segments(oracle, k):
    """the hot-feature case: id 0 in every row (one segment of 512 occurrences: the tail loop past 64) and a tail batch of 88 rows"""
    d, m8 = hot_case()
    m = oracle.Model(m8.n, k, True, True, 0.0, 0.002, 0.001)
    m.v[:] = oracle.init_values(1, m.n, k, 0.05)
    es, w, v, ref, st = run_case(d, m, 0, 0.05, 512, 8, PARITY)
    assert es.batches == 2 and es.max_feature_count == 512
    assert st.n_w.max() > 100.0                                  # (the hot feature's n: the relative part of the tolerance carries it)


def test_bit_reproducible():
    from libfm_amd import capi
    d, m = parity_case(64)
    res = []
    for _ in range(2):
        h = handle_for(capi, m, 1, LR)
        try:
            h.upload_rows(0, d.entries, d.row_ptr, d.target)
            h.ftrl_begin(**PARITY)
            for _ in range(2):
                h.ftrl_epoch(0, 64, 16)
            res.append(h.get_params() + h.ftrl_state_rows(np.arange(N, dtype=np.uint32)))
        finally:
            h.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_state():
    from libfm_amd import capi, ftrl
    k = 8
    d, m = parity_case(k)
    m.w[::7] = 0.0                                               # (zeros in the start values: z0 = 0 there)
    m.v[:, ::5] = 0.0
    ids = np.arange(N, dtype=np.uint32)
    touched = np.zeros(N, dtype=bool)
    touched[d.entries["id"]] = True
    assert touched.any() and not touched.all()
    opts = dict(PARITY, init_acc=0.25)
    h = handle_for(capi, m, 1, LR)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        _, w_before, v_before = h.get_params()                   # (as the device holds them: fp32)
        h.ftrl_begin(**opts)
        # the start state: n = init_acc, z0 = -theta0 D0 - sgn(theta0) l1 from the device's own fp32 parameters (a few fp32 roundings)
        zw, zv, nw, nv = h.ftrl_state_rows(ids)
        assert np.all(nw == 0.25) and np.all(nv == 0.25)
        for z, theta, l1, l2 in ((zw, w_before, 0.5, 0.01), (zv, v_before, 0.3, 0.01)):
            D0 = (1.0 + 0.5) / 0.05 + l2
            np.testing.assert_allclose(z, -theta * D0 - np.sign(theta) * l1, rtol=1e-6)
            assert np.all(z[theta == 0.0] == 0.0)
        for a, b in zip((w_before, v_before), h.get_params()[1:]):
            assert np.array_equal(a, b)                          # (begin changes nothing in the model)
        es = h.ftrl_epoch(0)                                      # batch 0 / micro-chunk 0: the library's choices
        assert es.batch_used >= 32 and es.w0_chunk_used == capi.default_w0_chunk(LR, 1) and es.rows == ROWS
        _, w, v = h.get_params()
        zw1, zv1, nw1, nv1 = h.ftrl_state_rows(ids)
        # untouched features: theta, z and n bit-unchanged; touched ones moved
        assert np.array_equal(w[~touched], w_before[~touched]) and np.array_equal(v[:, ~touched], v_before[:, ~touched])
        assert np.array_equal(zw1[~touched], zw[~touched]) and np.array_equal(zv1[:, ~touched], zv[:, ~touched])
        assert np.all(nw1[~touched] == 0.25) and np.all(nv1[:, ~touched] == 0.25)
        assert np.all(nw1[touched] >= 0.25) and (nw1[touched] > 0.25).mean() > 0.99 and (zw1[touched] != zw[touched]).mean() > 0.99
        # a subset of rows, in the caller's order
        sub = np.array([5, 0, 6399, 17], dtype=np.uint32)
        s = h.ftrl_state_rows(sub)
        assert np.array_equal(s[0], zw1[sub]) and np.array_equal(s[1], zv1[:, sub])
        assert np.array_equal(s[2], nw1[sub]) and np.array_equal(s[3], nv1[:, sub])
        # fmx_sgd_epoch and fmx_set_params inside a session leave z and n alone
        h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, 64, 16)
        h.set_params(m.w0, m.w, m.v)
        for a, b in zip(h.ftrl_state_rows(ids), (zw1, zv1, nw1, nv1)):
            assert np.array_equal(a, b)
        # begin again resets: n = the new init_acc, z from the parameters of THAT moment (here the start values again, new options)
        h.ftrl_begin(0.1, 2.0, 0.0, 0.0, 0.0, 0.0, 1.0)
        zw, zv, nw, nv = h.ftrl_state_rows(ids)
        assert np.all(nw == 1.0) and np.all(nv == 1.0)
        np.testing.assert_allclose(zv, -v_before * ((2.0 + 1.0) / 0.1), rtol=1e-6)
        np.testing.assert_allclose(zw, -w_before * ((2.0 + 1.0) / 0.1), rtol=1e-6)
        # alpha 0 = the handle's learn_rate, beta 1, no l1 / l2, init_acc 0: one epoch equals the restatement's with those values (from
        # start values without planted zeros: with l1 = 0 a coordinate that starts at 0 has z = 0, which IS the threshold)
        _, m = parity_case(k)
        h.set_params(m.w0, m.w, m.v)
        h.ftrl_begin()
        ref = m.copy()
        st = ftrl.FtrlState(ref, LR, 1.0)
        _, gz, gn = ftrl_gaps(d, m, 1, LR, 64, 16, 1, dict(alpha=LR, beta=1.0))
        h.ftrl_epoch(0, 64, 16)
        ftrl.epoch(ref, d, 1, LR, -1.0, 1.0, 64, 16, st)
        check_against(h, ref, st, ASSOC * gz, ASSOC * gn)
        # an empty slot
        h.upload_rows(1, np.zeros(0, dtype=capi.ENTRY_DTYPE), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.float32))
        es = h.ftrl_epoch(1, 64, 16)
        assert es.rows == 0 and es.batches == 0
        h.ftrl_end()
        h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, 64, 16)     # the handle trains on without a session
    finally:
        h.close()


def test_refusals():
    from libfm_amd import capi
    k = 8
    d, m = parity_case(k, n=100, rows=64, nnz=8)
    h = handle_for(capi, m, 0, LR)

    def code(fn, *a, **kw):
        with pytest.raises(capi.FmxError) as ei:
            fn(*a, **kw)
        return ei.value.code

    def begin_raw(*vals, flags=0):
        return h.lib.fmx_ftrl_begin(h.h, C.byref(capi.FtrlOpts(flags, 0, *vals)))
    good = [0.05, 1.0, 0.1, 0.1, 0.01, 0.01, 0.0]                 # alpha, beta, l1_w, l1_v, l2_w, l2_v, init_acc
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        h.upload_rows(1, d.entries, d.row_ptr, None)              # no targets
        ids = np.arange(4, dtype=np.uint32)
        # without a session
        assert code(h.ftrl_epoch, 0, 16, 4) == -3 and code(h.ftrl_state_rows, ids) == -3 and code(h.ftrl_end) == -3
        # FMX_E_ARG of begin
        assert h.lib.fmx_ftrl_begin(h.h, None) == -1
        assert begin_raw(*good, flags=1) == -1
        for i in range(len(good)):
            for bad in (-1.0, float("nan"), float("inf")):
                vals = list(good)
                vals[i] = bad
                assert begin_raw(*vals) == -1, (i, bad)
        assert begin_raw(1e-60, *good[1:]) == -1                  # alpha: not a positive fp32 number
        assert begin_raw(1e60, *good[1:]) == -1
        assert begin_raw(0.05, 0.0, 0.1, 0.1, 0.01, 0.01, 0.0) == -1        # beta == 0 && init_acc == 0
        assert code(h.ftrl_epoch, 0, 16, 4) == -3                 # (none of them opened a session)
        # an open SGDA or AdaGrad session, both ways round
        h.sgda_begin()
        assert code(h.ftrl_begin) == -3
        h.sgda_end()
        h.set_params(m.w0, m.w, m.v)                              # (fmx_sgda_begin zeroed w)
        h.adapt_begin()
        assert code(h.ftrl_begin) == -3
        h.adapt_end()
        h.ftrl_begin(*good)
        assert code(h.sgda_begin) == -3 and code(h.adapt_begin) == -3
        # slots
        assert code(h.ftrl_epoch, 5, 16, 4) == -3                 # never uploaded
        assert code(h.ftrl_epoch, 1, 16, 4) == -3                 # without targets
        # outputs and ids of _get_state_rows
        bufs = [np.zeros(4), np.zeros((4, k)), np.zeros(4), np.zeros((4, k))]
        for i in range(4):
            ptrs = [b.ctypes.data for b in bufs]
            ptrs[i] = None
            assert h.lib.fmx_ftrl_get_state_rows(h.h, ids.ctypes.data, 4, *ptrs) == -1
        assert h.lib.fmx_ftrl_get_state_rows(h.h, None, 4, *[b.ctypes.data for b in bufs]) == -1
        assert code(h.ftrl_state_rows, np.array([3, 100], dtype=np.uint32)) == -1
        assert h.lib.fmx_param_sparsity(h.h, None) == -1
        # an open ALS / MCMC session on the slot
        h.als_begin(0)
        assert code(h.ftrl_epoch, 0, 16, 4) == -3
        h.als_end()
        # kept `-relation` blocks
        be, br, _ = datagen.ragged_real(20, 4, 3, seed=62)
        h.upload_block_rows(4, d.entries, d.row_ptr, d.target, [(be, br, np.arange(64) % 4, 80)], keep=True)
        with pytest.raises(capi.FmxError) as ei:
            h.ftrl_epoch(4, 16, 4)
        assert ei.value.code == -4 and "relations are not supported with SGD" in ei.value.text
        # the handle and the session work afterwards
        es = h.ftrl_epoch(0, 16, 4)
        assert es.rows == 64 and es.batches == 4
        assert h.param_sparsity().features == 100
        h.ftrl_end()
    finally:
        h.close()
    # a feature shard, a communicator rank
    hs = capi.Handle(100, k, shard_rank=0, shard_world=2, learn_rate=LR)
    try:
        for fn in (hs.ftrl_begin, hs.param_sparsity):
            with pytest.raises(capi.FmxError) as ei:
                fn()
            assert ei.value.code == -4
    finally:
        hs.close()
    hc = capi.Handle(100, k, learn_rate=LR)
    try:
        hc.comm_init_rank(capi.comm_unique_id(), 0, 1)
        for fn in (hc.ftrl_begin, hc.param_sparsity):
            with pytest.raises(capi.FmxError) as ei:
                fn()
            assert ei.value.code == -4
    finally:
        hc.close()


def test_epoch_invalidates_a_kept_weight_side_stream():
    """a fused epoch with FMX_FLAG_KEEP_WSIDE leaves the slot's weight side stream valid; an FTRL epoch changes the linear weights, so
    fmx_evaluate afterwards must not read it: it equals fmx_evaluate on a fresh handle given the same parameters"""
    from libfm_amd import capi
    d, m = parity_case(8)
    h = handle_for(capi, m, 0, LR)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_FUSED, 64, 16, capi.FLAG_KEEP_WSIDE, 2)
        assert h.evaluate(0).flags & capi.EVAL_WSIDE             # (the stream is there and current)
        h.ftrl_begin(**PARITY)
        h.ftrl_epoch(0, 64, 16)
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
    # (a stale stream would be off by the epoch's steps -- with l1_w = 0.5 whole weights went to zero; two handles agree to the order of their sums)
    assert ev.rmse == pytest.approx(ef.rmse, rel=1e-6) and ev.mae == pytest.approx(ef.mae, rel=1e-6)


def planted(k, n):
    """w[n], v[k][n] of magnitudes 0.5 .. 1.5 with zeros of both signs, NaNs and whole zero rows (some with one NaN) planted"""
    rng = np.random.default_rng(1000 * k + n)
    w = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    v = rng.uniform(0.5, 1.5, (k, n)) * rng.choice([-1.0, 1.0], (k, n))
    w[rng.random(n) < 0.3] = 0.0
    w[rng.random(n) < 0.1] = -0.0
    w[rng.random(n) < 0.05] = np.nan
    v[rng.random((k, n)) < 0.3] = 0.0
    v[rng.random((k, n)) < 0.1] = -0.0
    v[rng.random((k, n)) < 0.02] = np.nan
    rows0 = rng.random(n) < 0.4
    v[:, rows0] = 0.0
    if k:
        v[0, rows0 & (rng.random(n) < 0.3)] = -0.0
        v[k - 1, rows0 & (rng.random(n) < 0.1)] = np.nan
    if n == 1:
        w[0] = -0.0
        v[:, 0] = 0.0
    return w, v


@pytest.mark.parametrize("k1", [True, False])
@pytest.mark.parametrize("n", [1, 200, 4099])
@pytest.mark.parametrize("k", [0, 1, 100])
def test_param_sparsity(k, n, k1):
    """planted zeros, -0 (counts) and NaN (does not) against numpy: no factors, one lane group per wavefront round and 64 (k 0, 1), a
    row of 112 floats of which 100 count (k 100); one feature, less than one wavefront of features, and a count no multiple of 64"""
    from libfm_amd import capi
    w, v = planted(k, n)
    h = capi.Handle(n, k, True, k1, 0, 0.0, 0.0, 0.0, LR, -1.0, 1.0)
    try:
        h.set_params(0.0, w, v)
        sp = h.param_sparsity()
        dead = (v == 0).all(axis=0) & ((w == 0) | (not k1))
        want = (n, int((w == 0).sum()), n * k, int((v == 0).sum()), int((v == 0).all(axis=0).sum()), int(dead.sum()))
        assert (sp.features, sp.w_zero, sp.v_coords, sp.v_zero, sp.v_zero_rows, sp.dead_features) == want
        if n > 1:
            assert 0 < want[1] < n and (k == 0 or 0 < want[3] < n * k) and 0 < want[5] <= want[4]
            assert np.isnan(w).any() and (k == 0 or np.isnan(v).any()) and np.signbit(w[w == 0]).any()
        sp2 = h.param_sparsity()                                  # (integer sums: the same again)
        assert (sp2.w_zero, sp2.v_zero, sp2.v_zero_rows, sp2.dead_features) == (want[1], want[3], want[4], want[5])
    finally:
        h.close()


def test_learner_and_cli(oracle, tmp_path, capsys):
    """`-optimizer ftrl` for five iterations ends at the parameters the restatement, driven the same way, ends at, and reports the zero
    counts of the model it saved; the learner's own sparsity() is the device's count of the model it hands back"""
    from libfm_amd import cli, ftrl
    from libfm_amd import learner as L
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
            "-regular", "0.01,0.02,0.01", "-init_stdev", "0.1", "-seed", "42", "-save_model", model, "-optimizer", "ftrl",
            "-ftrl_alpha", "0.1", "-ftrl_beta", "0.5", "-l1", "0.3,0.2", "-batch", "64", "-w0_chunk", "16"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(argv) == 0
    err = capsys.readouterr().err
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("#Iter=")]
    assert len(lines) == 5 and "Final\tTrain=" in buf.getvalue()
    n_attr = max(int(tr.entries["id"].max()), int(te.entries["id"].max())) + 1
    m = oracle.Model(n_attr, k, True, True, 0.01, 0.02, 0.01)
    R.srand(42)
    m.v[:] = R.init_v(k, n_attr, 0.0, 0.1)
    st = ftrl.FtrlState(m, 0.1, 0.5, 0.3, 0.2, 0.02, 0.01)
    for _ in range(5):
        ftrl.epoch(m, tr, 1, 0.05, -1.0, 1.0, 64, 16, st)
    txt = open(model).read().splitlines()
    assert txt[0] == "#global bias W0" and txt[2] == "#unary interactions Wj"
    w0 = float(txt[1])
    w = np.array([float(x) for x in txt[3:3 + n_attr]])
    v = np.array([[float(x) for x in ln.split()] for ln in txt[4 + n_attr:4 + 2 * n_attr]]).T
    # (the model file holds 6 significant digits: 5e-7 relative, inside the tolerances)
    assert abs(w0 - m.w0) <= RTOL * abs(m.w0) + ATOL
    np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=ATOL)
    check_zero_pattern("v", v, m.v, st.z_v, 0.2)
    check_zero_pattern("w", w, m.w, st.z_w, 0.3)
    assert (v == 0).mean() > 0.01
    sp_line = [ln for ln in err.splitlines() if ln.startswith("sparsity\t")]
    assert len(sp_line) == 1
    got = dict(t.split("=") for t in sp_line[0].split("\t")[1:])
    dead = (v == 0).all(axis=0) & (w == 0)
    assert {a: int(b) for a, b in got.items()} == {
        "features": n_attr, "w_zero": int((w == 0).sum()), "v_coords": n_attr * k, "v_zero": int((v == 0).sum()),
        "v_zero_rows": int((v == 0).all(axis=0).sum()), "dead_features": int(dead.sum())}
    assert float(lines[-1].split("\t")[1].split("=")[1]) == pytest.approx(oracle.evaluate(m, tr, 1, -1.0, 1.0)[0], abs=0.02)
    # the learner, driven directly (l2 None = the model's regw / regv): the same parameters, and sparsity() counts the model it hands back
    fm = L.FMModel()
    fm.num_attribute, fm.num_factor, fm.reg0, fm.regw, fm.regv = n_attr, k, 0.01, 0.02, 0.01
    R.srand(42)
    fm.w0, fm.w, fm.v = 0.0, np.zeros(n_attr), R.init_v(k, n_attr, 0.0, 0.1)
    l = L.FMLearnSGD()
    l.fm, l.task, l.num_iter, l.learn_rate, l.batch, l.w0_chunk = fm, 1, 5, 0.05, 64, 16
    l.min_target, l.max_target = -1.0, 1.0
    l.optimizer, l.ftrl_alpha, l.ftrl_beta, l.l1_w, l.l1_v = "ftrl", 0.1, 0.5, 0.3, 0.2
    l.out = io.StringIO()
    l.init()
    try:
        l.learn(L.Data(tr.entries, tr.row_ptr, tr.target), L.Data(te.entries, te.row_ptr, te.target))
        sp = l.sparsity()
    finally:
        l.close()
    np.testing.assert_allclose(fm.v, m.v, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(fm.w, m.w, rtol=RTOL, atol=ATOL)
    assert (sp.w_zero, sp.v_zero, sp.v_zero_rows) == (int((fm.w == 0).sum()), int((fm.v == 0).sum()), int((fm.v == 0).all(axis=0).sum()))
    assert sp.v_zero == int(got["v_zero"]) and sp.w_zero == int(got["w_zero"])       # (bit-reproducible: the CLI's run again)
