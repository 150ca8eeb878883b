"""GPU: the field-matrixed FM (fmx_fmfm_*, k_fmfm_sums / k_fmfm_gemm_t / k_fmfm_apply_seg / k_fmfm_mgrad / k_fmfm_mstep) against its
float64 restatement libfm_amd/fmfm.py (itself pinned to a brute-force double loop and to finite differences in tests/test_fmfm_cpu.py).

Tolerances start from tests/test_gpu_adagrad.py's: w0, w, v, M and predictions at rtol 1e-4 / atol 2e-5, the accumulators at rtol 1e-4.
The restatement run in fp32 (numpy) against itself in fp64 on exactly the cases below, and the device's largest gaps:
                                 predictions   w0       w        v        M        n_w      n_v      n_M   (parameters absolute,
    203 rows       fp32 numpy    7.9e-6        3.0e-7   1.6e-6   4.1e-6   2.9e-7   2.8e-5   9.8e-5   4.0e-6   accumulators relative)
                   device        4.1e-6        1.5e-7   1.8e-6   7.1e-6   5.1e-7   2.3e-5   1.1e-4   6.7e-6
    2233 rows      fp32 numpy                  7.2e-7   5.3e-6   5.5e-6   1.9e-6   1.6e-4   2.0e-4   4.1e-5
    (tiled x 11)   device                      1.0e-6   4.2e-6   4.7e-6   2.0e-6   1.2e-4   1.6e-4   4.0e-5
Four times the restatement's deviation is inside the tolerances except for n_w and n_v (203 rows) and for v, n_w, n_v and n_M (2233 rows:
4 x 5.5e-6 is 1.001 of v's tolerance at the worst element); those take 4x the restatement's own deviation (WIDER)."""
import types

import numpy as np
import pytest

import datagen
import fwfm_cases

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
# 4x the fp32 restatement's deviation where that is beyond the tolerances above (atol of v, rtol of n_w, n_v, n_M), by the rows' repetition
WIDER = {1: (ATOL, 1.12e-4, 3.93e-4, RTOL), 11: (2.19e-5, 6.48e-4, 8.16e-4, 1.63e-4)}
LR, ETA = 0.01, 0.05
ROWS = 203
BM, MCHUNK, MSPLIT = 64, 128, 8                                   # FMFM_BM of k_fmfm_gemm_t, FMFM_MCHUNK and FMFM_MSPLIT of k_fmfm_mgrad
WRAP = MCHUNK * MSPLIT                                            # from here on a partial of k_fmfm_mgrad walks more than one chunk


def random_m(F, k):
    from libfm_amd import fmfm
    return fmfm.random_m(F, k, np.random.default_rng(3 + 7 * F + k))



def open_handle(capi, m, groups, task=0, M=None, adagrad=False):
    h = capi.Handle(m.n, m.k, m.k0, m.k1, task, m.reg0, m.regw, m.regv, LR, -1.0, 1.0)
    h.set_params(m.w0, m.w, m.v)
    h.set_groups(groups)
    if adagrad:
        h.adapt_begin("adagrad", 1.0, ETA)
    h.fmfm_begin()
    if M is not None:
        h.fmfm_set_m(M)
    return h


@pytest.mark.parametrize("k, F", [(1, 1), (1, 17), (5, 3), (8, 2), (20, 5), (16, 39), (64, 17), (32, 64)])
def test_predict(oracle, k, F):
    """WP = 16, 32, 32, 16 (one MFMA block), 160 (k below KP), 624 (no multiple of the 64-wide tile), 1088, 2048 (the bound)"""
    from libfm_amd import capi, fmfm
    m, groups, _, d = fwfm_cases.make(oracle, k, F)
    M = random_m(F, k)
    h = open_handle(capi, m, groups, M=M)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        got = h.fmfm_predict(0, d.n_rows)
        ref = fmfm.predict(m, M, groups, d)
        print("k %d F %d: largest gap %.3g" % (k, F, np.abs(got - ref).max()))
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
        assert abs(h.fmfm_evaluate(0).rmse - np.sqrt(np.mean((np.clip(ref, -1, 1) - d.target) ** 2))) < 1e-4
        h.fmfm_set_m(fmfm.identity(F, k))                           # M == I is the plain FM: fmx_predict of the same handle
        np.testing.assert_allclose(h.fmfm_predict(0, d.n_rows), h.predict(0, d.n_rows), rtol=RTOL, atol=ATOL)
    finally:
        h.close()


def state_of(h, n):
    return h.get_params() + h.adapt_state_rows(np.arange(n, dtype=np.uint32)) + h.fmfm_get_m()


def tiled(d, times):                                                # the case's rows repeated, to reach a constant beyond 203 rows
    ptr = np.concatenate([[0], np.cumsum(np.tile(np.diff(d.row_ptr.astype(np.int64)), times))]).astype(d.row_ptr.dtype)
    return types.SimpleNamespace(entries=np.tile(d.entries, times), row_ptr=ptr, target=np.tile(d.target, times), n_rows=d.n_rows * times)


SHAPES = [(4, 3), (20, 5), (16, 17)]
BATCHES = [1, 7, 0, ROWS - 1, BM - 1, BM, BM + 1, MCHUNK - 1, MCHUNK, MCHUNK + 1]
# ... and on (20, 5) the rows 11 times over (2233): the wrap of a partial to its next chunk, and all rows in one batch -- 18 chunks, three
# for partials 0 and 1
CASES = [(k, F, b, 1) for k, F in SHAPES for b in BATCHES] + [(20, 5, b, 11) for b in (WRAP - 1, WRAP, WRAP + 1, 11 * ROWS)]


@pytest.mark.parametrize("task", [0, 1])
@pytest.mark.parametrize("k, F, batch, times", CASES)
def test_training(oracle, k, F, batch, times, task):
    from libfm_amd import adaptive, capi, fmfm
    m, groups, _, d = fwfm_cases.make(oracle, k, F, task)
    d = tiled(d, times) if times > 1 else d
    M = random_m(F, k)
    before, M0 = m.copy(), M.copy()
    st, nM = adaptive.AdaptState(m.n, k, 1.0), np.ones((F, F, k, k))
    h = open_handle(capi, m, groups, task, M, adagrad=True)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        for _ in range(3):
            es = h.fmfm_epoch(0, batch, 16)
            fmfm.epoch(m, st, M, nM, groups, d, task, LR, -1.0, 1.0, batch, 16, eta=ETA)
        assert es.rows == d.n_rows and es.batches == (1 if batch == 0 else -(-d.n_rows // batch))
        w0, w, v, nw, nv, gM, gnM = state_of(h, m.n)
    finally:
        h.close()
    rel = lambda a, b: (np.abs(a - b) / np.abs(b)).max()
    print("gaps: v %.3g w %.3g w0 %.3g M %.3g n_v %.3g n_w %.3g n_M %.3g" % (np.abs(v - m.v).max(), np.abs(w - m.w).max(), abs(w0 - m.w0),
                                                                            np.abs(gM - M).max(), rel(nv, st.n_v), rel(nw, st.n_w), rel(gnM, nM)))
    atol_v, rtol_nw, rtol_nv, rtol_nm = WIDER[times]
    for got, ref, atol in ((v, m.v, atol_v), (w, m.w, ATOL), (w0, m.w0, ATOL), (gM, M, ATOL)):
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=atol)
    for got, ref, rtol in ((nv, st.n_v, rtol_nv), (nw, st.n_w, rtol_nw), (gnM, nM, rtol_nm)):
        np.testing.assert_allclose(got, ref, rtol=rtol)
    for a in (gM, gnM):                                             # every lower block exactly the transpose of its upper block
        assert np.array_equal(a, a.transpose(1, 0, 3, 2))
    assert all(np.array_equal(gM[g, g], np.eye(k)) and np.array_equal(gnM[g, g], np.ones((k, k))) for g in range(F))
    assert np.abs(m.v - before.v).max() > 1e-3 and np.abs(M - M0).max() > 1e-3  # (moved far beyond the tolerances)


def test_bit_reproducible_and_untouched_features(oracle):
    from libfm_amd import capi
    m, groups, _, d = fwfm_cases.make(oracle, 16, 17, 1)
    M = random_m(17, 16)
    unseen = np.ones(m.n, dtype=bool)
    unseen[d.entries["id"]] = False
    res = []
    for _ in range(2):
        h = open_handle(capi, m, groups, 1, M, adagrad=True)
        try:
            h.upload_rows(0, d.entries, d.row_ptr, d.target)
            start = state_of(h, m.n)
            h.fmfm_epoch(0, 48, 16)
            h.fmfm_epoch(0, 48, 16)
            res.append(state_of(h, m.n))
        finally:
            h.close()
    assert all(np.array_equal(a, b) for a, b in zip(*res))
    for i in (1, 2, 3, 4):                                          # w, v, n_w, n_v: last axis the feature
        assert np.array_equal(res[0][i][..., unseen], start[i][..., unseen]) and not np.array_equal(res[0][i][..., ~unseen], start[i][..., ~unseen])


def test_learner_and_cli(oracle, tmp_path):
    """three iterations of `-model fmfm` and of the learner with model="fmfm" end at the matrices the restatement, driven the same way, ends at"""
    from libfm_amd import adaptive, cli, fmfm, learner as L
    from libfm_amd import refrand as R
    (_, groups, _, d), k, F = fwfm_cases.make(oracle, 8, 5, 1), 8, 5
    trf, meta, mout = str(tmp_path / "tr.libfm"), str(tmp_path / "meta"), str(tmp_path / "m.txt")
    d.write_libsvm(trf)
    n, reg = d.num_feature, (0.01, 0.002, 0.001)
    np.savetxt(meta, groups[:n], fmt="%d")
    assert cli.main(["-task", "c", "-train", trf, "-test", trf, "-dim", "1,1,%d" % k, "-iter", "3", "-method", "sgd", "-learn_rate", "0.05",
                     "-regular", "%g,%g,%g" % reg, "-init_stdev", "0.1", "-seed", "42", "-optimizer", "adagrad", "-batch", "64",
                     "-w0_chunk", "16", "-model", "fmfm", "-meta", meta, "-m_out", mout]) == 0
    m = oracle.Model(n, k, True, True, *reg)
    R.srand(42)
    m.v[:] = R.init_v(k, n, 0.0, 0.1)
    l = L.FMLearnSGD()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor, (l.fm.reg0, l.fm.regw, l.fm.regv) = n, k, reg
    l.fm.w0, l.fm.w, l.fm.v = 0.0, np.zeros(n), m.v.copy()
    l.task, l.num_iter, l.learn_rate, l.batch, l.w0_chunk, l.min_target, l.max_target = 1, 3, 0.05, 64, 16, -1.0, 1.0
    l.optimizer, l.model, l.groups, l.out = "adagrad", "fmfm", groups[:n], open(str(tmp_path / "log"), "w")
    st, M, nM = adaptive.AdaptState(n, k, 1.0), fmfm.identity(F, k), np.ones((F, F, k, k))
    for _ in range(3):
        fmfm.epoch(m, st, M, nM, groups[:n], d, 1, 0.05, -1.0, 1.0, 64, 16)
    assert np.abs(M - fmfm.identity(F, k)).max() > 1e-3
    lines = [ln.split() for ln in open(mout)]                       # a line `g h`, then the block's k rows; 6 significant digits
    assert [tuple(int(x) for x in ln) for ln in lines[::k + 1]] == list(zip(*np.triu_indices(F, 1)))
    blocks = np.array([ln for i, ln in enumerate(lines) if i % (k + 1)], dtype=np.float64).reshape(-1, k, k)
    np.testing.assert_allclose(blocks, M[np.triu_indices(F, 1)], rtol=RTOL, atol=ATOL)
    data = L.Data(d.entries, d.row_ptr, d.target)
    try:
        l.init()
        l.learn(data, data)
        np.testing.assert_allclose(l.m, M, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(l.predict_raw(data), fmfm.predict(m, M, groups[:n], d), rtol=RTOL, atol=ATOL)
        with pytest.raises(NotImplementedError):
            l.evaluate_ex(data)
    finally:
        l.close()


def bad_m(i):                       # not the transpose; not finite; a diagonal block that is not the identity (twice)
    bad = random_m(5, 8)
    at, val = [((0, 1, 2, 3), 9.0), ((2, 3, 0, 0), float("nan")), ((2, 2, 1, 1), 0.5), ((1, 1, 0, 3), 1e-9)][i]
    bad[at] = val
    return bad


OPTS = ["0.0, 0.0, 0.0, 1"] + ["%s0" % "".join(bad + ", " if j == i else "0.0, " for j in range(3))
                               for bad in ("-1.0", "float('nan')", "float('inf')") for i in range(3)]
BEGIN, OPEN = ["h.fmfm_begin()"], "h.fmfm_begin(); "
# what: (factors, fields (0: a bare handle, no rows), set-up, the calls that are refused, their code, what undoes the set-up)
REFUSALS = {
    "no_session": (8, 5, "", ["h.fmfm_epoch(0)", "h.fmfm_predict(0, ROWS)", "h.fmfm_evaluate(0)", "h.fmfm_get_m()",
                              "h.fmfm_set_m(random_m(5, 8))", "h.fmfm_end()"], -3, ""),
    "no_adagrad": (8, 5, OPEN, ["h.fmfm_epoch(0)"], -3, ""),
    "bad_opts": (8, 5, "", ["h.lib.fmx_fmfm_begin(h.h, None)"] + ["h.lib.fmx_fmfm_begin(h.h, C.byref(capi.FmfmOpts(%s)))" % o for o in OPTS], -1, ""),
    "bad_m": (8, 5, OPEN, ["h.fmfm_set_m(bad_m(%d))" % i for i in range(4)], -1, ""),
    "null_pointers": (8, 5, OPEN, ["h.lib.fmx_fmfm_set_m(h.h, None)", "h.lib.fmx_fmfm_get_m(h.h, None, None)",
                                   "h.lib.fmx_fmfm_predict(h.h, 0, None)", "h.lib.fmx_fmfm_evaluate(h.h, 0, None)"], -1, ""),
    "groups_changed": (8, 5, OPEN + "h.set_groups(np.arange(fwfm_cases.N) % 7)", ["h.fmfm_predict(0, ROWS)"], -3, ""),
    "slots": (8, 5, OPEN + "h.adapt_begin()", ["h.fmfm_epoch(5)", "h.fmfm_evaluate(5)", "h.fmfm_predict(5, ROWS)",     # never uploaded;
                                               "h.fmfm_epoch(1)", "h.fmfm_evaluate(1)"], -3, ""),                     # without targets
    "sgda": (8, 5, "h.sgda_begin()", BEGIN, -3, "h.sgda_end()"),
    "als": (8, 5, "h.als_begin(0)", BEGIN, -3, "h.als_end()"),
    "fwfm_open": (8, 5, "h.fwfm_begin()", BEGIN, -3, "h.fwfm_end()"),
    "ffm_open": (8, 1, "h.ffm_begin(8)", BEGIN, -3, "h.ffm_end()"),
    "fmfm_open": (8, 5, OPEN, ["h.fwfm_begin()", "h.ffm_begin(8)"], -3, ""),
    "shard": (8, 0, "", BEGIN, -4, ""),
    "comm": (8, 0, "h.comm_init_rank(capi.comm_unique_id(), 0, 1)", BEGIN, -4, ""),
    "blocks": (8, 5, OPEN + "h.upload_block_rows(4, d.entries, d.row_ptr, d.target, [datagen.ragged_real(20, 4, 3, seed=62)[:2] + "
                         "(np.arange(ROWS) % 4, 580)], keep=True); h.adapt_begin()",
               ["h.fmfm_epoch(4)", "h.fmfm_predict(4, ROWS)"], -4, ""),
    "weights": (8, 5, OPEN + "h.set_row_weights(0, np.ones(ROWS)); h.adapt_begin()", ["h.fmfm_epoch(0)"], -4, "h.set_row_weights(0, None)"),
    "too_many_fields": (8, 65, "", BEGIN, -4, ""),
    "too_many_factors": (256, 0, "", BEGIN, -4, ""),
    "too_wide": (64, 33, "", BEGIN, -4, ""),                        # 64 x 33 = 2112 columns
}


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(oracle, what):
    """every refusal of include/fmx.h "fmx_fmfm_*"; the handle predicts afterwards"""
    import ctypes as C
    from libfm_amd import capi
    k, F, setup, calls, code, undo = REFUSALS[what]
    _, _, _, d = fwfm_cases.make(oracle, 8, 5)
    h = capi.Handle(fwfm_cases.N, k, learn_rate=LR, **(dict(shard_rank=0, shard_world=2) if what == "shard" else {}))
    scope = dict(globals(), h=h, d=d, C=C, capi=capi)
    try:
        if F:
            h.set_groups(np.arange(fwfm_cases.N) % F)
            h.upload_rows(0, d.entries, d.row_ptr, d.target)
            h.upload_rows(1, d.entries, d.row_ptr, None)
        exec(setup, scope)
        for call in calls:
            try:
                got = eval(call, scope)
                got = got if isinstance(got, int) else 0
            except capi.FmxError as e:
                got = e.code
            assert got == code, call
        exec(undo, scope)
        if F:
            assert np.isfinite(h.predict(0, ROWS)).all()           # the handle is usable
            if not what.startswith("too_"):
                h.fmfm_begin()
                assert np.isfinite(h.fmfm_predict(0, ROWS)).all()
    finally:
        h.close()
