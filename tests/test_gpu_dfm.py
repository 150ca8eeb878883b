"""GPU: DeepFM with one hidden layer (fmx_dfm_*: k_fmfm_sums<KP, true> / k_dfm_gemm_h / k_dfm_gemm_z / k_fmfm_apply_seg / k_dfm_wgrad /
k_dfm_netstep) against its float64 restatement libfm_amd/dfm.py (itself pinned to a brute-force loop and to finite differences in
tests/test_dfm_cpu.py, which also holds every training case below to the kink condition).

Tolerances are tests/test_gpu_adagrad.py's: w0, w, v, the net and predictions at rtol 1e-4 / atol 2e-5, the accumulators at rtol 1e-4.
Four times the deviation of the restatement run in fp32 (numpy) from itself in fp64 on the same cases stays below 0.06 of every one of
them (the worst: n_v on the 2 233 rows, 1.4e-6 relative), so none is widened; the figures are in DESIGN.md section 33."""
import numpy as np
import pytest

import dfm_cases
from dfm_cases import ETA, LR, ROWS_T

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5


def open_handle(capi, m, groups, H, task=0, net=None, adagrad=False):
    h = capi.Handle(m.n, m.k, m.k0, m.k1, task, m.reg0, m.regw, m.regv, LR, -1.0, 1.0)
    h.set_params(m.w0, m.w, m.v)
    h.set_groups(groups)
    if adagrad:
        h.adapt_begin("adagrad", 1.0, ETA)
    h.dfm_begin(H)
    if net is not None:
        h.dfm_set_net(*net)
    return h


def state_of(h, n):
    net, acc = h.dfm_get_net()
    return h.get_params() + h.adapt_state_rows(np.arange(n, dtype=np.uint32)) + net + acc


@pytest.mark.parametrize("k, F, H", [(1, 1, 1), (4, 3, 8), (5, 17, 24), (8, 8, 64), (3, 33, 80), (4, 39, 200)])
def test_predict(oracle, k, F, H):
    """WP = 16, 16, 144 (off a multiple of 64), 64, 144, 160; H = 1, one column tile exactly, 80 across one tile, 200 over four"""
    from libfm_amd import capi, dfm
    m, groups, net, d = dfm_cases.make(oracle, k, F, H)
    h = open_handle(capi, m, groups, H, net=net)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        ref = dfm.predict(m, net, groups, d)
        np.testing.assert_allclose(h.dfm_predict(0, d.n_rows), ref, rtol=RTOL, atol=ATOL)
        assert abs(h.dfm_evaluate(0).rmse - np.sqrt(np.mean((np.clip(ref, -1, 1) - d.target) ** 2))) < 1e-4
    finally:
        h.close()


@pytest.mark.parametrize("case", dfm_cases.TRAIN)
def test_training(oracle, case):
    """three epochs; batch 202 of 503 rows: segments of several occurrences; 2 233 rows in one batch: partials 0 and 1 of k_dfm_wgrad
    walk three chunks"""
    from libfm_amd import capi, dfm
    k, F, H, batch, task, rows = case
    m0, groups, net0, d = dfm_cases.make(oracle, k, F, H, task, rows)
    m, st, net, n_net, _, _, _ = dfm_cases.train_reference(oracle, case)
    h = open_handle(capi, m0, groups, H, task, net0, adagrad=True)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        for _ in range(3):
            es = h.dfm_epoch(0, batch, 16)
        assert es.rows == rows and es.batches == (1 if batch == 0 else -(-rows // batch))
        w0, w, v, nw, nv, W1, b1, w2, nW1, nb1, nw2 = state_of(h, m.n)
        pred = h.dfm_predict(0, rows)
    finally:
        h.close()
    for got, ref in ((v, m.v), (w, m.w), (w0, m.w0), (W1, net[0]), (b1, net[1]), (w2, net[2]), (pred, dfm.predict(m, net, groups, d))):
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
    for got, ref in ((nv, st.n_v), (nw, st.n_w), (nW1, n_net[0]), (nb1, n_net[1]), (nw2, n_net[2])):
        np.testing.assert_allclose(got, ref, rtol=RTOL)
    assert np.abs(m.v - m0.v).max() > 1e-3 and np.abs(net[0] - net0[0]).max() > 1e-3        # (moved far beyond the tolerances)


def test_zero_net_bits_untouched_features_and_padding(oracle):
    """a zero net trains as fmx_adapt_epoch does and stays exactly zero; a random net twice gives identical bits, leaves the features no
    row names alone and V's padding (k = 5 in rows of 8 floats) zero: fmx_predict sums over it"""
    from libfm_amd import capi
    k, F, H = 5, 17, 24
    m, groups, net, d = dfm_cases.make(oracle, k, F, H, 1, ROWS_T)
    touched = np.isin(np.arange(m.n), d.entries["id"])
    res = []
    for which in ("adapt", "zero", "net", "net"):
        h = open_handle(capi, m, groups, H, 1, net if which == "net" else None, adagrad=True)
        try:
            h.upload_rows(0, d.entries, d.row_ptr, d.target)
            start = state_of(h, m.n)
            for _ in range(2):
                (h.adapt_epoch if which == "adapt" else h.dfm_epoch)(0, 202, 16)
            res.append(state_of(h, m.n))
            plain = h.predict(0, d.n_rows)
        finally:
            h.close()
    for a, b in zip(res[0][:5], res[1][:5]):
        np.testing.assert_allclose(b, a, rtol=RTOL, atol=ATOL)
    assert all(not a.any() for a in res[1][5:8]) and all((a == 1.0).all() for a in res[1][8:])
    assert all(np.array_equal(a, b) for a, b in zip(res[2], res[3]))
    w0, w, v, nw, nv = res[3][:5]
    assert not touched.all() and not np.array_equal(v[:, touched], start[2][:, touched])
    for got, was in ((w, start[1]), (nw, start[3]), (v.T, start[2].T), (nv.T, start[4].T)):
        assert np.array_equal(got[~touched], was[~touched])
    after = m.copy()
    after.w0, after.w[:], after.v[:] = w0, w, v
    np.testing.assert_allclose(plain, oracle.predict_raw(after, d), rtol=RTOL, atol=ATOL)


OPTS = ["8, 0.0, 0.0, 0.0, 1"] + ["8, %s0" % "".join(bad + ", " if j == i else "0.0, " for j in range(3))
                                  for bad in ("-1.0", "float('nan')", "float('inf')") for i in range(3)]
BEGIN, OPEN = ["h.dfm_begin(8)"], "h.dfm_begin(8); "
NAN_NET = "np.full((40, 8), np.nan), np.zeros(8), np.zeros(8)"
# what: (factors, fields (0: a bare handle, no rows), set-up, the calls that are refused, their code, what undoes the set-up)
REFUSALS = {
    "no_session": (8, 5, "", ["h.dfm_epoch(0)", "h.dfm_predict(0, ROWS)", "h.dfm_evaluate(0)", "h.lib.fmx_dfm_get_net(h.h, *[None] * 6)",
                              "h.lib.fmx_dfm_set_net(h.h, P, P, P)", "h.dfm_end()"], -3, ""),
    "no_adagrad": (8, 5, OPEN, ["h.dfm_epoch(0)"], -3, ""),
    "bad_opts": (8, 5, "", ["h.lib.fmx_dfm_begin(h.h, None)"] + ["h.lib.fmx_dfm_begin(h.h, C.byref(capi.DfmOpts(%s)))" % o for o in OPTS], -1, ""),
    "bad_net": (8, 5, OPEN, ["h.dfm_set_net(%s)" % NAN_NET, "h.lib.fmx_dfm_set_net(h.h, P, None, P)"], -1, ""),
    "null_pointers": (8, 5, OPEN, ["h.lib.fmx_dfm_predict(h.h, 0, None)", "h.lib.fmx_dfm_evaluate(h.h, 0, None)"], -1, ""),
    "hidden": (8, 5, "", ["h.dfm_begin(0)", "h.dfm_begin(513)"], -4, ""),
    "groups_changed": (8, 5, OPEN + "h.set_groups(np.arange(dfm_cases.N) % 7)", ["h.dfm_predict(0, ROWS)"], -3, ""),
    "slots": (8, 5, OPEN + "h.adapt_begin()", ["h.dfm_epoch(5)", "h.dfm_evaluate(5)", "h.dfm_predict(5, ROWS)",       # never uploaded;
                                               "h.dfm_epoch(1)", "h.dfm_evaluate(1)"], -3, ""),                       # without targets
    **{s + "_open": (8, 1 if s == "ffm" else 5, "h.%s_begin(%s)" % (s, a), BEGIN, -3, "h.%s_end()" % s)
       for s, a in (("sgda", ""), ("als", "0"), ("fwfm", ""), ("ffm", "8"), ("fmfm", ""), ("hofm", "3"))},
    "dfm_open": (8, 1, OPEN, ["h.fwfm_begin()", "h.ffm_begin(8)", "h.fmfm_begin()", "h.hofm_begin(3)"], -3, ""),
    "shard": (8, 0, "", BEGIN, -4, ""),
    "comm": (8, 0, "h.comm_init_rank(capi.comm_unique_id(), 0, 1)", BEGIN, -4, ""),
    "blocks": (8, 5, OPEN + "h.upload_block_rows(4, d.entries, d.row_ptr, d.target, [datagen.ragged_real(20, 4, 3, seed=62)[:2] + "
                      "(np.arange(ROWS) % 4, 580)], keep=True); h.adapt_begin()", ["h.dfm_epoch(4)", "h.dfm_predict(4, ROWS)"], -4, ""),
    "weights": (8, 5, OPEN + "h.set_row_weights(0, np.ones(ROWS)); h.adapt_begin()", ["h.dfm_epoch(0)"], -4, "h.set_row_weights(0, None)"),
    "too_many_fields": (8, 65, "", BEGIN, -4, ""),
    "too_many_factors": (256, 0, "", BEGIN, -4, ""),
    "too_wide": (64, 33, "", BEGIN, -4, ""),                        # 64 x 33 = 2112 columns
}


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(oracle, what):
    """every refusal of include/fmx.h "fmx_dfm_*", once; the handle predicts afterwards"""
    import ctypes as C
    import datagen
    from libfm_amd import capi
    k, F, setup, calls, code, undo = REFUSALS[what]
    _, _, _, d = dfm_cases.make(oracle, 8, 5, 8)
    h = capi.Handle(dfm_cases.N, k, learn_rate=LR, **(dict(shard_rank=0, shard_world=2) if what == "shard" else {}))
    scope = dict(h=h, d=d, C=C, capi=capi, np=np, datagen=datagen, dfm_cases=dfm_cases, ROWS=d.n_rows, P=np.zeros(400).ctypes.data)
    try:
        if F:
            h.set_groups(np.arange(dfm_cases.N) % F)
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
            assert np.isfinite(h.predict(0, d.n_rows)).all()       # the handle is usable
            if not what.startswith("too_"):
                h.dfm_begin(8)
                assert np.isfinite(h.dfm_predict(0, d.n_rows)).all()
    finally:
        h.close()


def test_learner_and_cli(oracle, tmp_path):
    """three iterations of `-model dfm -hidden 8` and of the learner with model="dfm" end at the net the restatement, driven the same way
    from the same start net, ends at"""
    from libfm_amd import adaptive, cli, dfm, learner as L
    from libfm_amd import refrand as R
    (_, groups, _, d), k, F, H = dfm_cases.make(oracle, 4, 5, 8, 1), 4, 5, 8
    trf, meta, nout = str(tmp_path / "tr.libfm"), str(tmp_path / "meta"), str(tmp_path / "net.txt")
    d.write_libsvm(trf)
    n, reg = d.num_feature, (0.01, 0.002, 0.001)
    np.savetxt(meta, groups[:n], fmt="%d")
    assert cli.main(["-task", "c", "-train", trf, "-test", trf, "-dim", "1,1,%d" % k, "-iter", "3", "-method", "sgd", "-learn_rate", "0.05",
                     "-regular", "%g,%g,%g" % reg, "-init_stdev", "0.1", "-seed", "46", "-optimizer", "adagrad", "-batch", "64",
                     "-w0_chunk", "16", "-model", "dfm", "-meta", meta, "-hidden", str(H), "-net_out", nout]) == 0
    m = oracle.Model(n, k, True, True, *reg)
    R.srand(46)
    m.v[:] = R.init_v(k, n, 0.0, 0.1)
    l = L.FMLearnSGD()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor, (l.fm.reg0, l.fm.regw, l.fm.regv) = n, k, reg
    l.fm.w0, l.fm.w, l.fm.v = 0.0, np.zeros(n), m.v.copy()
    l.task, l.num_iter, l.learn_rate, l.batch, l.w0_chunk, l.min_target, l.max_target = 1, 3, 0.05, 64, 16, -1.0, 1.0
    l.optimizer, l.model, l.groups, l.num_hidden, l.seed, l.out = "adagrad", "dfm", groups[:n], H, 46, open(str(tmp_path / "log"), "w")
    rng = np.random.default_rng(46)                                 # the learner's draw: W1, b1, w2 in this order
    net = tuple(rng.normal(0.0, 0.1, size=shape) for shape in ((F * k, H), H, H))
    st, n_net, start = adaptive.AdaptState(n, k, 1.0), tuple(np.ones_like(a) for a in net), net[0].copy()
    closest = min(dfm.epoch(m, st, net, n_net, groups[:n], d, 1, 0.05, -1.0, 1.0, 64, 16) for _ in range(3))
    assert closest >= 1e-4 and np.abs(net[0] - start).max() > 1e-3
    text = np.loadtxt(nout)                                         # b1, w2, then the rows of W1; 6 significant digits
    np.testing.assert_allclose(text, np.vstack([net[1], net[2], net[0]]), rtol=RTOL, atol=ATOL)
    data = L.Data(d.entries, d.row_ptr, d.target)
    try:
        l.init()
        l.learn(data, data)
        for got, ref in zip(l.net, net):
            np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(l.predict_raw(data), dfm.predict(m, net, groups[:n], d), rtol=RTOL, atol=ATOL)
        with pytest.raises(NotImplementedError):
            l.evaluate_ex(data)
    finally:
        l.close()
