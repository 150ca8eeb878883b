"""GPU: top-K retrieval (fmx_topk) against the fp64 oracle (tests/topk_oracle.py): bit-exact lists on dyadic data (ties
included) at every factor width and several forced split counts, tolerance checks on random and trained models, the existing
fmx_predict path on materialised joined rows, exclusion, edge cases, refusals, and the learner / CLI surface."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest

import datagen
import topk_oracle as T

pytestmark = pytest.mark.gpu
NONE = T.NONE


def handle(capi, n, k, w0, w, v, k0=True, k1=True, splits=None, **kw):
    old = os.environ.get("FMX_TOPK_SPLITS")
    if splits is not None:
        os.environ["FMX_TOPK_SPLITS"] = str(splits)
    try:
        h = capi.Handle(n, k, k0, k1, **kw)
    finally:
        if splits is not None:
            if old is None:
                del os.environ["FMX_TOPK_SPLITS"]
            else:
                os.environ["FMX_TOPK_SPLITS"] = old
    h.set_params(w0, w, v)
    return h


def dev_model(O, h, n, k, k0=True, k1=True):
    """the fp64 oracle model on the device's own fp32 parameters"""
    w0, w, v = h.get_params()
    m = O.Model(n, k, k0, k1)
    m.w0, m.w[:], m.v[:] = w0, w, np.asarray(v).reshape(k, n)
    return m


def dyadic_rows(rng, n, n_rows, max_nnz, dup_every=0, empty_every=0):
    ids, vals = [], []
    for r in range(n_rows):
        z = int(rng.integers(0, max_nnz + 1)) if not (empty_every and r % empty_every == 0) else 0
        ids.append([int(a) for a in rng.integers(0, n, z)])
        vals.append([float(a) for a in rng.choice([0.5, 1.0, -1.0], z)])
    if dup_every:                                    # duplicated candidate rows: equal scores, ties decided by the index
        for r in range(dup_every, n_rows, dup_every):
            ids[r], vals[r] = list(ids[r - dup_every]), list(vals[r - dup_every])
    return datagen._pack(ids, vals, np.zeros(n_rows))[:2]


def dyadic_model(rng, n, k):
    w0 = 0.375
    w = rng.integers(-8, 9, n) / 8.0
    v = rng.integers(-2, 3, (k, n)) / 4.0
    return w0, w, v


def tol(ref):
    return 1e-4 * np.abs(ref) + 1e-5


def check_lists(idx, sc, ref, K, exclude=None):
    """sorted, no duplicates, scores within tolerance of the oracle's, nothing clearly better left out"""
    Q, Cn = ref.shape
    for q in range(Q):
        ok = ~np.isnan(ref[q])
        if exclude is not None:
            ok[np.asarray(list(exclude[q]), dtype=np.int64)] = False
        n_ok = int(ok.sum())
        valid = idx[q] != NONE
        assert int(valid.sum()) == min(K, n_ok), q
        assert np.all(valid[:min(K, n_ok)])
        got = idx[q][valid].astype(np.int64)
        assert len(np.unique(got)) == len(got)
        assert ok[got].all()
        s = sc[q][valid]
        assert np.all(np.diff(s) <= 0), q
        r = ref[q, got]
        assert np.all(np.abs(s - r) <= tol(r)), (q, np.max(np.abs(s - r)))
        assert np.all(np.isneginf(sc[q][~valid]))
        if len(got) == K:
            kth = r.min()
            better = np.flatnonzero(ok & (ref[q] > kth + 2 * tol(kth)))
            assert np.isin(better, got).all(), q


@pytest.mark.parametrize("k", [1, 4, 16, 17, 64, 100, 1024])
def test_exact_dyadic_bit_equal(k, oracle):
    from libfm_amd import capi
    rng = np.random.default_rng(k)
    n = 300
    qe, qr = dyadic_rows(rng, n, 70, 4, empty_every=9)
    ce, cr = dyadic_rows(rng, n, 700, 4, dup_every=5, empty_every=13)
    w0, w, v = dyadic_model(rng, n, k)
    m = oracle.Model(n, k)
    m.w0, m.w[:], m.v[:] = w0, w, v
    ref = T.scores_decomposed(m, qe, qr, ce, cr)
    sel = {K: T.select(ref, K) for K in (1, 10, 100, 700, 1024)}
    for splits in (None, 1, 3, 64):
        h = handle(capi, n, k, w0, w, v, splits=splits)
        try:
            h.upload_rows(0, qe, qr, np.zeros(70, np.float32))
            h.upload_rows(1, ce, cr, np.zeros(700, np.float32))
            for K in ((1, 10, 100, 700, 1024) if splits is None else (10, 1024)):
                idx, sc = h.topk(0, 1, K)
                np.testing.assert_array_equal(idx, sel[K][0], err_msg="k=%d K=%d splits=%s" % (k, K, splits))
                np.testing.assert_array_equal(sc, sel[K][1])
        finally:
            h.close()


@pytest.mark.parametrize("k,K", [(0, 10), (1, 100), (8, 1024), (64, 10), (64, 100), (128, 1000), (1024, 10)])
def test_random_model_tolerance(k, K, oracle):
    from libfm_amd import capi
    rng = np.random.default_rng(100 + k)
    n = 2000
    qe, qr, _ = datagen.ragged_real(n, 150, 8, seed=k + 1, empty_every=17, duplicates=True)
    ce, cr, _ = datagen.ragged_real(n, 3001, 8, seed=k + 2, empty_every=23, duplicates=True)
    h = handle(capi, n, k, 0.1, rng.normal(0, 0.3, n), rng.normal(0, 0.2, (k, n)))
    try:
        h.upload_rows(0, qe, qr, np.zeros(150, np.float32))
        h.upload_rows(1, ce, cr, np.zeros(3001, np.float32))
        idx, sc = h.topk(0, 1, K)
        m = dev_model(oracle, h, n, k)
    finally:
        h.close()
    check_lists(idx, sc, T.scores_decomposed(m, qe, qr, ce, cr), K)


def test_large_candidate_set_sampled(oracle):
    """C = 2^20 + 3 (not a multiple of any tile), a sample of the queries checked"""
    from libfm_amd import capi
    n, k, C_, K = 5000, 64, (1 << 20) + 3, 100
    rng = np.random.default_rng(5)
    sizes = rng.integers(1, 4, C_)
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ce = np.zeros(int(rp[-1]), dtype=datagen.ENTRY_DTYPE)
    ce["id"] = rng.integers(0, n, len(ce))
    ce["value"] = rng.choice([1.0, 0.5], len(ce))
    qe, qr, _ = datagen.ragged_real(n, 200, 6, seed=9)
    h = handle(capi, n, k, 0.0, rng.normal(0, 0.3, n), rng.normal(0, 0.2, (k, n)))
    try:
        h.upload_rows(0, qe, qr, np.zeros(200, np.float32))
        h.upload_rows(1, ce, rp, np.zeros(C_, np.float32))
        idx, sc = h.topk(0, 1, K)
        m = dev_model(oracle, h, n, k)
    finally:
        h.close()
    sample = [0, 1, 77, 150, 199]
    check_lists(idx[sample], sc[sample], T.scores_decomposed(m, qe, qr, ce, rp, sample), K)


def _trained(kind, oracle):
    from libfm_amd import learner as L
    tr = datagen.movielens_shaped(60, 400, 6000, 21)
    fm = L.FMModel()
    fm.num_attribute, fm.num_factor = 460, 16
    fm.k0 = fm.k1 = True
    fm.w0, fm.w = 0.0, np.zeros(460)
    fm.v = np.random.default_rng(1).normal(0, 0.1, (16, 460))
    fm.reg0, fm.regw, fm.regv = 0.0, 0.01, 0.01
    data = L.Data(*tr)
    if kind == "sgd":
        l = L.FMLearnSGD()
        l.learn_rate, l.num_iter = 0.01, 5
    elif kind == "bpr":
        l = L.FMLearnPairSGD()
        l.learn_rate, l.num_iter, l.mode = 0.05, 3, "minibatch"
    else:
        l = L.FMLearnALS()
        l.num_iter, l.w_lambda, l.v_lambda = 3, 0.1, 0.1
        fm.w = np.random.default_rng(2).normal(0, 0.1, 460)
    l.fm, l.task, l.min_target, l.max_target = fm, 0, 1.0, 5.0
    l.out = io.StringIO()
    l.init()
    if kind == "bpr":
        y = tr[2]
        a, b = np.flatnonzero(y >= 4)[:500], np.flatnonzero(y <= 2)[:500]
        n_p = min(len(a), len(b))
        l.learn(data, (a[:n_p], b[:n_p]), data, (a[:n_p], b[:n_p]))
    else:
        l.learn(data, data)
    # queries: one row per user; candidates: one row per item
    users = L.Data(*datagen._pack([[u] for u in range(60)], [[1.0]] * 60, np.zeros(60)))
    items = L.Data(*datagen._pack([[60 + i] for i in range(400)], [[1.0]] * 400, np.zeros(400)))
    return l, users, items


@pytest.mark.parametrize("kind", ["sgd", "bpr", "als"])
def test_trained_models_and_recommend(kind, oracle):
    from libfm_amd import capi
    l, users, items = _trained(kind, oracle)
    try:
        ex = [list(range(u % 7)) + [5, 5] for u in range(60)]
        idx, sc = l.recommend(users, items, 20, ex)
        m = oracle.Model(460, 16)
        w0, w, v = l._h.get_params()
        m.w0, m.w[:], m.v[:] = w0, w, np.asarray(v).reshape(16, 460)
        ref = T.scores_decomposed(m, users.entries, users.row_ptr, items.entries, items.row_ptr)
        check_lists(idx, sc, ref, 20, ex)
        # the learner's call is Handle.topk on its slots
        if kind == "als":
            i2, s2 = l._h.topk(2, 3, 20, exclude=ex)
        else:
            i2, s2 = l._h.topk(l._slot(users), l._slot(items), 20, exclude=ex)
        np.testing.assert_array_equal(idx, i2)
        np.testing.assert_array_equal(sc, s2)
    finally:
        l.close()


def test_mcmc_recommend_raises():
    from libfm_amd import learner as L
    with pytest.raises(NotImplementedError):
        L.FMLearnMCMC().recommend(None, None, 10)


def test_matches_predict_on_joined_rows(oracle):
    from libfm_amd import capi
    n, k = 400, 32
    rng = np.random.default_rng(8)
    qe, qr, _ = datagen.ragged_real(n, 9, 6, seed=31, empty_every=4, duplicates=True)
    ce, cr, _ = datagen.ragged_real(n, 1000, 6, seed=32, empty_every=7, duplicates=True)
    h = handle(capi, n, k, -0.2, rng.normal(0, 0.3, n), rng.normal(0, 0.2, (k, n)))
    try:
        h.upload_rows(0, qe, qr, np.zeros(9, np.float32))
        h.upload_rows(1, ce, cr, np.zeros(1000, np.float32))
        idx, sc = h.topk(0, 1, 1000)
        je, jr = T.join_rows(qe, qr, ce, cr)
        h.upload_rows(2, je, jr, np.zeros(9000, np.float32))
        p = h.predict(2, 9000).reshape(9, 1000)
    finally:
        h.close()
    assert not (idx == NONE).any()
    check_lists(idx, sc, p, 1000)
    np.testing.assert_array_equal(np.sort(idx, axis=1), np.tile(np.arange(1000, dtype=np.uint32), (9, 1)))


def test_exclusion(oracle):
    from libfm_amd import capi
    n, k, Cn, K = 300, 8, 500, 50
    rng = np.random.default_rng(12)
    qe, qr, _ = datagen.ragged_real(n, 40, 5, seed=41)
    ce, cr, _ = datagen.ragged_real(n, Cn, 5, seed=42)
    ex = [list(rng.integers(0, Cn, int(rng.integers(0, 300)))) for _ in range(40)]
    ex[3] = []
    ex[5] = list(range(Cn))[::-1] + [0, 1]          # everything excluded: all padding
    ex[6] = list(range(Cn - 10))                    # fewer eligible than K
    h = handle(capi, n, k, 0.0, rng.normal(0, 0.3, n), rng.normal(0, 0.2, (k, n)))
    try:
        h.upload_rows(0, qe, qr, np.zeros(40, np.float32))
        h.upload_rows(1, ce, cr, np.zeros(Cn, np.float32))
        idx, sc = h.topk(0, 1, K, exclude=ex)
        m = dev_model(oracle, h, n, k)
    finally:
        h.close()
    for q in range(40):
        assert not np.isin(idx[q], np.asarray(ex[q], dtype=np.int64)).any()
    assert (idx[5] == NONE).all() and np.isneginf(sc[5]).all()
    assert (idx[6] != NONE).sum() == 10
    check_lists(idx, sc, T.scores_decomposed(m, qe, qr, ce, cr), K, ex)


def test_edge_cases_chunking_determinism(oracle):
    from libfm_amd import capi
    n, k = 200, 16
    rng = np.random.default_rng(13)
    qe, qr, _ = datagen.ragged_real(n, 150, 5, seed=51, empty_every=3, duplicates=True)
    ce, cr, _ = datagen.ragged_real(n, 900, 5, seed=52, empty_every=5, duplicates=True)
    w, v = rng.normal(0, 0.3, n), rng.normal(0, 0.2, (k, n))
    results = []
    for splits in (None, 1, 7):
        h = handle(capi, n, k, 0.25, w, v, splits=splits)
        try:
            h.upload_rows(0, qe, qr, np.zeros(150, np.float32))
            h.upload_rows(1, ce, cr, np.zeros(900, np.float32))
            one = h.topk(0, 1, 33)
            again = h.topk(0, 1, 33)
            np.testing.assert_array_equal(one[0], again[0])
            np.testing.assert_array_equal(one[1], again[1])
            parts = [h.topk(0, 1, 33, query_row0=r0, n_query=nq) for r0, nq in ((0, 1), (1, 64), (65, 70), (135, 15))]
            np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), one[0])
            np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), one[1])
            results.append(one)
            m = dev_model(oracle, h, n, k)
            # same slot, Q = 1
            i_s, s_s = h.topk(1, 1, 5, query_row0=4, n_query=1)
            check_lists(i_s, s_s, T.scores_decomposed(m, ce, cr, ce, cr, [4]), 5)
            # C < K and C = 1
            h.upload_rows(2, ce[:int(cr[3])], cr[:4], np.zeros(3, np.float32))
            h.upload_rows(3, ce[:int(cr[1])], cr[:2], np.zeros(1, np.float32))
            i3, s3 = h.topk(0, 2, 10)
            assert (i3[:, 3:] == NONE).all() and (i3[:, :3] != NONE).all()
            i1, s1 = h.topk(0, 3, 1)
            assert (i1 == 0).all()
            e0 = h.topk(0, 1, 4, n_query=0)
            assert e0[0].shape == (0, 4)
        finally:
            h.close()
        check_lists(one[0], one[1], T.scores_decomposed(m, qe, qr, ce, cr), 33)
    for r in results[1:]:
        np.testing.assert_array_equal(r[0], results[0][0])
        np.testing.assert_array_equal(r[1], results[0][1])


def test_refusals(oracle):
    from libfm_amd import capi
    n, k = 100, 8
    rng = np.random.default_rng(14)
    qe, qr, _ = datagen.ragged_real(n, 10, 4, seed=61)
    h = handle(capi, n, k, 0.0, rng.normal(0, 0.3, n), rng.normal(0, 0.2, (k, n)))
    try:
        h.upload_rows(0, qe, qr, np.zeros(10, np.float32))

        def code(*a, **kw):
            with pytest.raises(capi.FmxError) as ei:
                h.topk(*a, **kw)
            return ei.value.code
        assert code(0, 0, 0) == -1 and code(0, 0, 1025) == -1
        assert code(0, 0, 5, query_row0=8, n_query=3) == -1
        assert code(0, 5, 5) == -3                                        # never uploaded
        # an out-of-range exclusion index: FMX_E_ARG and the outputs untouched
        idx = np.full((10, 5), 7, dtype=np.uint32)
        sc = np.full((10, 5), 1.5)
        ptr = np.array([0] * 5 + [1] * 6, dtype=np.uint64)
        bad = np.array([10], dtype=np.uint32)
        opts = capi.TopkOpts(5, 0, 0, 10, 0, ptr.ctypes.data, bad.ctypes.data)
        assert h.lib.fmx_topk(h.h, 0, 0, C.byref(opts), idx.ctypes.data, sc.ctypes.data, None) == -1
        assert (idx == 7).all() and (sc == 1.5).all()
        # kept relation blocks
        be, br, _ = datagen.ragged_real(20, 4, 3, seed=62)
        h.upload_block_rows(4, qe, qr, np.zeros(10, np.float32), [(be, br, np.arange(10) % 4, 80)], keep=True)
        assert code(4, 0, 5) == -4 and code(0, 4, 5) == -4
        h.topk(0, 0, 5)                                                   # the handle stays usable
    finally:
        h.close()
    hs = capi.Handle(n, k, shard_rank=0, shard_world=2)
    try:
        hs.upload_rows(0, qe, qr, np.zeros(10, np.float32))
        with pytest.raises(capi.FmxError) as ei:
            hs.topk(0, 0, 5)
        assert ei.value.code == -4
    finally:
        hs.close()


def test_cli_topk_and_metrics(tmp_path, oracle):
    from libfm_amd import cli, ranking
    tr = datagen.movielens_shaped(30, 50, 1500, 71)
    te = datagen.movielens_shaped(30, 50, 60, 72)
    files = {}
    for tag, (ent, rp, y) in (("train", tr), ("test", te)):
        files[tag] = str(tmp_path / (tag + ".libfm"))
        oracle.Data(ent, rp, y).write_libsvm(files[tag])
    cand = datagen._pack([[30 + i] for i in range(50)], [[1.0]] * 50, np.zeros(50))
    files["cand"] = str(tmp_path / "cand.libfm")
    oracle.Data(*cand).write_libsvm(files["cand"])
    files["ex"] = str(tmp_path / "ex.txt")
    with open(files["ex"], "w") as f:
        f.write("0 3\n0 4\n2 0\n")
    out = str(tmp_path / "top.txt")
    model_f = str(tmp_path / "model")
    argv = ["-task", "r", "-method", "sgd", "-train", files["train"], "-test", files["test"], "-dim", "1,1,4", "-iter", "3",
            "-learn_rate", "0.01", "-seed", "3", "-save_model", model_f, "-topk", "7", "-candidates", files["cand"],
            "-exclude", files["ex"], "-topk_out", out]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(argv) == 0
    assert "Top-K\tqueries=60\tcandidates=50\tK=7" in buf.getvalue()
    lines = open(out).read().splitlines()
    assert len(lines) == 60
    got = [[int(t.split(":")[0]) for t in ln.split()] for ln in lines]
    assert all(len(g) == 7 for g in got) and not ({3, 4} & set(got[0])) and 0 not in got[2]
    # the lists from the saved model through the oracle
    from libfm_amd import learner as L
    fm = L.FMModel()
    fm.num_attribute, fm.num_factor = 80, 4
    fm.k0 = fm.k1 = True
    fm.w0, fm.w, fm.v = 0.0, np.zeros(80), np.zeros((4, 80))
    assert fm.load_model(model_f)
    m = oracle.Model(80, 4)
    m.w0, m.w[:], m.v[:] = fm.w0, fm.w, fm.v
    ex = [[3, 4], [], [0]] + [[] for _ in range(57)]
    ridx, rsc = T.select(T.scores_decomposed(m, te[0], te[1], cand[0], cand[1]), 7, ex)
    for q in range(60):
        s = np.array([float(t.split(":")[1]) for t in lines[q].split()])
        np.testing.assert_allclose(s, rsc[q], rtol=1e-4, atol=1e-4)
    # ranking.metrics on device lists equals the metrics on oracle lists (exact arithmetic)
    rng = np.random.default_rng(3)
    qe, qr = dyadic_rows(rng, 200, 40, 3)
    ce, cr = dyadic_rows(rng, 200, 300, 3, dup_every=4)
    w0, w, v = dyadic_model(rng, 200, 8)
    mm = oracle.Model(200, 8)
    mm.w0, mm.w[:], mm.v[:] = w0, w, v
    from libfm_amd import capi
    h = handle(capi, 200, 8, w0, w, v)
    try:
        h.upload_rows(0, qe, qr, np.zeros(40, np.float32))
        h.upload_rows(1, ce, cr, np.zeros(300, np.float32))
        idx, _ = h.topk(0, 1, 10)
    finally:
        h.close()
    ridx, _ = T.select(T.scores_decomposed(mm, qe, qr, ce, cr), 10)
    rel_ptr = np.arange(0, 41 * 5, 5)
    rel_idx = rng.integers(0, 300, 200)
    assert ranking.metrics(idx, rel_ptr, rel_idx) == ranking.metrics(ridx, rel_ptr, rel_idx)
