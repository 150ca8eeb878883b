"""GPU: pairwise ranking (BPR) around fm_pairSGD -- fmx_upload_pairs / fmx_pair_epoch / fmx_pair_evaluate.

FMX_SGD_SEQUENTIAL against the real reference (tests/golden/bpr_*.npz), FMX_SGD_MINIBATCH against the fp64 batch rule of
tests/bpr_oracle.py, the pair metrics, edge cases, the refusals, the other entry points on the trained handle, and the CLI.
Tolerances as tests/test_gpu_sequential.py: |gpu - ref| <= 1e-4 |ref| + 1e-5 on w and V, w0 to 1e-12 relative."""
import contextlib
import io
import os

import numpy as np
import pytest

import bpr_oracle as B
import datagen
from conftest import GOLDEN_DIR, golden_cases

pytestmark = pytest.mark.gpu

CASES = [c for c in golden_cases() if c.startswith("bpr_")]
RTOL, ATOL = 1e-4, 1e-5


def close(gpu, ref, what=""):
    err = np.abs(np.asarray(gpu) - np.asarray(ref))
    bound = RTOL * np.abs(ref) + ATOL
    assert (err <= bound).all(), "%s: max excess %g" % (what, float((err - bound).max()))


def w0_close(gpu, ref):
    assert abs(gpu - ref) <= 1e-12 * max(abs(ref), 1e-300) or gpu == ref, (gpu, ref)


def model(O, n, k, k0, k1, reg, w0, w, v, f32=True):
    m = O.Model(n, k, k0, k1, *reg)
    m.w0 = float(w0)
    m.w[:] = np.asarray(w, np.float32) if f32 else w
    m.v[:] = np.asarray(v, np.float32) if f32 else v
    return m


def handle(capi, n, k, k0, k1, reg, lr, m):
    h = capi.Handle(n, k, k0, k1, capi.TASK_REGRESSION, *reg, lr, 1.0, 5.0, device=0)
    h.set_params(m.w0, m.w, m.v)
    return h


def check_params(h, m, what):
    w0, w, v = h.get_params()
    close(w, m.w, what + " w")
    close(v, m.v, what + " v")
    w0_close(w0, m.w0)


@pytest.mark.parametrize("name", CASES)
def test_sequential_matches_reference(name, oracle):
    from libfm_amd import capi
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    n, k, k0, k1, lr, reg = int(z["n"]), int(z["k"]), bool(z["k0"]), bool(z["k1"]), float(z["lr"]), [float(x) for x in z["reg"]]
    m = model(oracle, n, k, k0, k1, reg, z["init_w0"], z["init_w"], z["init_v"], f32=False)
    h = handle(capi, n, k, k0, k1, reg, lr, m)
    P = len(z["pair_a"])
    h.upload_rows(0, z["train_entries"], z["train_row_ptr"], np.zeros(len(z["train_row_ptr"]) - 1, np.float32))
    h.upload_pairs(0, z["pair_a"], z["pair_b"])
    for it in range(int(z["iters"])):
        st = h.pair_epoch(0, capi.SGD_SEQUENTIAL)
        assert st.rows == P and st.batches == P
        if it == 0:
            check_params(h, model(oracle, n, k, k0, k1, reg, z["epoch1_w0"], z["epoch1_w"], z["epoch1_v"], f32=False), name + " epoch 1")
    check_params(h, model(oracle, n, k, k0, k1, reg, z["final_w0"], z["final_w"], z["final_v"], f32=False), name + " final")
    h.upload_rows(1, z["test_entries"], z["test_row_ptr"], None)
    p = h.predict(1, len(z["test_row_ptr"]) - 1)
    np.testing.assert_allclose(p, z["test_pred"], rtol=5e-5, atol=5e-5)
    h.close()


def rows_and_pairs(n, n_rows, n_pairs, max_nnz, seed, dup=True, empty_every=0):
    ent, rp, _ = datagen.ragged_real(n, n_rows, max_nnz, seed, duplicates=dup, empty_every=empty_every)
    rng = np.random.default_rng(seed + 7)
    return ent, rp, rng.integers(0, n_rows, n_pairs).astype(np.uint32), rng.integers(0, n_rows, n_pairs).astype(np.uint32)


def start_model(O, n, k, k0=True, k1=True, reg=(0.01, 0.01, 0.02), seed=3):
    rng = np.random.default_rng(seed)
    return model(O, n, k, k0, k1, reg, 0.25, rng.normal(0, 0.1, n), rng.normal(0, 0.1, (k, n)))


def run_both(capi, O, ent, rp, pa, pb, k, lr, mode, batch, n, m0, epochs=1):
    """device and oracle from the same fp32-exact start; returns (handle, oracle model)"""
    h = handle(capi, n, k, m0.k0, m0.k1, (m0.reg0, m0.regw, m0.regv), lr, m0)
    h.upload_rows(0, ent, rp, np.zeros(len(rp) - 1, np.float32))
    h.upload_pairs(0, pa, pb)
    ref = m0.copy()
    for _ in range(epochs):
        st = h.pair_epoch(0, mode, batch)
        if mode == capi.SGD_SEQUENTIAL:
            B.pair_epoch_loop(ref, ent, rp, pa, pb, lr)
        else:
            B.pair_epoch_batch(ref, ent, rp, pa, pb, lr, batch)
            assert st.batch_used == batch and st.batches == (len(pa) + batch - 1) // batch and st.max_feature_count >= 1
    return h, ref


@pytest.mark.parametrize("batch", [1, 7, 64, 600])
def test_minibatch_matches_batch_rule(batch, oracle):
    from libfm_amd import capi
    n, k, lr = 50, 8, 0.05
    ent, rp, pa, pb = rows_and_pairs(n, 150, 500, 9, 31)
    m0 = start_model(oracle, n, k)
    h, ref = run_both(capi, oracle, ent, rp, pa, pb, k, lr, capi.SGD_MINIBATCH, batch, n, m0)
    check_params(h, ref, "batch %d" % batch)
    if batch == 1:                                       # B = 1 is the loop: the same numbers as FMX_SGD_SEQUENTIAL
        hs, _ = run_both(capi, oracle, ent, rp, pa, pb, k, lr, capi.SGD_SEQUENTIAL, 1, n, m0)
        _, w1, v1 = h.get_params()
        _, ws, vs = hs.get_params()
        close(w1, ws, "B=1 vs sequential w")
        close(v1, vs, "B=1 vs sequential v")
        hs.close()
    h.close()


def test_minibatch_is_deterministic(oracle):
    from libfm_amd import capi
    n, k, lr = 300, 64, 0.05
    ent, rp, pa, pb = rows_and_pairs(n, 2000, 6000, 12, 41)
    m0 = start_model(oracle, n, k)
    out = []
    for _ in range(2):
        h = handle(capi, n, k, True, True, (0.0, 0.01, 0.02), lr, m0)
        h.upload_rows(0, ent, rp, np.zeros(len(rp) - 1, np.float32))
        h.upload_pairs(0, pa, pb)
        for _ in range(2):
            h.pair_epoch(0, capi.SGD_MINIBATCH, 64)
        out.append(h.get_params())
        h.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def test_pair_evaluate_matches_numpy(oracle):
    from libfm_amd import capi
    n, k = 80, 16
    ent, rp, pa, pb = rows_and_pairs(n, 300, 3000, 10, 51)
    m0 = start_model(oracle, n, k)
    h = handle(capi, n, k, True, True, (0.0, 0.0, 0.0), 0.05, m0)
    h.upload_rows(0, ent, rp, np.zeros(len(rp) - 1, np.float32))
    h.upload_pairs(0, pa, pb)
    h.pair_epoch(0, capi.SGD_MINIBATCH, 128)
    w0, w, v = h.get_params()
    cur = model(oracle, n, k, True, True, (0.0, 0.0, 0.0), w0, w, v)
    d = B.pair_d(cur, ent, rp, pa, pb)
    ev = h.pair_evaluate(0)
    assert ev.pairs == len(pa)
    ok = np.abs(d) >= 1e-6
    assert abs(ev.accuracy * len(pa) - (d > 0).sum()) <= (~ok).sum()
    acc, loss = B.pair_metrics(d)
    assert abs(ev.loss - loss) <= 1e-5 * loss
    assert h.pair_evaluate(0).loss == ev.loss                  # a fixed-order reduction
    h.close()


@pytest.mark.parametrize("k", [1, 5, 64, 128, 1000])
def test_edge_cases_both_modes(k, oracle):
    """a pair with a == b, empty rows, ids repeated inside a row and shared by both rows, at k from 1 to 1000"""
    from libfm_amd import capi
    n, lr = 40, 0.05
    n_pairs = 60 if k >= 128 else 200
    ent, rp, pa, pb = rows_and_pairs(n, 80, n_pairs, 8, 61 + k, empty_every=9)
    pa[3] = pb[3] = 5                                         # a == b
    pa[4], pb[4] = 8, 17                                      # both empty (empty_every = 9)
    pa[5], pb[5] = 8, 2
    m0 = start_model(oracle, n, k, seed=k)
    for mode, batch in ((capi.SGD_SEQUENTIAL, 1), (capi.SGD_MINIBATCH, 7)):
        h, ref = run_both(capi, oracle, ent, rp, pa, pb, k, lr, mode, batch, n, m0)
        check_params(h, ref, "k %d mode %d" % (k, mode))
        h.close()


def test_one_feature_in_every_pair_of_a_4096_batch(oracle):
    from libfm_amd import capi
    n, k, lr, P = 400, 8, 0.001, 4096
    rng = np.random.default_rng(71)
    ids, vals = [], []
    for r in range(600):                                       # feature 0 in every row, then two random ones
        ids.append([0] + rng.integers(1, n, 2).tolist())
        vals.append([1.0] + rng.uniform(-1, 1, 2).round(3).tolist())
    ent, rp, _ = datagen._pack(ids, vals, [0.0] * len(ids))
    pa = rng.integers(0, 600, P).astype(np.uint32)
    pb = rng.integers(0, 600, P).astype(np.uint32)
    m0 = start_model(oracle, n, k)
    h, ref = run_both(capi, oracle, ent, rp, pa, pb, k, lr, capi.SGD_MINIBATCH, P, n, m0)
    check_params(h, ref, "4096-pair batch")
    st = h.pair_epoch(0, capi.SGD_MINIBATCH, P)
    assert st.max_feature_count == 2 * P                      # feature 0: one entry in each row of each pair
    h.close()


def test_refusals_leave_the_handle_usable(oracle):
    from libfm_amd import capi
    n, k, lr = 50, 4, 0.05
    ent, rp, pa, pb = rows_and_pairs(n, 60, 100, 6, 81, dup=False)
    m0 = start_model(oracle, n, k)
    h = handle(capi, n, k, True, True, (m0.reg0, m0.regw, m0.regv), lr, m0)
    y = np.linspace(1, 5, len(rp) - 1).astype(np.float32)
    h.upload_rows(0, ent, rp, y)

    def code(fn, *a):
        with pytest.raises(capi.FmxError) as e:
            fn(*a)
        return e.value.code

    assert code(h.pair_epoch, 0, capi.SGD_SEQUENTIAL) == -3              # no pairs yet
    assert code(h.pair_evaluate, 0) == -3
    bad = pa.copy()
    bad[7] = len(rp) - 1                                                 # a row outside the slot: nothing changes
    assert code(h.upload_pairs, 0, bad, pb) == -1
    assert code(h.pair_epoch, 0, capi.SGD_SEQUENTIAL) == -3
    h.upload_pairs(0, pa, pb)
    assert code(h.pair_epoch, 0, capi.SGD_HOGWILD) == -4
    h.als_begin(0)
    assert code(h.pair_epoch, 0, capi.SGD_MINIBATCH) == -3               # open ALS session on the slot
    h.als_end()
    h.sgda_begin()
    assert code(h.pair_epoch, 0, capi.SGD_SEQUENTIAL) == -3              # open SGDA session
    h.sgda_end()
    h.set_params(m0.w0, m0.w, m0.v)
    blk_ent = np.zeros(1, dtype=ent.dtype)
    blk_ent["id"], blk_ent["value"] = 0, 1.0                             # one block row holding attribute n - 1
    h.upload_block_rows(1, ent, rp, y, [(blk_ent, np.array([0, 1], np.uint64), np.zeros(len(rp) - 1, np.uint32), n - 1)], keep=True)
    h.upload_pairs(1, pa, pb)
    assert code(h.pair_epoch, 1, capi.SGD_SEQUENTIAL) == -4              # kept -relation blocks
    h.free_rows(1)
    h.upload_rows(2, ent, rp, y)
    h.upload_pairs(2, pa, pb)
    h.free_rows(2)
    assert code(h.pair_epoch, 2, capi.SGD_SEQUENTIAL) == -3              # fmx_free_rows dropped the pairs (and the rows)
    h.upload_rows(2, ent, rp, y)
    h.upload_pairs(2, pa, pb)
    h.upload_rows(2, ent, rp, y)
    assert code(h.pair_epoch, 2, capi.SGD_SEQUENTIAL) == -3              # a new upload dropped them
    ref = m0.copy()
    h.pair_epoch(0, capi.SGD_SEQUENTIAL)                                 # ... and the handle still trains
    B.pair_epoch_loop(ref, ent, rp, pa, pb, lr)
    check_params(h, ref, "after refusals")
    h.close()
    s = capi.Handle(n, k, True, True, capi.TASK_REGRESSION, 0.0, 0.01, 0.01, lr, 1.0, 5.0, device=0, shard_rank=0, shard_world=2)
    s.set_params(m0.w0, m0.w, m0.v)
    s.upload_rows(0, ent, rp, y)
    s.upload_pairs(0, pa, pb)
    assert code(s.pair_epoch, 0, capi.SGD_SEQUENTIAL) == -4              # feature shard
    assert code(s.pair_evaluate, 0) == -4
    s.close()


def test_other_entry_points_after_pair_epochs(oracle):
    from libfm_amd import capi
    n, k, lr = 60, 8, 0.05
    ent, rp, pa, pb = rows_and_pairs(n, 120, 300, 8, 91)
    y = np.random.default_rng(5).integers(1, 6, len(rp) - 1).astype(np.float32)
    m0 = start_model(oracle, n, k)
    h = handle(capi, n, k, True, True, (0.0, 0.01, 0.02), lr, m0)
    h.upload_rows(0, ent, rp, y)
    h.upload_pairs(0, pa, pb)
    h.pair_epoch(0, capi.SGD_SEQUENTIAL)
    h.pair_epoch(0, capi.SGD_MINIBATCH, 16)
    w0, w, v = h.get_params()
    ref = model(oracle, n, k, True, True, (0.0, 0.01, 0.02), w0, w, v)
    d = oracle.Data(ent, rp, y)
    np.testing.assert_allclose(h.predict(0, len(y)), oracle.predict_raw(ref, d), rtol=5e-5, atol=5e-5)
    rmse, mae = oracle.evaluate(ref, d, 0, 1.0, 5.0)
    ev = h.evaluate(0)
    assert abs(ev.rmse - rmse) <= 1e-4 * rmse and abs(ev.mae - mae) <= 1e-4 * mae
    h.sgd_epoch(0, capi.SGD_SEQUENTIAL)
    oracle.sgd_epoch_online(ref, d, 0, lr, 1.0, 5.0)
    w0g, wg, vg = h.get_params()
    close(wg, ref.w, "sgd after pairs w")
    close(vg, ref.v, "sgd after pairs v")
    assert abs(w0g - ref.w0) <= 1e-4 * abs(ref.w0) + 1e-6
    h.close()


def test_cli_bpr_end_to_end(tmp_path, oracle):
    """MovieLens-shaped rows from a planted model; of two rated items of one user the higher-rated row is row a"""
    from libfm_amd import cli

    def pairs_of(ent, rp, y, n_users, rng, per_user):
        users = ent["id"][rp[:-1].astype(np.int64)]
        a, b = [], []
        for u in range(n_users):
            rows = np.flatnonzero(users == u)
            if len(rows) < 2:
                continue
            for _ in range(per_user):
                r, s = rng.choice(rows, 2, replace=False)
                if y[r] != y[s]:
                    a.append(r if y[r] > y[s] else s)
                    b.append(s if y[r] > y[s] else r)
        return np.array(a), np.array(b)

    rng = np.random.default_rng(3)
    nu, ni = 60, 40
    tr = datagen.movielens_shaped(nu, ni, 3000, 111, noise=0.1)
    te = datagen.movielens_shaped(nu, ni, 500, 112, noise=0.1)
    files = {}
    for tag, (ent, rp, y) in (("train", tr), ("test", te)):
        files[tag] = str(tmp_path / (tag + ".libfm"))
        oracle.Data(ent, rp, y).write_libsvm(files[tag])
        a, b = pairs_of(ent, rp, y, nu, rng, 40)
        files[tag + "_pairs"] = str(tmp_path / (tag + ".pairs"))
        with open(files[tag + "_pairs"], "w") as f:
            f.write("".join("%d %d\n" % (x, z) for x, z in zip(a, b)))
    out, model_f = str(tmp_path / "pred"), str(tmp_path / "model")
    argv = ["-method", "bpr", "-train", files["train"], "-test", files["test"], "-train_pairs", files["train_pairs"],
            "-test_pairs", files["test_pairs"], "-dim", "1,1,8", "-iter", "30", "-learn_rate", "0.05", "-regular", "0,0,0.001",
            "-init_stdev", "0.1", "-seed", "7", "-out", out, "-save_model", model_f]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(argv) == 0
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("#Iter=")]
    assert len(lines) == 30, buf.getvalue()[-2000:]
    train_acc = float(lines[-1].split("\t")[1].split("=")[1])
    assert train_acc > 0.8, lines[-1]
    assert len(np.loadtxt(out)) == len(te[1]) - 1
    assert open(model_f).readline().strip() == "#global bias W0"


def test_sequential_pairs_longer_than_the_lds(oracle):
    """pairs of more than 2048 entries are merged in a global buffer instead of LDS"""
    from libfm_amd import capi
    n, k, lr = 3000, 8, 0.01
    rng = np.random.default_rng(121)
    ids = [rng.choice(n, 1500, replace=False).tolist() for _ in range(6)]
    ids[2][1] = ids[2][0]                                      # a repeated id inside a long row
    vals = [rng.uniform(-1, 1, 1500).round(3).tolist() for _ in range(6)]
    ent, rp, _ = datagen._pack(ids, vals, [0.0] * 6)
    pa, pb = np.array([0, 2, 4, 1, 3], np.uint32), np.array([1, 3, 5, 2, 3], np.uint32)
    m0 = start_model(oracle, n, k)
    h, ref = run_both(capi, oracle, ent, rp, pa, pb, k, lr, capi.SGD_SEQUENTIAL, 1, n, m0, epochs=2)
    check_params(h, ref, "long rows")
    h.close()
