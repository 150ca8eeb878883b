"""GPU: fmx_evaluate_ex / fmx_group_evaluate_ex -- exact AUC and log loss reduced on the device (include/fmx.h).

The oracle is libfm_amd.evalmetrics.classification_metrics applied to THE DEVICE'S OWN fmx_predict output of the same slot and
parameters: the integer fields (pos, neg, nan_rows, correct, auc_num2) are compared with ==, the log loss within the forward
bound of an fp64 sum (logloss_bound below).  n = 50 features, k = 2 (one case at k = 0, one at k = 17), 1 .. 3 entries per row."""
import ctypes as C
import math

import numpy as np
import pytest

from libfm_amd.evalmetrics import classification_metrics

pytestmark = pytest.mark.gpu

N, K = 50, 2
SCORE_GRID_CAP = 2048        # EVALX_BLOCKS of libfm_amd/csrc/fmx_eval_kernels.h: blocks of 256 threads the score kernel's grid is capped at
ONE_STRIDE_PLUS_A_WAVE = SCORE_GRID_CAP * 256 + 64      # one wavefront more than a single stride of the capped grid covers
ROW_COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 4097, ONE_STRIDE_PLUS_A_WAVE]
INT_FIELDS = ("rows", "pos", "neg", "nan_rows", "correct", "auc_num2")
LINKS = {"logistic": 0, "probit": 1}


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


def make_rows(capi, rows, seed, dyadic, positive_values=False):
    """1 .. 3 entries per row with distinct ids; dyadic: values from a few multiples of 1/8 (every sum of the prediction is then
    exact in fp32 whatever its order), else seeded real values"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 4, rows)
    rp = np.zeros(rows + 1, dtype=np.uint64)
    rp[1:] = np.cumsum(sizes)
    ent = np.zeros(int(rp[-1]), dtype=capi.ENTRY_DTYPE)
    base = rng.integers(0, N, rows)
    step = rng.integers(1, N // 3, rows)                 # ids base, base + step, base + 2 step (mod N): distinct inside a row
    row_of = np.repeat(np.arange(rows), sizes)
    pos_in_row = np.arange(len(ent)) - np.repeat(rp[:-1].astype(np.int64), sizes)
    ent["id"] = ((base[row_of] + pos_in_row * step[row_of]) % N).astype(np.uint32)
    if dyadic:
        ent["value"] = rng.choice(np.array([1.0, 0.5, 2.0] if positive_values else [1.0, 0.5, -1.0, 2.0]), len(ent)).astype(np.float32)
    else:
        v = rng.normal(0.0, 1.0, len(ent))
        ent["value"] = (np.abs(v) if positive_values else v).astype(np.float32)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    return ent, rp, y


def make_params(seed, dyadic, k=K):
    rng = np.random.default_rng(1000 + seed)
    if dyadic:
        lv = np.array([-0.5, -0.125, 0.0, 0.125, 0.5, 1.0])
        return 0.125, rng.choice(lv, N), rng.choice(lv, (k, N))
    return 0.07, rng.normal(0, 0.6, N), rng.normal(0, 0.6, (k, N))


def handle(capi, task=1, k=K, **kw):
    return capi.Handle(N, k, True, True, task, 0.0, 0.001, 0.002, 0.01, -1.0, 1.0, **kw)


def logloss_bound(want, rows):
    """|device - oracle| allowed: the device adds `rows` non-negative fp64 terms in a fixed order; the forward error of such a sum
    is at most (rows - 1) u |sum| with u = 2^-53, whatever the order, and the oracle's own sum (math.fsum) is correctly rounded;
    each term carries a few ulp of the device's log1p / exp / erfc / log on top (relative, since the terms are non-negative).
    rows * 2^-53 * 4 covers both; the absolute 1e-12 covers sums near zero, where -log(q) with q near 1 has no relative accuracy."""
    return abs(want) * rows * 2.0 ** -53 * 4 + 1e-12


def check_against_oracle(capi, h, slot, rows, y, links=("logistic", "probit")):
    p = h.predict(slot, rows)
    out = None
    for link in links:
        ev = h.evaluate_ex(slot, LINKS[link])
        want = classification_metrics(p, y, link)
        got = {f: int(getattr(ev, f)) for f in INT_FIELDS}
        print(link, rows, got, ev.auc, ev.logloss, "oracle", want["auc_num2"], want["auc"], want["logloss"])
        assert got == {f: want[f] for f in INT_FIELDS}
        if math.isnan(want["auc"]):
            assert math.isnan(ev.auc)
        else:
            assert ev.auc == want["auc_num2"] / (2 * want["pos"] * want["neg"])
        if math.isnan(want["logloss"]):
            assert math.isnan(ev.logloss)
        elif math.isinf(want["logloss"]):
            assert ev.logloss == want["logloss"]
        else:
            assert abs(ev.logloss - want["logloss"]) <= logloss_bound(want["logloss"], rows)
        assert ev.accuracy == want["correct"] / rows and ev.rmse == 0.0 and ev.mae == 0.0
        out = out or (ev, want)
    return out


@pytest.fixture(scope="module")
def hc(capi):
    h = handle(capi)
    yield h
    h.close()


@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "real"])
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_counts_auc_and_logloss_equal_the_oracle(capi, hc, rows, dyadic):
    ent, rp, y = make_rows(capi, rows, rows + 7 * dyadic, dyadic)
    hc.set_params(*make_params(rows, dyadic))
    hc.upload_rows(0, ent, rp, y)
    ev, want = check_against_oracle(capi, hc, 0, rows, y)
    if dyadic and rows >= 255:                             # ties dominate: far fewer distinct scores than rows
        assert len(np.unique(hc.predict(0, rows))) < rows // 2
    if want["pos"] and want["neg"]:
        assert ev.rank_seconds > 0.0
    assert ev.device_seconds >= ev.rank_seconds


@pytest.mark.parametrize("k", [0, 17])
def test_other_factor_widths(capi, k):
    h = handle(capi, k=k)
    ent, rp, y = make_rows(capi, 257, 3, False)
    w0, w, v = make_params(5, False, k)
    h.set_params(w0, w, v if k else None)
    h.upload_rows(0, ent, rp, y)
    check_against_oracle(capi, h, 0, 257, y)
    h.close()


def test_single_value_cases(capi, hc):
    ent, rp, y = make_rows(capi, 300, 11, True)
    hc.set_params(0.0, np.zeros(N), np.zeros((K, N)))      # a zero model: every score equal
    hc.upload_rows(0, ent, rp, y)
    ev, want = check_against_oracle(capi, hc, 0, 300, y)
    assert ev.auc == 0.5 and ev.auc_num2 == ev.pos * ev.neg
    hc.set_params(*make_params(1, False))
    for sign in (1.0, -1.0):                               # one class only
        hc.upload_rows(0, ent, rp, np.full(300, sign, dtype=np.float32))
        ev, _ = check_against_oracle(capi, hc, 0, 300, np.full(300, sign, dtype=np.float32))
        assert math.isnan(ev.auc) and ev.auc_num2 == 0 and (ev.pos, ev.neg) == ((300, 0) if sign > 0 else (0, 300))
        assert not math.isnan(ev.logloss)
    hc.upload_rows(0, ent[:0], np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.float32))     # an empty slot
    ev = hc.evaluate_ex(0)
    assert ev.rows == 0 and math.isnan(ev.auc) and math.isnan(ev.logloss)
    assert (ev.pos, ev.neg, ev.correct, ev.auc_num2, ev.nan_rows) == (0, 0, 0, 0, 0)


def test_nan_and_infinite_weights(capi, hc):
    rows, j = 4097, 17
    ent, rp, y = make_rows(capi, rows, 21, False, positive_values=True)
    holds_j = np.add.reduceat((ent["id"] == j).astype(np.int64), rp[:-1].astype(np.int64)) > 0
    w0, w, v = make_params(2, False)
    w[j] = np.nan
    hc.set_params(w0, w, v)
    hc.upload_rows(0, ent, rp, y)
    ev, want = check_against_oracle(capi, hc, 0, rows, y)
    assert ev.nan_rows == int(holds_j.sum()) > 0
    assert math.isnan(ev.auc) and math.isnan(ev.logloss) and ev.auc_num2 == 0
    assert (ev.pos, ev.neg, ev.correct) == (want["pos"], want["neg"], want["correct"]) and ev.correct > 0
    w[j] = np.inf                                          # (positive values: w_j x is +inf in every row that holds j)
    hc.set_params(w0, w, v)
    p = hc.predict(0, rows)
    assert np.all(np.isposinf(p[holds_j])) and np.all(np.isfinite(p[~holds_j]))
    ev, want = check_against_oracle(capi, hc, 0, rows, y)
    assert ev.nan_rows == 0 and ev.auc_num2 == want["auc_num2"] > 0
    assert ev.logloss == math.inf                          # some of those rows are negatives


@pytest.mark.parametrize("task", [0, 1])
def test_rmse_mae_accuracy_agree_with_fmx_evaluate(capi, task):
    rows = 4097
    ent, rp, y = make_rows(capi, rows, 31, False)
    if task == 0:
        y = np.random.default_rng(5).normal(0.0, 0.8, rows).astype(np.float32)
    h = handle(capi, task=task)
    h.set_params(*make_params(3, False))
    h.upload_rows(0, ent, rp, y)
    a, b = h.evaluate(0), h.evaluate_ex(0)
    print(task, a.rmse, b.rmse, a.mae, b.mae, a.accuracy, b.accuracy)
    assert abs(a.rmse - b.rmse) <= 1e-12 and abs(a.mae - b.mae) <= 1e-12 and abs(a.accuracy - b.accuracy) <= 1e-12
    assert b.rows == rows
    if task == 0:                                          # a regression handle: no classification fields, nothing sorted
        assert b.rmse > 0 and b.mae > 0 and b.accuracy == 0.0
        assert (b.pos, b.neg, b.correct, b.nan_rows, b.auc_num2) == (0, 0, 0, 0, 0)
        assert math.isnan(b.auc) and math.isnan(b.logloss) and b.rank_seconds == 0.0
    else:
        assert b.rmse == 0.0 and b.mae == 0.0 and b.accuracy > 0
    h.close()


def _fields(ev):
    return {name: getattr(ev, name) for name, _ in type(ev)._fields_ if name not in ("device_seconds", "rank_seconds")}


@pytest.mark.parametrize("task", [0, 1])
def test_two_calls_are_bit_identical(capi, task):
    rows = ONE_STRIDE_PLUS_A_WAVE
    ent, rp, y = make_rows(capi, rows, 41, False)
    h = handle(capi, task=task)
    h.set_params(*make_params(4, False))
    h.upload_rows(0, ent, rp, y)
    a, b = _fields(h.evaluate_ex(0, 1)), _fields(h.evaluate_ex(0, 1))
    for f in a:
        assert np.float64(a[f]).tobytes() == np.float64(b[f]).tobytes() if isinstance(a[f], float) else a[f] == b[f], f
    h.close()


def test_weight_side_stream(capi):
    rows = 4097
    ent, rp, y = make_rows(capi, rows, 51, False)
    h1, h2 = handle(capi), handle(capi)
    h1.set_params(*make_params(6, False))
    h1.upload_rows(0, ent, rp, y)
    h1.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_FUSED, 256, 32, capi.FLAG_KEEP_WSIDE, 2)
    ev1 = h1.evaluate_ex(0)
    assert ev1.flags & capi.EVAL_WSIDE
    h2.set_params(*h1.get_params())                        # the same fp32 parameters, no side stream
    h2.upload_rows(0, ent, rp, y)
    ev2 = h2.evaluate_ex(0)
    assert not (ev2.flags & capi.EVAL_WSIDE)
    assert {f: getattr(ev1, f) for f in INT_FIELDS} == {f: getattr(ev2, f) for f in INT_FIELDS}
    assert ev1.pos and ev1.neg and ev1.auc_num2
    check_against_oracle(capi, h1, 0, rows, y, links=("logistic",))
    h1.close()
    h2.close()


def _relational(capi, rows, seed):
    """dyadic block-structured rows over the N attributes: main rows of one entry (ids 0 .. 9), one block of 7 rows with 1 .. 2
    entries over the block's 40 attributes (global ids 10 .. 49)"""
    rng = np.random.default_rng(seed)
    vals = np.array([1.0, 0.5, -1.0, 2.0])
    ent = np.zeros(rows, dtype=capi.ENTRY_DTYPE)
    ent["id"], ent["value"] = rng.integers(0, 10, rows), rng.choice(vals, rows)
    rp = np.arange(rows + 1, dtype=np.uint64)
    bsizes = rng.integers(1, 3, 7)
    brp = np.zeros(8, dtype=np.uint64)
    brp[1:] = np.cumsum(bsizes)
    bent = np.zeros(int(brp[-1]), dtype=capi.ENTRY_DTYPE)
    bent["id"] = np.concatenate([rng.choice(40, s, replace=False) for s in bsizes])
    bent["value"] = rng.choice(vals, len(bent))
    mp = rng.integers(0, 7, rows).astype(np.uint32)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    return ent, rp, y, [(bent, brp, mp, 10)]


def test_kept_relation_blocks(capi, hc):
    rows = 4097
    ent, rp, y, rel = _relational(capi, rows, 61)
    hc.set_params(*make_params(7, True))
    hc.upload_block_rows(0, ent, rp, y, rel, keep=True)
    hc.upload_block_rows(1, ent, rp, y, rel, keep=False)
    for link in LINKS.values():
        a, b = hc.evaluate_ex(0, link), hc.evaluate_ex(1, link)
        assert {f: getattr(a, f) for f in INT_FIELDS} == {f: getattr(b, f) for f in INT_FIELDS}
        assert a.auc_num2 > 0 and abs(a.logloss - b.logloss) <= logloss_bound(b.logloss, rows)
    check_against_oracle(capi, hc, 0, rows, y)
    hc.free_rows(1)


@pytest.mark.parametrize("world", [2, 3])
def test_loopback_groups(capi, hc, world):
    rows = 4097
    ent, rp, y = make_rows(capi, rows, 71, True)
    params = make_params(8, True)
    hc.set_params(*params)
    hc.upload_rows(0, ent, rp, y)
    hs = [handle(capi, device=0, shard_rank=r, shard_world=world, shard_hash=1) for r in range(world)]
    g = capi.Group(hs)
    g.set_params(*params)
    g.upload_rows(0, ent, rp, y)
    for link in LINKS.values():
        one, grp = hc.evaluate_ex(0, link), g.evaluate_ex(0, link)
        assert {f: getattr(grp, f) for f in INT_FIELDS} == {f: getattr(one, f) for f in INT_FIELDS}
        assert one.auc_num2 > 0 and grp.auc == one.auc
        assert abs(grp.logloss - one.logloss) <= logloss_bound(one.logloss, rows)
    # a shard handle passed to fmx_evaluate_ex itself
    with pytest.raises(capi.FmxError) as ei:
        hs[1].evaluate_ex(0)
    assert ei.value.code == -4 and "fmx_evaluate_ex" in ei.value.text
    g.close()
    for h in hs:
        h.close()


def test_kept_blocks_on_shards(capi, hc):
    rows = 4097
    ent, rp, y, rel = _relational(capi, rows, 81)
    params = make_params(9, True)
    hc.set_params(*params)
    hc.upload_block_rows(0, ent, rp, y, rel, keep=True)
    hs = [handle(capi, device=0, shard_rank=r, shard_world=2, shard_hash=1) for r in range(2)]
    g = capi.Group(hs)
    g.set_params(*params)
    g.upload_block_rows(0, ent, rp, y, rel, keep=True)
    one, grp = hc.evaluate_ex(0), g.evaluate_ex(0)
    assert {f: getattr(grp, f) for f in INT_FIELDS} == {f: getattr(one, f) for f in INT_FIELDS}
    assert abs(grp.logloss - one.logloss) <= logloss_bound(one.logloss, rows)
    g.close()
    for h in hs:
        h.close()


def test_one_handle_group_forwards(capi):
    rows = 257
    ent, rp, y = make_rows(capi, rows, 91, False)
    h = handle(capi)
    g = capi.Group([h])
    h.set_params(*make_params(10, False))
    h.upload_rows(0, ent, rp, y)
    assert _fields(g.evaluate_ex(0, 1)) == _fields(h.evaluate_ex(0, 1))
    g.close()
    h.close()


def test_refusals(capi, hc):
    lib = capi.load()
    ent, rp, y = make_rows(capi, 10, 1, True)
    hc.upload_rows(0, ent, rp, y)
    hc.upload_rows(2, ent, rp, None)                        # a slot without targets
    out = capi.EvalEx()

    def refused(rc, code):
        assert rc == code
        assert b"fmx_evaluate_ex" in lib.fmx_last_error(hc.h)

    refused(lib.fmx_evaluate_ex(hc.h, 0, None, None), -1)                                          # NULL out
    refused(lib.fmx_evaluate_ex(hc.h, 0, C.byref(capi.EvalOpts(2, 0)), C.byref(out)), -1)          # unknown link
    refused(lib.fmx_evaluate_ex(hc.h, 0, C.byref(capi.EvalOpts(0, 1)), C.byref(out)), -1)          # flags != 0
    refused(lib.fmx_evaluate_ex(hc.h, 5, None, C.byref(out)), -3)                                  # never uploaded
    refused(lib.fmx_evaluate_ex(hc.h, 2, None, C.byref(out)), -3)                                  # no targets
    assert lib.fmx_evaluate_ex(hc.h, 0, None, C.byref(out)) == 0 and out.rows == 10                # NULL opts = logistic
    assert out.logloss == hc.evaluate_ex(0, capi.LINK_LOGISTIC).logloss
    hc.free_rows(2)


def _separable(capi, rows, seed):
    """a toy set a linear model separates: feature 0 .. 24 in positive rows, 25 .. 49 in negative rows, plus one shared feature"""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    ent = np.zeros(2 * rows, dtype=capi.ENTRY_DTYPE)
    ent["id"][0::2] = np.where(y > 0, rng.integers(0, 24, rows), rng.integers(25, 49, rows))
    ent["id"][1::2] = 49
    ent["value"] = 1.0
    return ent, np.arange(0, 2 * rows + 1, 2, dtype=np.uint64), y


def test_learner_extra_metrics(capi, capsys):
    from libfm_amd import learner as L
    tr, te = L.Data(*_separable(capi, 200, 1)), L.Data(*_separable(capi, 200, 2))
    l = L.FMLearnSGD()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor = N, K
    l.fm.init(np.random.default_rng(3))
    l.task, l.learn_rate, l.num_iter, l.min_target, l.max_target = L.TASK_CLASSIFICATION, 0.05, 5, -1.0, 1.0
    l.extra_metrics = ("auc", "logloss")
    l.init()
    l.learn(tr, te)
    want = classification_metrics(l.predict_raw(te), te.target)
    assert l.log[-1]["auc_test"] == want["auc"] and want["auc"] > 0.9
    assert abs(l.log[-1]["logloss_test"] - want["logloss"]) <= logloss_bound(want["logloss"], 200)
    assert set(l.log[-1]) >= {"auc_train", "auc_test", "logloss_train", "logloss_test"}
    ev = l.evaluate_ex(te)
    assert ev.auc_num2 == want["auc_num2"]
    err = capsys.readouterr().err
    assert err.count("\tauc: Train=") == 5 and err.count("\tlogloss: Train=") == 5
    l.close()
    m = L.FMLearnMCMC()
    m.extra_metrics = ("auc",)
    with pytest.raises(NotImplementedError):
        m.learn(tr, te)


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-handle", "two-shards"])
def test_als_learner_extra_metrics(capi, capsys, devices):
    """the ALS learner scores with the probit link, on one handle and over a loopback group of two shards"""
    from libfm_amd import learner as L
    tr, te = L.Data(*_separable(capi, 200, 1)), L.Data(*_separable(capi, 200, 2))
    l = L.FMLearnALS()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor = N, K
    l.fm.init(np.random.default_rng(3))
    l.task, l.num_iter, l.min_target, l.max_target = L.TASK_CLASSIFICATION, 2, -1.0, 1.0
    l.w_lambda = l.v_lambda = 1.0
    l.devices = devices
    l.extra_metrics = ("auc", "logloss")
    l.init()
    l.learn(tr, te)
    want = classification_metrics(l._h.predict(1, te.num_cases), te.target, "probit")
    assert l.log[-1]["auc_test"] == want["auc"] and int(l.evaluate_ex(te).auc_num2) == want["auc_num2"]
    assert abs(l.log[-1]["logloss_test"] - want["logloss"]) <= logloss_bound(want["logloss"], 200)
    err = capsys.readouterr().err
    assert err.count("\tauc: Train=") == 2 and err.count("\tlogloss: Train=") == 2
    l.close()


def _write_libfm(path, ent, rp, y):
    with open(path, "w") as f:
        for r in range(len(y)):
            f.write("%g %s\n" % (y[r], " ".join("%d:%g" % (e["id"], e["value"]) for e in ent[int(rp[r]):int(rp[r + 1])])))


def test_cli_metrics_flag(capi, tmp_path, capsys):
    from libfm_amd import cli
    trf, tef = str(tmp_path / "tr.libfm"), str(tmp_path / "te.libfm")
    _write_libfm(trf, *_separable(capi, 200, 1))
    _write_libfm(tef, *_separable(capi, 200, 2))
    argv = ["-task", "c", "-train", trf, "-test", tef, "-dim", "1,1,2", "-iter", "3", "-method", "sgd", "-learn_rate", "0.05",
            "-init_stdev", "0.1", "-seed", "42"]
    assert cli.main(argv) == 0
    plain = capsys.readouterr()
    assert cli.main(argv + ["-metrics", "auc,logloss"]) == 0
    flagged = capsys.readouterr()
    assert flagged.out == plain.out and plain.out.count("#Iter=") == 3
    assert "auc:" not in plain.err and "logloss:" not in plain.err
    assert flagged.err.count("\tauc: Train=") == 3 and flagged.err.count("\tlogloss: Train=") == 3
    for extra in (["-task", "r"], ["-method", "mcmc"]):      # (a repeated flag: the later value holds)
        assert cli.main(argv + ["-metrics", "auc"] + extra) == 0
        cap = capsys.readouterr()
        assert "ERROR:" in cap.err and "-metrics" in cap.err and "#Iter=" not in cap.out
