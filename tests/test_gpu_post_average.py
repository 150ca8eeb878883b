"""GPU: fmx_post_* / fmx_group_post_* -- the averaged predictions of `-method mcmc` kept on the device (include/fmx.h, DESIGN.md
section 15).

The draws are seeded parameter sets put there with set_params; no sweep is needed.  The oracle is
libfm_amd.evalmetrics.PosteriorAverage fed THE DEVICE'S OWN fmx_predict output after each set_params: on regression handles the
sums are compared with == (clamp and add are exact restatements), on classification handles within draws * 64 * 2^-53 (the
device's exp against the host's inside the same polynomial, on values <= 1).  The integer fields of the metrics are compared with
== against the oracle applied to the device's own downloaded sums (post_get), the fp64 metrics within the forward bound of an
fp64 sum (metric_bound below).  n = 200 features, k = 2 (cases at k = 0 and k = 17)."""
import ctypes as C
import math

import numpy as np
import pytest

from libfm_amd.evalmetrics import (POST_ALL, POST_LATE, POST_THIS, PosteriorAverage, posterior_evaluate_ex, posterior_mean,
                                   posterior_metric)

pytestmark = pytest.mark.gpu

N, K = 200, 2
GRID_CAP = 2048              # EVALX_BLOCKS of libfm_amd/csrc/fmx_eval_kernels.h: blocks of 256 threads the grids are capped at
ONE_STRIDE_PLUS_A_WAVE = GRID_CAP * 256 + 64
WHICH = (POST_THIS, POST_ALL, POST_LATE)
METRIC_INTS = ("rows", "nan_rows", "correct")
EVAL_INTS = ("rows", "nan_rows", "pos", "neg", "correct", "auc_num2")
LO, HI = -1.0, 1.0


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


def make_rows(capi, rows, seed, dyadic, task=1, one_entry=False):
    """1 .. 3 entries per row with distinct ids (one_entry: exactly one); dyadic: values from a few multiples of 1/8 (every sum of
    the prediction is then exact in fp32 whatever its order), else seeded real values"""
    rng = np.random.default_rng(seed)
    sizes = np.ones(rows, dtype=np.int64) if one_entry else rng.integers(1, 4, rows)
    rp = np.zeros(rows + 1, dtype=np.uint64)
    rp[1:] = np.cumsum(sizes)
    ent = np.zeros(int(rp[-1]), dtype=capi.ENTRY_DTYPE)
    base, step = rng.integers(0, N, rows), rng.integers(1, N // 3, rows)
    row_of = np.repeat(np.arange(rows), sizes)
    pos_in_row = np.arange(len(ent)) - np.repeat(rp[:-1].astype(np.int64), sizes)
    ent["id"] = ((base[row_of] + pos_in_row * step[row_of]) % N).astype(np.uint32)
    ent["value"] = (rng.choice(np.array([1.0, 0.5, -1.0, 2.0]), len(ent)) if dyadic else rng.normal(0.0, 1.0, len(ent))).astype(np.float32)
    if task == 1:
        y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    else:
        y = rng.normal(0.0, 0.8, rows).astype(np.float32)
    return ent, rp, y


def make_params(seed, dyadic, k=K):
    rng = np.random.default_rng(1000 + seed)
    if dyadic:
        lv = np.array([-0.5, -0.125, 0.0, 0.125, 0.5, 1.0])
        return 0.125, rng.choice(lv, N), rng.choice(lv, (k, N)) if k else None
    return 0.07, rng.normal(0, 0.6, N), rng.normal(0, 0.6, (k, N)) if k else None


def handle(capi, task=1, k=K, **kw):
    return capi.Handle(N, k, True, True, task, 0.0, 0.001, 0.002, 0.01, LO, HI, **kw)


def metric_bound(want, rows):
    """|device - oracle| allowed for rmse / mae / ll_ref / logloss: the device adds `rows` terms of one sign in fp64 in a fixed
    order -- forward error at most (rows - 1) u |sum|, u = 2^-53, whatever the order -- and each term carries a few ulp of the
    device's log / log10 / sqrt on top; rows * 2^-53 * 4 covers both, the absolute 1e-12 covers sums near zero (the bound of
    tests/test_gpu_eval_ex.py)"""
    return abs(want) * rows * 2.0 ** -53 * 4 + 1e-12


def sum_bound(task, draws):
    return 0.0 if task == 0 else draws * 64 * 2.0 ** -53


def close_to(got, want, rows):
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want):
        return got == want
    return abs(got - want) <= metric_bound(want, rows)


def device_means(h, slot, rows, eval_n):
    """the three vectors' means over the evaluated rows from the device's own sums (None: no draw in the vector yet)"""
    out = {}
    for which in WHICH:
        vec, cnt = h.post_get(slot, which, rows)
        out[which] = None if cnt == 0 else (vec if which == POST_THIS else posterior_mean(vec, cnt))[:eval_n]
    return out


def check_stats(task, st, means, y, eval_n, tag=""):
    for which in WHICH:
        want, got = posterior_metric(task, means[which], y, LO, HI), st.m[which]
        print(tag, "which", which, {f: getattr(got, f) for f, _ in type(got)._fields_}, "oracle", want)
        assert {f: int(getattr(got, f)) for f in METRIC_INTS} == {f: want[f] for f in METRIC_INTS}
        for f in ("rmse", "mae", "accuracy", "ll_ref"):
            assert close_to(getattr(got, f), want[f], max(eval_n, 1)), (which, f)
        if want["rows"]:
            assert got.accuracy == want["correct"] / want["rows"]


def check_eval_ex(task, ev, mean, y, tag=""):
    want = posterior_evaluate_ex(task, mean, y, LO, HI)
    print(tag, {f: int(getattr(ev, f)) for f in EVAL_INTS}, ev.auc, ev.logloss, ev.rmse, ev.mae, "oracle", want["auc_num2"], want["auc"],
          want["logloss"], want["rmse"], want["mae"])
    assert {f: int(getattr(ev, f)) for f in EVAL_INTS} == {f: want[f] for f in EVAL_INTS}
    if math.isnan(want["auc"]):
        assert math.isnan(ev.auc)
    else:
        assert ev.auc == want["auc_num2"] / (2 * want["pos"] * want["neg"])
    for f in ("logloss", "rmse", "mae"):
        assert close_to(getattr(ev, f), want[f], max(want["rows"], 1)), f
    assert ev.accuracy == (want["correct"] / want["rows"] if want["rows"] and task == 1 else 0.0)
    return want


def run_case(capi, h, task, rows, draws, burn_in, eval_rows, dyadic, seed, one_entry=False, eval_which=WHICH):
    ent, rp, y = make_rows(capi, rows, seed, dyadic, task, one_entry)
    h.upload_rows(0, ent, rp, y)
    h.post_begin(0, burn_in, eval_rows)
    eval_n = eval_rows or rows
    oracle = PosteriorAverage(task, LO, HI, burn_in, eval_rows)
    for d in range(draws):
        w0, w, v = make_params(seed + 31 * d, dyadic, h.k)
        h.set_params(w0, w, v)
        oracle.accumulate(h.predict(0, rows))
        st = h.post_accumulate(0)
        assert (st.draws, st.late_draws) == (oracle.draws, oracle.late_draws) and st.device_seconds > 0
        worst = 0.0
        for which in WHICH:
            got, cnt = h.post_get(0, which, rows)
            assert cnt == oracle.count(which)
            worst = max(worst, float(np.max(np.abs(got - oracle.get(which)))))
        print("draw", d, "rows", rows, "task", task, "max |device sum - oracle sum|", worst)
        assert worst <= sum_bound(task, d + 1)
        check_stats(task, st, device_means(h, 0, rows, eval_n), y, eval_n, "draw %d" % d)
    means = device_means(h, 0, rows, eval_n)
    for which in eval_which:
        ev = h.post_evaluate_ex(0, which)
        want = check_eval_ex(task, ev, means[which], y, "evaluate_ex which %d" % which)
        if want["pos"] and want["neg"] and not want["nan_rows"]:
            assert ev.rank_seconds > 0.0
        assert ev.device_seconds >= ev.rank_seconds
    return oracle, y


@pytest.fixture(scope="module")
def hs(capi):
    pair = {0: handle(capi, 0), 1: handle(capi, 1)}
    yield pair
    for h in pair.values():
        h.close()


# rows, draws, burn_in, eval_rows (-1: rows - 1): every row count with 7 draws across burn_in = 5; 1 draw and the other burn-ins and
# eval_rows spread over them
CASES = [(1, 7, 5, 0), (1, 1, 0, 1), (63, 7, 5, 1), (64, 7, 1, -1), (64, 1, 9, 0), (65, 7, 5, 0), (65, 7, 9, -1), (257, 7, 5, -1),
         (257, 7, 0, 1), (4097, 7, 5, 0), (4097, 1, 1, -1)]


@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "real"])
@pytest.mark.parametrize("task", [0, 1], ids=["regression", "classification"])
@pytest.mark.parametrize("rows,draws,burn_in,eval_rows", CASES)
def test_sums_and_metrics_equal_the_oracle(capi, hs, task, rows, draws, burn_in, eval_rows, dyadic):
    eval_rows = rows - 1 if eval_rows < 0 else eval_rows
    oracle, _ = run_case(capi, hs[task], task, rows, draws, burn_in, eval_rows, dyadic, rows + 7 * dyadic + burn_in)
    if dyadic and task == 1 and rows >= 4097:              # ties dominate: far fewer distinct values of a draw than rows
        assert len(np.unique(oracle.get(POST_THIS))) < rows // 2


@pytest.mark.parametrize("task", [0, 1], ids=["regression", "classification"])
@pytest.mark.parametrize("draws,burn_in", [(7, 5), (1, 0)])
def test_one_wavefront_past_one_stride_of_the_grid(capi, hs, task, draws, burn_in):
    """a one-entry-per-row slot; the AUC oracle (a Python sort) is taken for the mean over all draws only"""
    run_case(capi, hs[task], task, ONE_STRIDE_PLUS_A_WAVE, draws, burn_in, ONE_STRIDE_PLUS_A_WAVE - 1, draws == 1, 5 + draws,
             one_entry=True, eval_which=(POST_ALL,))


@pytest.mark.parametrize("task", [0, 1], ids=["regression", "classification"])
@pytest.mark.parametrize("k", [0, 17])
def test_other_factor_widths(capi, task, k):
    h = handle(capi, task, k)
    run_case(capi, h, task, 257, 7, 5, 0, False, 3 + k)
    h.close()


def test_a_zero_model_and_one_class(capi, hs):
    h, rows = hs[1], 300
    ent, rp, y = make_rows(capi, rows, 11, True)
    h.upload_rows(0, ent, rp, y)
    h.post_begin(0, 1)
    h.set_params(0.0, np.zeros(N), np.zeros((K, N)))       # every draw cdf(0): all means equal
    for _ in range(3):
        st = h.post_accumulate(0)
    for which in WHICH:
        ev = h.post_evaluate_ex(0, which)
        assert ev.auc == 0.5 and ev.auc_num2 == ev.pos * ev.neg > 0
        vec, cnt = h.post_get(0, which, rows)
        assert np.all(vec == vec[0]) and abs(vec[0] / cnt - 0.5) < 1e-8
    assert st.m[POST_ALL].correct == int((y > 0).sum())    # .5000000005 >= .5: the positives
    h.set_params(*make_params(1, False))
    for sign in (1.0, -1.0):                               # one class only
        ys = np.full(rows, sign, dtype=np.float32)
        h.upload_rows(0, ent, rp, ys)
        h.post_begin(0, 0)
        h.post_accumulate(0)
        means = device_means(h, 0, rows, rows)
        ev = h.post_evaluate_ex(0, POST_ALL)
        check_eval_ex(1, ev, means[POST_ALL], ys)
        assert math.isnan(ev.auc) and ev.auc_num2 == 0 and (ev.pos, ev.neg) == ((rows, 0) if sign > 0 else (0, rows))
        assert not math.isnan(ev.logloss) and ev.rank_seconds == 0.0


@pytest.mark.parametrize("task", [0, 1], ids=["regression", "classification"])
def test_a_nan_parameter_in_one_draw(capi, hs, task):
    """draw 3 of 7 has a NaN weight: the rows that hold the feature are NaN in ALL and LATE from then on, THIS recovers in draw 4"""
    h, rows, j = hs[task], 4097, 17
    ent, rp, y = make_rows(capi, rows, 21, False, task)
    holds_j = np.add.reduceat((ent["id"] == j).astype(np.int64), rp[:-1].astype(np.int64)) > 0
    n_bad = int(holds_j.sum())
    assert 0 < n_bad < rows
    h.upload_rows(0, ent, rp, y)
    h.post_begin(0, 1)
    for d in range(7):
        w0, w, v = make_params(50 + d, False)
        if d == 2:
            w[j] = np.nan
        h.set_params(w0, w, v)
        st = h.post_accumulate(0)
        want = (n_bad if d == 2 else 0, n_bad if d >= 2 else 0, n_bad if d >= 2 else 0)
        assert tuple(int(st.m[q].nan_rows) for q in WHICH) == want, d
        check_stats(task, st, device_means(h, 0, rows, rows), y, rows, "draw %d" % d)
        for q, bad in zip(WHICH, want):
            m = st.m[q]
            if q == POST_LATE and d < 1:                    # burn_in = 1: no late draw yet
                assert m.rows == 0 and math.isnan(m.rmse) and math.isnan(m.ll_ref)
                continue
            assert all(math.isnan(x) == bool(bad) for x in ((m.rmse, m.mae) if task == 0 else (m.ll_ref,)))
            assert m.rows == rows and (task == 0 or 0 < m.correct <= rows - bad)
    means = device_means(h, 0, rows, rows)
    for which in WHICH:
        ev = h.post_evaluate_ex(0, which)
        check_eval_ex(task, ev, means[which], y)
        assert ev.nan_rows == (0 if which == POST_THIS else n_bad)
        assert math.isnan(ev.auc) == (task == 0 or which != POST_THIS) and (which == POST_THIS or ev.auc_num2 == 0)
    vec, _ = h.post_get(0, POST_ALL, rows)
    assert np.array_equal(np.isnan(vec), holds_j)


def test_saturated_means(capi, hs):
    """a weight of 40 on one feature with positive values: cdf = 1.0 exactly, log loss +inf on its negatives, ll_ref finite"""
    h, rows, j = hs[1], 257, 5
    ent, rp, y = make_rows(capi, rows, 23, True)
    ent["value"] = np.abs(ent["value"])
    holds_j = np.add.reduceat((ent["id"] == j).astype(np.int64), rp[:-1].astype(np.int64)) > 0
    assert (holds_j & (y < 0)).any()
    w = np.zeros(N)
    w[j] = 80.0                                            # (values >= 0.5)
    h.upload_rows(0, ent, rp, y)
    h.post_begin(0, 0)
    h.set_params(0.0, w, np.zeros((K, N)))
    st = h.post_accumulate(0)
    vec, _ = h.post_get(0, POST_ALL, rows)
    assert np.all(vec[holds_j] == 1.0)
    ev = h.post_evaluate_ex(0, POST_ALL)
    check_eval_ex(1, ev, vec, y)
    assert ev.logloss == math.inf and math.isfinite(st.m[POST_ALL].ll_ref) and ev.auc_num2 > 0


def _fields(s):
    out = {}
    for name, _ in type(s)._fields_:
        if name in ("device_seconds", "rank_seconds"):
            continue
        v = getattr(s, name)
        out[name] = [bytes(m) for m in v] if name == "m" else (np.float64(v).tobytes() if isinstance(v, float) else v)
    return out


@pytest.mark.parametrize("task", [0, 1], ids=["regression", "classification"])
def test_two_sequences_are_bit_identical(capi, hs, task):
    h, rows = hs[task], ONE_STRIDE_PLUS_A_WAVE
    ent, rp, y = make_rows(capi, rows, 41, False, task, one_entry=True)
    h.upload_rows(0, ent, rp, y)
    runs = []
    for _ in range(2):
        h.post_begin(0, 1)
        got = []
        for d in range(3):
            h.set_params(*make_params(60 + d, False))
            got.append(_fields(h.post_accumulate(0)))
        got += [_fields(h.post_evaluate_ex(0, q)) for q in WHICH]
        got += [h.post_get(0, q, rows)[0].tobytes() for q in WHICH]
        runs.append(got)
    assert runs[0] == runs[1]


def test_state_and_refusals(capi, hs):
    lib, h = capi.load(), hs[1]
    ent, rp, y = make_rows(capi, 10, 1, True)
    h.upload_rows(0, ent, rp, y)
    h.upload_rows(2, ent, rp, None)                         # a slot without targets
    h.set_params(*make_params(2, True))
    ev, st = capi.EvalEx(), capi.PostStats()

    def refused(rc, code, who):
        assert rc == code
        assert who.encode() in lib.fmx_last_error(h.h)

    # without fmx_post_begin
    refused(lib.fmx_post_accumulate(h.h, 0, C.byref(st)), -3, "fmx_post_accumulate")
    refused(lib.fmx_post_evaluate_ex(h.h, 0, 1, C.byref(ev)), -3, "fmx_post_evaluate_ex")
    refused(lib.fmx_post_get(h.h, 0, 1, None, None), -3, "fmx_post_get")
    refused(lib.fmx_post_end(h.h, 0), -3, "fmx_post_end")
    # arguments
    refused(lib.fmx_post_begin(h.h, 0, C.byref(capi.PostOpts(5, 0, 1, 0))), -1, "fmx_post_begin")       # flags != 0
    refused(lib.fmx_post_begin(h.h, 0, C.byref(capi.PostOpts(5, 11, 0, 0))), -1, "fmx_post_begin")      # eval_rows > n_rows
    refused(lib.fmx_post_begin(h.h, 5, None), -3, "fmx_post_begin")                                     # never uploaded
    refused(lib.fmx_post_begin(h.h, 2, None), -3, "fmx_post_begin")                                     # no targets
    refused(lib.fmx_post_begin(h.h, 99, None), -1, "fmx_post_begin")                                    # no such slot
    assert lib.fmx_post_begin(h.h, 0, None) == 0                                                        # NULL opts = {5, 0, 0}
    refused(lib.fmx_post_evaluate_ex(h.h, 0, 1, None), -1, "fmx_post_evaluate_ex")                      # NULL out
    refused(lib.fmx_post_evaluate_ex(h.h, 0, 3, C.byref(ev)), -1, "fmx_post_evaluate_ex")               # which > 2
    refused(lib.fmx_post_get(h.h, 0, 3, None, None), -1, "fmx_post_get")
    # before the first draw: zero sums, an empty result
    assert lib.fmx_post_evaluate_ex(h.h, 0, 1, C.byref(ev)) == 0 and ev.rows == 0 and math.isnan(ev.auc) and math.isnan(ev.logloss)
    vec, cnt = h.post_get(0, POST_ALL, 10)
    assert cnt == 0 and not vec.any()
    assert lib.fmx_post_accumulate(h.h, 0, None) == 0                                                   # NULL out
    for d in range(5):
        st = h.post_accumulate(0)
    assert (st.draws, st.late_draws) == (6, 1) and st.m[POST_LATE].rows == 10                           # burn_in = 5 by default
    first, _ = h.post_get(0, POST_THIS, 10)
    # begin again = reset
    h.post_begin(0, 0)
    assert h.post_get(0, POST_ALL, 10)[1] == 0 and not h.post_get(0, POST_ALL, 10)[0].any()
    st = h.post_accumulate(0)
    assert (st.draws, st.late_draws) == (1, 1)
    assert np.array_equal(h.post_get(0, POST_ALL, 10)[0], first) and np.array_equal(h.post_get(0, POST_LATE, 10)[0], first)
    # a re-upload drops the accumulator, so does fmx_free_rows
    h.upload_rows(0, ent, rp, y)
    refused(lib.fmx_post_accumulate(h.h, 0, C.byref(st)), -3, "fmx_post_accumulate")
    h.post_begin(0)
    h.post_end(0)
    refused(lib.fmx_post_get(h.h, 0, 1, None, None), -3, "fmx_post_get")
    h.post_begin(0)
    h.free_rows(0)
    refused(lib.fmx_post_end(h.h, 0), -3, "fmx_post_end")
    # an empty slot: FMX_OK with zero rows
    h.upload_rows(0, ent[:0], np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.float32))
    h.post_begin(0, 0)
    st = h.post_accumulate(0)
    assert (st.draws, st.late_draws) == (1, 1) and all(st.m[q].rows == 0 and math.isnan(st.m[q].rmse) for q in WHICH)
    ev = h.post_evaluate_ex(0, POST_ALL)
    assert ev.rows == 0 and math.isnan(ev.auc) and h.post_get(0, POST_ALL, 0)[1] == 1
    h.free_rows(2)
    # a feature shard passed to the per-handle calls
    shard = handle(capi, device=0, shard_rank=1, shard_world=2, shard_hash=1)
    for who, call in (("fmx_post_begin", lambda: lib.fmx_post_begin(shard.h, 0, None)),
                      ("fmx_post_accumulate", lambda: lib.fmx_post_accumulate(shard.h, 0, None)),
                      ("fmx_post_evaluate_ex", lambda: lib.fmx_post_evaluate_ex(shard.h, 0, 1, C.byref(ev))),
                      ("fmx_post_get", lambda: lib.fmx_post_get(shard.h, 0, 1, None, None)),
                      ("fmx_post_end", lambda: lib.fmx_post_end(shard.h, 0))):
        assert call() == -4 and who.encode() in lib.fmx_last_error(shard.h)
    shard.close()


def _relational(capi, rows, seed):
    """dyadic block-structured rows over the N attributes: main rows of one entry (ids 0 .. 9), one block of 7 rows with 1 .. 2
    entries over the block's 190 attributes (global ids 10 .. 199)"""
    rng = np.random.default_rng(seed)
    vals = np.array([1.0, 0.5, -1.0, 2.0])
    ent = np.zeros(rows, dtype=capi.ENTRY_DTYPE)
    ent["id"], ent["value"] = rng.integers(0, 10, rows), rng.choice(vals, rows)
    rp = np.arange(rows + 1, dtype=np.uint64)
    bsizes = rng.integers(1, 3, 7)
    brp = np.zeros(8, dtype=np.uint64)
    brp[1:] = np.cumsum(bsizes)
    bent = np.zeros(int(brp[-1]), dtype=capi.ENTRY_DTYPE)
    bent["id"] = np.concatenate([rng.choice(N - 10, s, replace=False) for s in bsizes])
    bent["value"] = rng.choice(vals, len(bent))
    mp = rng.integers(0, 7, rows).astype(np.uint32)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    return ent, rp, y, [(bent, brp, mp, 10)]


def _same(a, b, rows, draws, task=1):
    """two accumulators of the same dyadic draws: y-hat is exact in fp32 whatever the order of its sums, so the integer fields are
    equal and the sums differ by no more than the classification bound"""
    (ha, sa), (hb, sb) = a, b
    for which in WHICH:
        (va, ca), (vb, cb) = ha.post_get(sa, which, rows), hb.post_get(sb, which, rows)
        assert ca == cb and float(np.max(np.abs(va - vb))) <= sum_bound(task, draws)
        ea, eb = ha.post_evaluate_ex(sa, which), hb.post_evaluate_ex(sb, which)
        assert {f: getattr(ea, f) for f in EVAL_INTS} == {f: getattr(eb, f) for f in EVAL_INTS}
        assert ea.auc_num2 > 0 and ea.auc == eb.auc and close_to(ea.logloss, eb.logloss, rows)


@pytest.mark.parametrize("world", [2, 3])
def test_loopback_groups(capi, hs, world):
    rows, draws, h = 4097, 7, hs[1]
    ent, rp, y = make_rows(capi, rows, 71, True)
    shards = [handle(capi, device=0, shard_rank=r, shard_world=world, shard_hash=1) for r in range(world)]
    g = capi.Group(shards)
    h.upload_rows(0, ent, rp, y)
    g.upload_rows(0, ent, rp, y)
    h.post_begin(0, 5, rows - 1)
    g.post_begin(0, 5, rows - 1)
    for d in range(draws):
        params = make_params(80 + d, True)
        h.set_params(*params)
        g.set_params(*params)
        one, grp = h.post_accumulate(0), g.post_accumulate(0)
        assert (grp.draws, grp.late_draws) == (one.draws, one.late_draws)
        for q in WHICH:
            assert {f: getattr(grp.m[q], f) for f in METRIC_INTS} == {f: getattr(one.m[q], f) for f in METRIC_INTS}
            assert close_to(grp.m[q].ll_ref, one.m[q].ll_ref, rows) and close_to(grp.m[q].accuracy, one.m[q].accuracy, 0)
    _same((h, 0), (g, 0), rows, draws)
    g.upload_rows(0, ent, rp, y)                            # a re-upload drops the group's accumulator too
    with pytest.raises(capi.FmxError) as ei:
        g.post_accumulate(0)
    assert ei.value.code == -3
    g.post_begin(0)
    g.post_end(0)
    g.close()
    for s in shards:
        s.close()


def test_one_handle_group_forwards(capi):
    rows = 257
    ent, rp, y = make_rows(capi, rows, 91, False)
    h = handle(capi)
    g = capi.Group([h])
    h.set_params(*make_params(10, False))
    h.upload_rows(0, ent, rp, y)
    g.post_begin(0, 0)
    a = _fields(g.post_accumulate(0))
    via_group = _fields(g.post_evaluate_ex(0, POST_ALL))
    assert via_group == _fields(h.post_evaluate_ex(0, POST_ALL))
    h.post_begin(0, 0)
    assert _fields(h.post_accumulate(0)) == a
    g.post_end(0)
    g.close()
    h.close()


def test_kept_relation_blocks(capi, hs):
    rows, draws, h = 257, 3, hs[1]
    ent, rp, y, rel = _relational(capi, rows, 61)
    h.upload_block_rows(0, ent, rp, y, rel, keep=True)
    h.upload_block_rows(1, ent, rp, y, rel, keep=False)
    h.post_begin(0, 1)
    h.post_begin(1, 1)
    for d in range(draws):
        h.set_params(*make_params(7 + d, True))
        a, b = h.post_accumulate(0), h.post_accumulate(1)
        for q in WHICH:
            assert {f: getattr(a.m[q], f) for f in METRIC_INTS} == {f: getattr(b.m[q], f) for f in METRIC_INTS}
    _same((h, 0), (h, 1), rows, draws)
    oracle = PosteriorAverage(1, LO, HI, 0)
    oracle.accumulate(h.predict(0, rows))
    assert float(np.max(np.abs(h.post_get(0, POST_THIS, rows)[0] - oracle.get(POST_THIS)))) <= sum_bound(1, 1)
    h.free_rows(1)


# ---- the learners ----------------------------------------------------------------------------------------------------------------
def _separable(capi, rows, seed):
    """a toy set a linear model separates: feature 0 .. 99 in positive rows, 100 .. 198 in negative rows, plus one shared feature"""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    ent = np.zeros(2 * rows, dtype=capi.ENTRY_DTYPE)
    ent["id"][0::2] = np.where(y > 0, rng.integers(0, 100, rows), rng.integers(100, 199, rows))
    ent["id"][1::2] = N - 1
    ent["value"] = 1.0
    return ent, np.arange(0, 2 * rows + 1, 2, dtype=np.uint64), y


def _learn(L, cls, task, devices, device_average, tr, te, record=None):
    import io
    l = cls()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor = N, K
    l.fm.init(np.random.default_rng(3))
    l.task, l.num_iter, l.min_target, l.max_target = task, 8, LO, HI
    l.w_lambda = l.v_lambda = 1.0
    l.seed, l.devices, l.device_average, l.out = 5, devices, device_average, io.StringIO()
    if device_average:
        l.extra_metrics = ("auc", "logloss")
    l.init()
    if record is not None:                                  # the host route's predictions, iteration by iteration
        predict = l._h.predict
        l._h.predict = lambda slot, n: record.append(predict(slot, n)) or record[-1]
    l.learn(tr, te)
    return l


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-handle", "two-shards"])
@pytest.mark.parametrize("task", [0, 1], ids=["regression", "classification"])
@pytest.mark.parametrize("method", ["als", "mcmc"])
def test_learners_with_device_average(capi, capsys, method, task, devices):
    from libfm_amd import learner as L
    cls = L.FMLearnALS if method == "als" else L.FMLearnMCMC
    rows, iters = 200, 8
    tr, te = L.Data(*_separable(capi, rows, 1)), L.Data(*_separable(capi, rows, 2))
    host_p = []
    off = _learn(L, cls, task, devices, False, tr, te, host_p)
    capsys.readouterr()
    on = _learn(L, cls, task, devices, True, tr, te)
    err = capsys.readouterr().err
    if task == 1:                                           # no mean of the host route within 1e-9 of the 0.5 the accuracy turns on
        s = np.zeros(rows)
        for i, p in enumerate(host_p):
            s += L.cdf_gaussian(p)
            assert np.min(np.abs(s / (i + 1) - 0.5)) > 1e-9
    off_lines, on_lines = off.out.getvalue().splitlines(), on.out.getvalue().splitlines()
    print("\n".join(on_lines))
    assert len(off_lines) == len(on_lines) == iters and all(ln.startswith("#Iter=") for ln in on_lines)
    if task == 1:
        assert all(ln.count("\tTest(ll)=") == 1 for ln in on_lines)
        on_lines = [ln[:ln.index("\tTest(ll)=")] for ln in on_lines]
    assert on_lines == off_lines
    worst = float(np.max(np.abs(on.predict(te) - off.predict(te))))
    print(method, task, devices, "max |predict on - off|", worst)
    assert worst <= sum_bound(task, iters)
    names = ("this", "all", "all_but5")
    want_keys = {"rmse_mcmc_" + n for n in names} if task == 0 else {p + n for p in ("acc_mcmc_", "ll_mcmc_") for n in names}
    assert all(want_keys <= set(row) for row in on.log) and not any(want_keys & set(row) for row in off.log)
    late = on.log[4]["rmse_mcmc_all_but5" if task == 0 else "acc_mcmc_all_but5"]
    assert math.isnan(late) and not math.isnan(on.log[5]["rmse_mcmc_all_but5" if task == 0 else "acc_mcmc_all_but5"])
    with pytest.raises(NotImplementedError):
        on.evaluate_ex(tr)
    ev = on.evaluate_ex(te)
    want = posterior_evaluate_ex(task, posterior_mean(on.pred_sum_all, iters), te.target, LO, HI)
    assert {f: int(getattr(ev, f)) for f in EVAL_INTS} == {f: want[f] for f in EVAL_INTS} and ev.rows == rows
    if task == 1:
        assert on.log[-1]["auc_test"] == want["auc"] and want["auc"] > 0.5
        assert close_to(on.log[-1]["logloss_test"], want["logloss"], rows)
        assert err.count("\tauc: Test=") == iters and err.count("\tlogloss: Test=") == iters and "Train=" not in err
        assert "auc_train" not in on.log[-1]
    else:
        assert "auc:" not in err and close_to(ev.rmse, want["rmse"], rows)
    if method == "mcmc":                                    # the default keeps refusing
        with pytest.raises(NotImplementedError):
            off.evaluate_ex(te)
    off.close()
    on.close()


def _write_libfm(path, ent, rp, y):
    with open(path, "w") as f:
        for r in range(len(y)):
            f.write("%g %s\n" % (y[r], " ".join("%d:%g" % (e["id"], e["value"]) for e in ent[int(rp[r]):int(rp[r + 1])])))


def test_cli_device_average(capi, capsys, tmp_path):
    from libfm_amd import cli
    trf, tef, rlog = str(tmp_path / "tr.libfm"), str(tmp_path / "te.libfm"), str(tmp_path / "rlog.tsv")
    _write_libfm(trf, *_separable(capi, 200, 1))
    _write_libfm(tef, *_separable(capi, 200, 2))
    argv = ["-task", "c", "-train", trf, "-test", tef, "-dim", "1,1,2", "-iter", "6", "-method", "mcmc", "-init_stdev", "0.1", "-seed", "42"]
    assert cli.main(argv) == 0
    plain = capsys.readouterr()
    assert plain.out.count("#Iter=") == 6 and "Test(ll)" not in plain.out and "ERROR" not in plain.err
    assert cli.main(argv + ["-device_average", "1", "-metrics", "auc", "-rlog", rlog]) == 0
    flagged = capsys.readouterr()
    assert "ERROR" not in flagged.err and flagged.out.count("\tTest(ll)=") == 6 and flagged.err.count("\tauc: Test=") == 6
    header = open(rlog).readline().split("\t")
    assert {"auc_test", "acc_mcmc_all", "ll_mcmc_this", "acc_mcmc_all_but5"} <= {c.strip() for c in header}
