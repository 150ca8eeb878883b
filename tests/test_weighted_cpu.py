"""CPU: per-row weights in the restatements of the AdaGrad and FTRL epochs (libfm_amd/adaptive.py, libfm_amd/ftrl.py, `weights=`) and
the restatement of fmx_evaluate_weighted (evalmetrics.weighted_metrics) -- what tests/test_gpu_weighted.py holds the device to.

The rule (include/fmx.h "per-row weights"): m_e = c_e * multiplier in the working dtype, c_e rounded to float32 first; the bias and
the owners then see m_e.  The regularisation terms count occurrences and rows, not weight.

test_conditioning shows the margin of the GPU file's tolerances at its own shape and weights: the restatement run in fp32 sits at
least 10 x inside the tolerance the device is held to against the fp64 one.  Measured: AdaGrad parameters <= 5.3e-7 absolute,
accumulators <= 5.8e-6 relative; FTRL parameters <= 3e-7 (the bound is 2e-5 + 1e-4 |x| and 1e-4 relative)."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from test_ftrl_cpu import PARITY, parity_case

RTOL, ATOL = 1e-4, 2e-5                                 # tests/test_gpu_adagrad.py, tests/test_gpu_ftrl.py
LR, ETA = 0.01, 0.05
BATCH, CHUNK, EPOCHS = 64, 16, 3
GPU_CASES = [(1, 0), (8, 1), (64, 0), (64, 1), (100, 1), (128, 0)]      # (k, task) of the GPU parity tests
RULES = ("adagrad", "ftrl")


def case_weights(rows=512):
    return np.random.default_rng(3).choice([0, .5, .75, 1, 1, 1.25, 1.5, 2], rows)


def run_rule(rule, d, m0, task, weights, dtype=np.float64, epochs=EPOCHS, batch=BATCH, chunk=CHUNK, lr=LR, opts=None):
    """`epochs` epochs of the restatement from a copy of m0: (model, state)"""
    from libfm_amd import adaptive, ftrl
    m = m0.copy()
    if rule == "adagrad":
        st = adaptive.AdaptState(m.n, m.k, 1.0)
        for _ in range(epochs):
            adaptive.epoch(m, d, task, lr, -1.0, 1.0, batch, chunk, st, eta=ETA, dtype=dtype, weights=weights)
    else:
        st = ftrl.FtrlState(m, **(PARITY if opts is None else opts))
        for _ in range(epochs):
            ftrl.epoch(m, d, task, lr, -1.0, 1.0, batch, chunk, st, dtype=dtype, weights=weights)
    return m, st


def state_arrays(rule, st):
    return (st.n_w, st.n_v) if rule == "adagrad" else (st.z_w, st.z_v, st.n_w, st.n_v)


def weighted_ftrl_gaps(d, m0, task, weights, opts=None, **kw):
    """largest absolute gaps (z, n) between the weighted FTRL restatement in fp32 and in fp64: the absolute term of the device's state
    tolerance, as tests/test_ftrl_cpu.ftrl_gaps gives it for the unweighted epochs (n starts at 0: no relative bound exists)"""
    (_, a), (_, b) = (run_rule("ftrl", d, m0, task, weights, dt, opts=opts, **kw) for dt in (np.float64, np.float32))

    def gap(x, y):
        return float(np.abs(x - y).max()) if x.size else 0.0
    return max(gap(a.z_v, b.z_v), gap(a.z_w, b.z_w)), max(gap(a.n_v, b.n_v), gap(a.n_w, b.n_w))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("task", [0, 1])
def test_all_ones_is_the_unweighted_epoch(rule, dtype, task):
    d, m0 = parity_case(8)
    a, sa = run_rule(rule, d, m0, task, None, dtype, epochs=2)
    b, sb = run_rule(rule, d, m0, task, np.ones(d.n_rows), dtype, epochs=2)
    assert a.w0 == b.w0 and np.array_equal(a.w, b.w) and np.array_equal(a.v, b.v)
    for x, y in zip(state_arrays(rule, sa), state_arrays(rule, sb)):
        assert np.array_equal(x, y)
    c, _ = run_rule(rule, d, m0, task, case_weights(), dtype, epochs=2)
    assert np.abs(c.v - a.v).max() > 1e-4                        # (and weights that are not all ones do change the model)


def repeated_set(d, c):
    """the set in which row e stands c[e] times, in row order"""
    rp = d.row_ptr.astype(np.int64)
    rows = [[(int(i), float(x)) for i, x in d.entries[rp[e]:rp[e + 1]]] for e in range(d.n_rows)]
    rep = [e for e in range(d.n_rows) for _ in range(int(c[e]))]
    return O.Data.from_rows([rows[e] for e in rep], d.target[rep])


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("task", [0, 1])
def test_integer_weights_repeat_rows(rule, task):
    """no regularisation, the whole set one batch and one micro-chunk: weight c_e = the row repeated c_e times (every sum of the rule is
    then a sum over rows of c_e times the row's term)"""
    n, k = 200, 4
    d = O.synth_rows(5, 0, 96, 6, n)
    c = np.random.default_rng(11).integers(0, 4, d.n_rows)
    assert (c == 0).any() and (c == 3).any()
    m0 = O.Model(n, k, True, True, 0.0, 0.0, 0.0)
    m0.v[:] = O.init_values(1, n, k, 0.05)
    m0.w[:] = O.init_values(2, n, 1, 0.02)[0]
    m0.w0 = 0.03
    opts = dict(alpha=0.05, beta=1.0, l1_w=0.0, l1_v=0.0, l2_w=0.0, l2_v=0.0, init_acc=0.5)
    a, sa = run_rule(rule, d, m0, task, c, batch=0, chunk=0, opts=opts)
    b, sb = run_rule(rule, repeated_set(d, c), m0, task, None, batch=0, chunk=0, opts=opts)
    gaps = [abs(a.w0 - b.w0), np.abs(a.w - b.w).max(), np.abs(a.v - b.v).max()]
    gaps += [np.abs(x - y).max() for x, y in zip(state_arrays(rule, sa), state_arrays(rule, sb))]
    print("largest gap %.3g" % max(gaps))
    assert max(gaps) <= 1e-12
    assert np.abs(a.v - m0.v).max() > 1e-3


def two_rows():
    """rows {0: 1} and {0: 2}, targets +1 / -1, weights 2 and 0.5; regression in [-1, 1]; w0 = 0.5, w_0 = 0.1, no factors;
    lr = 0.1, reg0 = 0.1, one batch, micro-chunk 1.  By hand:
      rest = (0.1, 0.2)
      row 0: w0s = 0.5    p = 0.6    m = 2   (0.6 - 1)   = -0.8      w0 = 0.5   - 0.1 (-0.8   + 0.1 * 0.5)   = 0.575
      row 1: w0s = 0.575  p = 0.775  m = 0.5 (0.775 + 1) =  0.8875   w0 = 0.575 - 0.1 (0.8875 + 0.1 * 0.575) = 0.4805
      sum_occ m x = -0.8 * 1 + 0.8875 * 2 = 0.975"""
    d = O.Data.from_rows([[(0, 1.0)], [(0, 2.0)]], np.array([1.0, -1.0], dtype=np.float32))
    m = O.Model(1, 0, True, True, 0.1, 0.01, 0.0)
    m.w0, m.w[0] = 0.5, 0.1
    return d, m, np.array([2.0, 0.5])


def test_two_rows_by_hand_adagrad():
    """g_w = 0.975 + 2 occurrences * regw 0.01 * 0.1 = 0.977;  n = 1 + 0.977^2 = 1.954529;  w = 0.1 - 0.05 * 0.977 / sqrt(1.954529)"""
    from libfm_amd import adaptive
    d, m, c = two_rows()
    st = adaptive.AdaptState(1, 0, 1.0)
    adaptive.epoch(m, d, 0, 0.1, -1.0, 1.0, 0, 1, st, eta=0.05, weights=c)
    assert m.w0 == pytest.approx(0.4805, abs=1e-15)
    assert st.n_w[0] == pytest.approx(1.954529, abs=1e-14)
    assert m.w[0] == pytest.approx(0.1 - 0.05 * 0.977 / math.sqrt(1.954529), abs=1e-15)      # = 0.0650583419900...
    assert m.w[0] == pytest.approx(0.06505834199, abs=1e-11)


def test_two_rows_by_hand_ftrl():
    """alpha 0.05, beta 1, l1 0.1, l2 0.01, n_0 = 0:  D_0 = 1 / 0.05 + 0.01 = 20.01,  z_0 = -0.1 * 20.01 - 0.1 = -2.101
    g = 0.975 (no regularisation term);  n' = 0.950625,  sqrt = 0.975,  sigma = 0.975 / 0.05 = 19.5
    z' = -2.101 + 0.975 - 19.5 * 0.1 = -3.076;  D' = 1.975 / 0.05 + 0.01 = 39.51;  w = (3.076 - 0.1) / 39.51 = 0.0753227..."""
    from libfm_amd import ftrl
    d, m, c = two_rows()
    st = ftrl.FtrlState(m, alpha=0.05, beta=1.0, l1_w=0.1, l1_v=0.0, l2_w=0.01, l2_v=0.0, init_acc=0.0)
    assert st.z_w[0] == pytest.approx(-2.101, abs=1e-14)
    ftrl.epoch(m, d, 0, 0.1, -1.0, 1.0, 0, 1, st, weights=c)
    assert m.w0 == pytest.approx(0.4805, abs=1e-15)
    assert st.n_w[0] == pytest.approx(0.950625, abs=1e-14)
    assert st.z_w[0] == pytest.approx(-3.076, abs=1e-13)
    assert m.w[0] == pytest.approx(2.976 / 39.51, abs=1e-14)


def test_weights_are_checked():
    from libfm_amd import adaptive
    d, m, _ = two_rows()
    st = adaptive.AdaptState(1, 0, 1.0)
    for bad in ([1.0, -1.0], [1.0, math.nan], [math.inf, 1.0], [1.0]):
        with pytest.raises(ValueError):
            adaptive.epoch(m, d, 0, 0.1, -1.0, 1.0, 0, 1, st, weights=bad)


# ---- weighted_metrics against literals ---------------------------------------------------------------------------------------

def test_weighted_metrics_logistic_literal():
    """scores (0, ln 3, -ln 3), targets (+1, -1, -1), weights (2, 1, 0.5): l = ln 2, ln 4, ln(4/3)"""
    from libfm_amd.evalmetrics import weighted_metrics
    r = weighted_metrics([0.0, math.log(3.0), -math.log(3.0)], [1, -1, -1], [2, 1, 0.5])
    assert (r["rows"], r["nan_rows"]) == (3, 0)
    assert (r["weight_sum"], r["pos_weight"], r["neg_weight"], r["correct_weight"]) == (3.5, 2.0, 1.5, 2.5)
    want = 2 * math.log(2.0) + math.log(4.0) + 0.5 * math.log(4.0 / 3.0)
    assert r["loss_sum"] == pytest.approx(want, rel=1e-7)       # (the scores pass through float32)
    assert r["logloss"] == pytest.approx(want / 3.5, rel=1e-7)
    assert r["accuracy"] == 2.5 / 3.5


def test_weighted_metrics_zero_weight_row_with_infinite_loss():
    """probit at z = -40: erfc underflows, l = +inf; with weight 0 the row adds exactly 0"""
    from libfm_amd.evalmetrics import loss_term, weighted_metrics
    assert loss_term(-40.0, "probit") == math.inf
    r = weighted_metrics([-40.0, 0.0], [1, 1], [0.0, 3.0], link="probit")
    assert r["loss_sum"] == pytest.approx(3.0 * math.log(2.0), rel=1e-15)
    assert r["logloss"] == pytest.approx(math.log(2.0), rel=1e-15)
    assert (r["weight_sum"], r["pos_weight"], r["correct_weight"], r["accuracy"]) == (3.0, 3.0, 3.0, 1.0)
    r = weighted_metrics([-40.0, 0.0], [1, 1], [1.0, 3.0], link="probit")
    assert r["loss_sum"] == math.inf and r["logloss"] == math.inf


def test_weighted_metrics_probit_literal():
    from libfm_amd.evalmetrics import weighted_metrics
    r = weighted_metrics([1.0, 1.0], [1, -1], [1.0, 2.0], link="probit")
    phi = 0.5 * math.erfc(-1.0 / math.sqrt(2.0))                 # Phi(1) = 0.8413447460685429
    assert phi == pytest.approx(0.8413447460685429, rel=1e-15)
    assert r["logloss"] == pytest.approx((-math.log(phi) - 2.0 * math.log(1.0 - phi)) / 3.0, rel=1e-12)
    assert r["accuracy"] == 1.0 / 3.0


def test_weighted_metrics_zero_weight_sum_and_nan_score():
    from libfm_amd.evalmetrics import weighted_metrics
    r = weighted_metrics([0.5, -0.5], [1, -1], [0.0, 0.0])
    assert r["weight_sum"] == 0.0 and r["loss_sum"] == 0.0 and r["rows"] == 2
    assert math.isnan(r["logloss"]) and math.isnan(r["accuracy"])
    r = weighted_metrics([math.nan, 1.0, -1.0], [1, 1, 1], [0.0, 1.0, 2.0])
    assert (r["rows"], r["nan_rows"]) == (3, 1)                  # a NaN score counts whatever its weight ...
    assert (r["weight_sum"], r["pos_weight"], r["neg_weight"], r["correct_weight"]) == (3.0, 3.0, 0.0, 1.0)
    assert math.isnan(r["logloss"]) and math.isnan(r["accuracy"])   # ... and makes the ratios NaN
    assert r["loss_sum"] == pytest.approx(math.log1p(math.exp(-1.0)) + 2.0 * (1.0 + math.log1p(math.exp(-1.0))), rel=1e-15)
    r = weighted_metrics([math.nan, 1.0], [-1, 1], [1.0, 1.0])
    assert r["correct_weight"] == 1.0 and math.isnan(r["loss_sum"])   # a NaN score is never correct


def test_weighted_metrics_regression_literal():
    """scores (0.5, 3, -2) clamp to (0.5, 1, -1) in [-1, 1]; targets (1, 0, -1); weights (1, 2, 0): err = (-0.5, 1, 0)"""
    from libfm_amd.evalmetrics import weighted_metrics
    r = weighted_metrics([0.5, 3.0, -2.0], [1.0, 0.0, -1.0], [1.0, 2.0, 0.0], task=0, min_target=-1.0, max_target=1.0)
    assert (r["weight_sum"], r["sq_sum"], r["abs_sum"]) == (3.0, 2.25, 2.5)
    assert r["rmse"] == math.sqrt(0.75) and r["mae"] == 2.5 / 3.0
    assert math.isnan(r["logloss"]) and math.isnan(r["accuracy"]) and r["nan_rows"] == 0
    with pytest.raises(ValueError):
        weighted_metrics([0.0], [1.0], [-1.0])
    with pytest.raises(ValueError):
        weighted_metrics([0.0], [1.0], [1.0], link="cauchy")


# ---- conditioning of the GPU cases -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("k, task", GPU_CASES)
def test_conditioning(rule, k, task):
    """the shape, start model, batch, micro-chunk, epochs and weights of tests/test_gpu_weighted.py's parity cases: fp32 against fp64
    at least 10 x inside the device's tolerance -- parameters rtol 1e-4 / atol 2e-5 under both rules, AdaGrad's accumulators rtol 1e-4.
    FTRL's z and n have no such bound to be inside of: n starts at 0, so the device's tolerance on them IS 8 x this fp32 gap
    (weighted_ftrl_gaps, as in tests/test_gpu_ftrl.py); what is asserted for them is that this gap stays what fp32 rounding explains:
    a coordinate's z and n take at most 3 epochs x 8 batches = 24 steps of a few fp32 operations each on values of |z| <= 8
    ((beta + 1) / alpha x |theta| + l1) and n <= 2, so 24 x 4 x 2^-24 x 8 = 4.6e-5 bounds the drift; 1e-4 is that with a factor 2.
    Measured: z <= 9.6e-6, n <= 1.9e-5 (tests/test_gpu_ftrl.py reports 3.7e-6 / 9.3e-6 for the unweighted epochs)."""
    d, m0 = parity_case(k)
    c = case_weights(d.n_rows)
    a, sa = run_rule(rule, d, m0, task, c, np.float64)
    b, sb = run_rule(rule, d, m0, task, c, np.float32)
    gp = max(np.abs(a.v - b.v).max(), np.abs(a.w - b.w).max(), abs(a.w0 - b.w0))
    print("%s k %d task %d: parameters %.3g" % (rule, k, task, gp))
    for x, y in ((a.v, b.v), (a.w, b.w), (np.array([a.w0]), np.array([b.w0]))):
        assert np.all(np.abs(x - y) <= (RTOL * np.abs(x) + ATOL) / 10.0)
    if rule == "adagrad":
        gn = max((np.abs(sa.n_v - sb.n_v) / sa.n_v).max(), (np.abs(sa.n_w - sb.n_w) / sa.n_w).max())
        print("accumulators (relative) %.3g" % gn)
        assert gn <= RTOL / 10.0
    else:
        gz = max(np.abs(sa.z_v - sb.z_v).max(), np.abs(sa.z_w - sb.z_w).max())
        gn = max(np.abs(sa.n_v - sb.n_v).max(), np.abs(sa.n_w - sb.n_w).max())
        print("z %.3g  n %.3g" % (gz, gn))
        assert gz <= 1e-4 and gn <= 1e-4
    assert np.abs(a.v - m0.v).max() > 1e-3
