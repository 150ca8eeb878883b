"""GPU: per-row weights (fmx_set_row_weights): the weighted epochs of fmx_adapt_epoch / fmx_ftrl_epoch (k_scan_weighted) against the
float64 restatements with `weights=` (libfm_amd/adaptive.py, libfm_amd/ftrl.py; pinned in tests/test_weighted_cpu.py), the edges of
the kernel's tile pipeline, the lifetime of the weights, the refusals of the trainers without a weighted form, and
fmx_evaluate_weighted (k_evalw_score / k_evalw_final) against evalmetrics.weighted_metrics.

Tolerances.  Epochs: those of tests/test_gpu_adagrad.py and tests/test_gpu_ftrl.py -- parameters rtol 1e-4 / atol 2e-5, AdaGrad's
accumulators rtol 1e-4, FTRL's z and n rtol 1e-4 plus 8 x the gap between the restatement in fp32 and in fp64 at the test's own shape
and weights (n starts at 0).  Their argument, d(step)/dg <= eta / sqrt(init_acc), does not involve the weights;
tests/test_weighted_cpu.py::test_conditioning shows the margin at the parity shape (fp32 restatement 5.3e-7 / 5.8e-6 from the fp64 one).
fmx_evaluate_weighted: 1e-10 relative on every sum and ratio.  The device's sums differ from math.fsum's only by the order of at most
7e4 fp64 additions of non-negative terms: n * 2^-53 = 8e-12; the limit leaves one decade.  Counts are exact."""
import contextlib
import io
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_ftrl_cpu import PARITY, parity_case
from test_gpu_adagrad import check_against as check_adagrad
from test_weighted_cpu import BATCH, CHUNK, EPOCHS, ETA, GPU_CASES, LR, case_weights, repeated_set, run_rule, weighted_ftrl_gaps

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
ASSOC = 8.0                 # the device sums in another association than the fp32 restatement (tests/test_gpu_ftrl.py)
E_ARG, E_STATE, E_UNSUPPORTED = -1, -3, -4


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


def scan_tile():
    """the tile length of k_scan_weighted, from its header"""
    txt = open(os.path.join(ROOT, "libfm_amd", "csrc", "fmx_weighted_kernels.h")).read()
    return int(re.search(r"constexpr\s+int\s+SCANW_TILE\s*=\s*(\d+)\s*;", txt).group(1))


def handle_for(capi, m, task, lr=LR):
    h = capi.Handle(m.n, m.k, m.k0, m.k1, task, m.reg0, m.regw, m.regv, lr, -1.0, 1.0)
    h.set_params(m.w0, m.w, m.v)
    return h


def weighted_status(capi, es):
    assert es.status & capi.STAT_WEIGHTED and es.status & capi.STAT_SCAN_SERIAL and not es.status & capi.STAT_SCAN_PIT, es.status


def check_ftrl(h, m, st, atol_z, atol_n):
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


def device_epochs(capi, rule, d, m0, task, weights, batch=BATCH, chunk=CHUNK, epochs=EPOCHS, lr=LR, opts=None):
    """`epochs` epochs of the rule on a fresh handle; returns (handle, stats of the last epoch): the caller closes the handle"""
    h = handle_for(capi, m0, task, lr)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        if weights is not None:
            h.set_row_weights(0, weights)
        if rule == "adagrad":
            h.adapt_begin("adagrad", 1.0, ETA)
        else:
            h.ftrl_begin(**(PARITY if opts is None else opts))
        for _ in range(epochs):
            es = h.adapt_epoch(0, batch, chunk) if rule == "adagrad" else h.ftrl_epoch(0, batch, chunk)
    except Exception:
        h.close()
        raise
    return h, es


def run_parity(capi, rule, k, task, k0=True, k1=True):
    d, m0 = parity_case(k, k0, k1)
    c = case_weights(d.n_rows)
    m, st = run_rule(rule, d, m0, task, c)
    h, es = device_epochs(capi, rule, d, m0, task, c)
    try:
        assert es.rows == d.n_rows and es.batches == 8 and es.batch_used == BATCH and es.w0_chunk_used == CHUNK
        weighted_status(capi, es)
        if rule == "adagrad":
            check_adagrad(h, m, st)
        else:
            gz, gn = weighted_ftrl_gaps(d, m0, task, c)
            check_ftrl(h, m, st, ASSOC * gz, ASSOC * gn)
    finally:
        h.close()
    if k:
        assert np.abs(m.v - m0.v).max() > 1e-3                   # (three epochs moved the parameters far beyond the tolerances)
    unweighted, _ = run_rule(rule, d, m0, task, None)
    assert np.abs(m.v - unweighted.v).max() > 10 * ATOL          # (and the weights moved them far from the unweighted model)


@pytest.mark.parametrize("k, task", GPU_CASES)
@pytest.mark.parametrize("rule", ["adagrad", "ftrl"])
def test_parity(capi, rule, k, task):
    run_parity(capi, rule, k, task)


@pytest.mark.parametrize("rule", ["adagrad", "ftrl"])
def test_parity_without_linear_weights(capi, rule):
    run_parity(capi, rule, 8, 1, k1=False)


@pytest.mark.parametrize("rule", ["adagrad", "ftrl"])
def test_parity_without_bias(capi, rule):
    """k0 = False: only mult is needed, the batch is one micro-chunk"""
    run_parity(capi, rule, 8, 0, k0=False)


# ---- edges of k_scan_weighted: k = 8, 4 entries per row ---------------------------------------------------------------------------

def edge_case(oracle, rows, seed=21, n=2000, k=8):
    d = oracle.synth_rows(seed, 0, rows, 4, n)
    m = oracle.Model(n, k, True, True, 0.01, 0.002, 0.001)
    m.v[:] = oracle.init_values(1, n, k, 0.05)
    m.w[:] = oracle.init_values(2, n, 1, 0.02)[0]
    m.w0 = 0.03
    return d, m, case_weights(rows)


def run_edge(capi, oracle, rows, batch, chunk, task=1, epochs=2):
    d, m0, c = edge_case(oracle, rows)
    m, st = run_rule("adagrad", d, m0, task, c, batch=batch, chunk=chunk, epochs=epochs)
    h, es = device_epochs(capi, "adagrad", d, m0, task, c, batch=batch, chunk=chunk, epochs=epochs)
    try:
        assert es.rows == rows and es.batches == (rows + batch - 1) // batch and es.w0_chunk_used == chunk
        weighted_status(capi, es)
        check_adagrad(h, m, st)
    finally:
        h.close()
    assert abs(m.w0 - m0.w0) > 10 * ATOL


@pytest.mark.parametrize("rows", ["T-1", "T", "T+1", "2T+3"])
def test_one_batch_around_the_tile(capi, oracle, rows):
    T = scan_tile()
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[rows]
    run_edge(capi, oracle, n, n, 16)


def test_tiles_in_the_general_form(capi, oracle):
    """micro-chunk 16 above runs the sub-piece form of the kernel; 300 crosses the tile boundaries in the general one"""
    T = scan_tile()
    run_edge(capi, oracle, 2 * T + 3, 2 * T + 3, 300)


def test_batches_off_alignment(capi, oracle):
    """batch 63: every batch but the first starts off 16-byte alignment in target[] and weight[] (the dword path of the tile fetch),
    and the last batch is ragged (512 = 8 * 63 + 8)"""
    run_edge(capi, oracle, 512, 63, 16)


@pytest.mark.parametrize("task", [0, 1])
@pytest.mark.parametrize("chunk", [1, 7, 16, 32, 64, 256, 300, 700])
def test_micro_chunks(capi, oracle, chunk, task):
    """batches of 600 and 100 rows (neither a multiple of 64); 16, 32 and 64 take the kernel's sub-piece form, the others the general
    one: 256 its four-per-lane block, 300 the block and a tail, 700 is longer than the batch"""
    run_edge(capi, oracle, 700, 600, chunk, task=task)


def test_large_batch_stays_serial(capi, oracle):
    """one batch of 8192 + 100 rows at a power-of-two micro-chunk: the unweighted recurrence may run parallel in time there
    (k_scan_pit), the weighted one is the chain (weighted_status in run_edge) -- five tiles"""
    run_edge(capi, oracle, 8192 + 100, 8192 + 100, 32)


# ---- consistency ----------------------------------------------------------------------------------------------------------------

def params_and_state(h, rule, n):
    ids = np.arange(n, dtype=np.uint32)
    return h.get_params() + (h.adapt_state_rows(ids) if rule == "adagrad" else h.ftrl_state_rows(ids))


def assert_close_runs(rule, a, b, atol_state=0.0):
    """two device runs within the parity tolerances of each other: (w0, w, v) then the state tables"""
    assert abs(a[0] - b[0]) <= RTOL * abs(b[0]) + ATOL
    for x, y in zip(a[1:3], b[1:3]):
        np.testing.assert_allclose(x, y, rtol=RTOL, atol=ATOL)
    for x, y in zip(a[3:], b[3:]):
        np.testing.assert_allclose(x, y, rtol=RTOL, atol=atol_state)


@pytest.mark.parametrize("rule", ["adagrad", "ftrl"])
def test_all_ones_against_the_unweighted_epoch(capi, rule):
    """the same handle: three unweighted epochs, then parameters and session reset, all-ones weights, three weighted epochs"""
    d, m0 = parity_case(8)
    gz, gn = weighted_ftrl_gaps(d, m0, 1, np.ones(d.n_rows)) if rule == "ftrl" else (0.0, 0.0)
    h, es = device_epochs(capi, rule, d, m0, 1, None)
    try:
        assert not es.status & capi.STAT_WEIGHTED
        plain = params_and_state(h, rule, m0.n)
        h.set_params(m0.w0, m0.w, m0.v)
        h.set_row_weights(0, np.ones(d.n_rows))
        if rule == "adagrad":
            h.adapt_begin("adagrad", 1.0, ETA)
        else:
            h.ftrl_begin(**PARITY)
        for _ in range(EPOCHS):
            es = h.adapt_epoch(0, BATCH, CHUNK) if rule == "adagrad" else h.ftrl_epoch(0, BATCH, CHUNK)
        weighted_status(capi, es)
        ones = params_and_state(h, rule, m0.n)
    finally:
        h.close()
    assert np.abs(plain[2] - m0.v).max() > 1e-3
    if rule == "adagrad":
        assert_close_runs(rule, ones, plain)
    else:                                                        # z, z then n, n: the absolute terms of the parity test
        assert_close_runs(rule, ones[:3], plain[:3])
        for x, y, a in zip(ones[3:], plain[3:], (gz, gz, gn, gn)):
            np.testing.assert_allclose(x, y, rtol=RTOL, atol=ASSOC * a)


@pytest.mark.parametrize("rule", ["adagrad", "ftrl"])
def test_integer_weights_against_repeated_rows(capi, oracle, rule):
    """no regularisation, the slot one batch and one micro-chunk: integer weights 0 .. 3 on 96 rows against the set with every row
    repeated c_e times (tests/test_weighted_cpu.py::test_integer_weights_repeat_rows is the same identity in fp64, within 1e-12)"""
    n, k = 200, 8
    d = oracle.synth_rows(5, 0, 96, 6, n)
    c = np.random.default_rng(11).integers(0, 4, d.n_rows)
    rep = repeated_set(d, c)
    m0 = oracle.Model(n, k, True, True, 0.0, 0.0, 0.0)
    m0.v[:] = oracle.init_values(1, n, k, 0.05)
    m0.w[:] = oracle.init_values(2, n, 1, 0.02)[0]
    m0.w0 = 0.03
    opts = dict(alpha=0.05, beta=1.0, l1_w=0.0, l1_v=0.0, l2_w=0.0, l2_v=0.0, init_acc=0.5)
    res = []
    for data, weights in ((d, c), (rep, None)):
        h, es = device_epochs(capi, rule, data, m0, 1, weights, batch=data.n_rows, chunk=1000, opts=opts)
        try:
            assert es.batches == 1
            res.append(params_and_state(h, rule, n))
        finally:
            h.close()
    assert np.abs(res[0][2] - m0.v).max() > 1e-3
    assert_close_runs(rule, res[0], res[1], atol_state=ATOL)     # (FTRL's z passes through 0: the parameters' absolute term)


# ---- bit-exact cases ------------------------------------------------------------------------------------------------------------

def test_zero_weights_change_nothing(capi):
    """AdaGrad, every weight 0, no regularisation: g = 0 for every touched coordinate, so n' = fmaf(0, 0, n) = n and
    theta' = theta - eta * 0 / sqrt(n) = theta; the bias moves by lr * (0 + rows * 0 * w0s) = 0"""
    d, m0 = parity_case(8)
    m0.reg0 = m0.regw = m0.regv = 0.0
    h = handle_for(capi, m0, 1)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        h.set_row_weights(0, np.zeros(d.n_rows))
        h.adapt_begin("adagrad", 0.7, ETA)
        before = params_and_state(h, "adagrad", m0.n)
        for _ in range(2):
            weighted_status(capi, h.adapt_epoch(0, BATCH, CHUNK))
        after = params_and_state(h, "adagrad", m0.n)
    finally:
        h.close()
    assert after[0] == before[0] == m0.w0
    for a, b in zip(after[1:], before[1:]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("rule", ["adagrad", "ftrl"])
def test_bit_reproducible(capi, rule):
    d, m0 = parity_case(64)
    res = []
    for _ in range(2):
        h, _ = device_epochs(capi, rule, d, m0, 1, case_weights(d.n_rows), epochs=2)
        try:
            res.append(params_and_state(h, rule, m0.n))
        finally:
            h.close()
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1:], res[1][1:]):
        assert np.array_equal(a, b)


# ---- lifetime and refusals --------------------------------------------------------------------------------------------------------

def refused(capi, fn, code, *words):
    with pytest.raises(capi.FmxError) as ei:
        fn()
    assert ei.value.code == code, ei.value.text
    for w in words:
        assert w in ei.value.text, ei.value.text


def test_lifetime(capi):
    d, m0 = parity_case(8)
    c = case_weights(d.n_rows).astype(np.float32)
    h = handle_for(capi, m0, 1)
    try:
        assert h.lib.fmx_set_row_weights(h.h, 3, c.ctypes.data) == E_STATE                      # never uploaded
        assert b"fmx_set_row_weights" in h.lib.fmx_last_error(h.h)
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        refused(capi, lambda: h.get_row_weights(0), E_STATE, "fmx_get_row_weights")
        refused(capi, lambda: h.evaluate_weighted(0), E_STATE, "fmx_evaluate_weighted", "fmx_set_row_weights")
        h.set_row_weights(0, c)
        assert np.array_equal(h.get_row_weights(0), c)
        for row, bad in ((5, np.nan), (17, np.inf), (300, -1.0)):
            w = c.copy()
            w[row] = bad
            w[400] = np.nan                                      # (the FIRST offending row is named)
            refused(capi, lambda: h.set_row_weights(0, w), E_ARG, "row %d " % row)
            assert np.array_equal(h.get_row_weights(0), c)       # the old weights still stand
        h.set_row_weights(0, 2 * c)                              # a new call replaces them
        assert np.array_equal(h.get_row_weights(0), 2 * c)
        h.set_row_weights(0, None)                               # NULL drops them
        refused(capi, lambda: h.get_row_weights(0), E_STATE)
        h.set_row_weights(0, c)
        h.upload_rows(0, d.entries, d.row_ptr, d.target)         # an upload drops them
        refused(capi, lambda: h.get_row_weights(0), E_STATE)
        h.adapt_begin("adagrad", 1.0, ETA)
        assert not h.adapt_epoch(0, BATCH, CHUNK).status & capi.STAT_WEIGHTED
        h.adapt_end()
        h.upload_rows(1, d.entries[:0], np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.float32))   # an empty slot takes weights
        h.set_row_weights(1, np.zeros(0))
        assert len(h.get_row_weights(1)) == 0
        ev = h.evaluate_weighted(1)
        assert ev.rows == 0 and ev.weight_sum == 0.0 and math.isnan(ev.logloss) and math.isnan(ev.accuracy)
        h.ftrl_begin(**PARITY)
        assert h.ftrl_epoch(1, BATCH, CHUNK).rows == 0
    finally:
        h.close()


def test_trainers_without_a_weighted_form_refuse(capi):
    import torch
    d, m0 = parity_case(8)
    h = handle_for(capi, m0, 1)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
        h.upload_rows(1, d.entries, d.row_ptr, d.target)         # (an unweighted validation slot)
        nf = h.partial_floats(d.n_rows)
        buf = torch.zeros(nf, dtype=torch.float32, device=torch.device("cuda:0"))
        torch.cuda.synchronize()
        h.sgda_begin()
        calls = {
            "fmx_sgd_epoch": lambda: h.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, BATCH, CHUNK),
            "fmx_sgd_partial": lambda: h.sgd_partial(0, 0, d.n_rows, buf.data_ptr()),
            "fmx_sgd_finish": lambda: h.sgd_finish(0, 0, d.n_rows, buf.data_ptr(), w0_chunk=CHUNK),
            "fmx_sgda_epoch": lambda: h.sgda_epoch(0, 1, True),
            "fmx_sgda_epoch_minibatch": lambda: h.sgda_epoch_minibatch(0, 1, True, BATCH, CHUNK),
        }
        h.set_row_weights(0, case_weights(d.n_rows))
        before = h.get_params()
        for name, call in calls.items():
            refused(capi, call, E_UNSUPPORTED, name, "fmx_set_row_weights")
        h.sgda_epoch(1, 0, True)                                 # weights on the VALIDATION slot are not in the way
        h.set_params(*before)
        h.sgda_end()
        refused(capi, lambda: h.als_begin(0), E_UNSUPPORTED, "fmx_als_begin", "fmx_set_row_weights")
        after = h.get_params()
        assert after[0] == before[0] and all(np.array_equal(a, b) for a, b in zip(after[1:], before[1:]))   # refused before any launch
        assert h.evaluate_ex(0).rows == d.n_rows and len(h.predict(0, d.n_rows)) == d.n_rows               # scoring ignores the weights
        h.set_row_weights(0, None)                               # after the drop every one of them runs
        h.sgda_begin()
        for name, call in calls.items():
            call()
            h.synchronize()
        h.sgda_end()
        h.als_begin(0)
        h.als_end()
        assert np.isfinite(h.get_params()[2]).all()
    finally:
        h.close()


# ---- fmx_evaluate_weighted ----------------------------------------------------------------------------------------------------------

EW_N, EW_K = 500, 4
EW_SUMS = ("weight_sum", "pos_weight", "neg_weight", "correct_weight", "loss_sum", "sq_sum", "abs_sum")
EW_RATIOS = ("logloss", "rmse", "mae", "accuracy")


def ew_handle(capi, oracle, task, rows, seed=3):
    rng = np.random.default_rng(100 + seed)
    h = capi.Handle(EW_N, EW_K, True, True, task, 0.0, 0.0, 0.0, 0.01, -1.0, 1.0)
    h.set_params(0.07, rng.normal(0, 0.6, EW_N), rng.normal(0, 0.6, (EW_K, EW_N)))
    d = oracle.synth_rows(seed, 0, rows, 3, EW_N)
    y = d.target if task == 1 else rng.normal(0, 0.7, rows).astype(np.float32)
    h.upload_rows(0, d.entries, d.row_ptr, y)
    return h, d, y


def ew_check(ev, want):
    print({f: getattr(ev, f) for f in EW_SUMS + EW_RATIOS}, "restatement", {f: want[f] for f in EW_SUMS + EW_RATIOS})
    assert (ev.rows, ev.nan_rows) == (want["rows"], want["nan_rows"])
    for f in EW_SUMS + EW_RATIOS:
        got, w = getattr(ev, f), want[f]
        if math.isnan(w) or math.isinf(w):
            assert (math.isnan(got) and math.isnan(w)) or got == w, f
        else:
            assert abs(got - w) <= 1e-10 * abs(w), (f, got, w)


def ew_fields(ev):
    return [np.float64(getattr(ev, f)).tobytes() for f in EW_SUMS + EW_RATIOS] + [ev.rows, ev.nan_rows]


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 70000])
@pytest.mark.parametrize("link, task", [("logistic", 1), ("probit", 1), ("logistic", 0)], ids=["logistic", "probit", "regression"])
def test_evaluate_weighted(capi, oracle, rows, link, task):
    from libfm_amd.evalmetrics import weighted_metrics
    h, d, y = ew_handle(capi, oracle, task, rows)
    try:
        c = case_weights(rows)
        if rows == 1:
            c[:] = 1.5
        h.set_row_weights(0, c)
        ev = h.evaluate_weighted(0, capi.LINK_LOGISTIC if link == "logistic" else capi.LINK_PROBIT)
        want = weighted_metrics(h.predict(0, rows), y, c, link, task, -1.0, 1.0)
        ew_check(ev, want)
        assert ev.weight_sum > 0 and ev.device_seconds > 0
        assert not math.isnan(ev.logloss if task else ev.rmse)
        again = h.evaluate_weighted(0, capi.LINK_LOGISTIC if link == "logistic" else capi.LINK_PROBIT)
        assert ew_fields(again) == ew_fields(ev)                 # two calls are bit-identical
        ex = h.evaluate_ex(0)                                    # (the unweighted metrics do not see the weights)
        assert ex.rows == rows
    finally:
        h.close()


def test_evaluate_weighted_nan_score_and_zero_weights(capi, oracle):
    from libfm_amd.evalmetrics import weighted_metrics
    rows, j = 1000, 17
    h, d, y = ew_handle(capi, oracle, 1, rows)
    try:
        c = case_weights(rows)
        h.set_row_weights(0, c)
        w0, w, v = h.get_params()
        w[j] = np.nan
        h.set_params(w0, w, v)
        p = h.predict(0, rows)
        assert 0 < np.isnan(p).sum() < rows
        ev = h.evaluate_weighted(0)
        want = weighted_metrics(p, y, c)
        ew_check(ev, want)
        assert ev.nan_rows == int(np.isnan(p).sum()) and math.isnan(ev.logloss) and math.isnan(ev.accuracy)
        assert ev.weight_sum > 0 and ev.correct_weight > 0
        c0 = np.where(np.isnan(p), 0.0, c)                       # the NaN rows at weight 0: they add nothing, but still count
        h.set_row_weights(0, c0)
        ev = h.evaluate_weighted(0)
        ew_check(ev, weighted_metrics(p, y, c0))
        assert ev.nan_rows > 0 and math.isfinite(ev.loss_sum) and math.isnan(ev.logloss)
        w[j] = 0.0
        h.set_params(w0, w, v)
        h.set_row_weights(0, np.zeros(rows))                     # every weight 0
        ev = h.evaluate_weighted(0)
        assert (ev.rows, ev.nan_rows, ev.weight_sum, ev.loss_sum, ev.correct_weight) == (rows, 0, 0.0, 0.0, 0.0)
        assert math.isnan(ev.logloss) and math.isnan(ev.accuracy)
    finally:
        h.close()


# ---- the learner and the command line ---------------------------------------------------------------------------------------------

def _separable(capi, rows, seed):
    """a toy set a linear model separates: feature 0 .. 24 in positive rows, 25 .. 49 in negative rows, plus one shared feature"""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    ent = np.zeros(2 * rows, dtype=capi.ENTRY_DTYPE)
    ent["id"][0::2] = np.where(y > 0, rng.integers(0, 24, rows), rng.integers(25, 49, rows))
    ent["id"][1::2] = 49
    ent["value"] = 1.0
    return ent, np.arange(0, 2 * rows + 1, 2, dtype=np.uint64), y


def _write_libfm(path, ent, rp, y):
    with open(path, "w") as f:
        for r in range(len(y)):
            f.write("%g %s\n" % (y[r], " ".join("%d:%g" % (e["id"], e["value"]) for e in ent[int(rp[r]):int(rp[r + 1])])))


def test_learner_weights(capi, capsys):
    from libfm_amd import learner as L
    from libfm_amd.evalmetrics import weighted_metrics
    tr, te = L.Data(*_separable(capi, 200, 1)), L.Data(*_separable(capi, 200, 2))
    ctr, cte = np.where(tr.target < 0, 4.0, 1.0), np.where(te.target < 0, 4.0, 1.0)

    def learner(optimizer):
        l = L.FMLearnSGD()
        l.fm = L.FMModel()
        l.fm.num_attribute, l.fm.num_factor = 64, 4
        l.fm.init(np.random.default_rng(3))
        l.task, l.learn_rate, l.num_iter, l.min_target, l.max_target = L.TASK_CLASSIFICATION, 0.05, 3, -1.0, 1.0
        l.optimizer, l.batch, l.out = optimizer, 64, io.StringIO()
        l.extra_metrics = ("logloss", "wlogloss")
        l.init()
        l.set_weights(tr, ctr)
        return l
    l = learner("sgd")
    with pytest.raises(ValueError, match="set_weights"):
        l.learn(tr, te)
    l.close()
    l = learner("ftrl")
    l.learn(tr, te)                                              # the test set carries no weights yet: nan
    assert math.isnan(l.log[-1]["wlogloss_test"]) and l.log[-1]["wlogloss_train"] > 0
    l.set_weights(te, cte)                                       # attached to the set's slot after the upload
    want = weighted_metrics(l.predict_raw(te), te.target, cte)
    got = l.evaluate_weighted(te)
    assert abs(got.logloss - want["logloss"]) <= 1e-10 * want["logloss"] and got.weight_sum == float(cte.sum())
    assert abs(l.log[-1]["wlogloss_train"] - weighted_metrics(l.predict_raw(tr), tr.target, ctr)["logloss"]) <= 1e-10
    assert capsys.readouterr().err.count("\twlogloss: Train=") == 3
    l.close()


def test_cli_weights_flags(capi, tmp_path, capsys):
    from libfm_amd import cli
    trf, tef, trw, tew = (str(tmp_path / f) for f in ("tr.libfm", "te.libfm", "tr.w", "te.w"))
    tr, te = _separable(capi, 200, 1), _separable(capi, 200, 2)
    _write_libfm(trf, *tr)
    _write_libfm(tef, *te)
    for path, y in ((trw, tr[2]), (tew, te[2])):
        with open(path, "w") as f:
            f.write("".join("%g\n" % (4.0 if t < 0 else 1.0) for t in y))
    argv = ["-task", "c", "-train", trf, "-test", tef, "-dim", "1,1,2", "-iter", "3", "-method", "sgd", "-learn_rate", "0.05",
            "-init_stdev", "0.1", "-seed", "42", "-optimizer", "adagrad", "-batch", "64"]
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(argv) == 0
        plain = capsys.readouterr()
        assert cli.main(argv + ["-train_weights", trw, "-test_weights", tew, "-metrics", "logloss,wlogloss"]) == 0
        flagged = capsys.readouterr()
        assert "ERROR" not in plain.err and "ERROR" not in flagged.err
        assert flagged.err.count("\twlogloss: Train=") == 3 and flagged.err.count("\tlogloss: Train=") == 3
        assert "nan" not in flagged.err
        for extra, word in ((["-optimizer", "sgd"], "weighted form"), (["-method", "als"], "")):
            assert cli.main(argv + ["-train_weights", trw] + extra) == 0          # (a repeated flag: the later value holds)
            err = capsys.readouterr().err
            assert "ERROR:" in err and word in err
        assert cli.main(argv + ["-metrics", "wlogloss"]) == 0
        assert "-train_weights" in capsys.readouterr().err
        with open(trw, "a") as f:
            f.write("-1\n")
        assert cli.main(argv + ["-train_weights", trw]) == 0
        assert "ERROR:" in capsys.readouterr().err
