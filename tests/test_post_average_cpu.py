"""CPU: libfm_amd.evalmetrics.PosteriorAverage -- the restatement of the posterior accumulator (include/fmx.h "fmx_post_*",
DESIGN.md section 15) that tests/test_gpu_post_average.py holds the device to -- against literals worked out by hand and a plain
Python double loop in the shape of fm_learn_mcmc_simultaneous.h:127-161, 272-309; the range and monotonicity of
ref_cdf_gaussian, which the device's 64-bit sort keys rest on; the CLI's refusals; and the exported symbols."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from libfm_amd import evalmetrics as E
from libfm_amd.evalmetrics import POST_ALL, POST_LATE, POST_THIS, PosteriorAverage, ref_cdf_gaussian

INF, NAN = float("inf"), float("nan")
REG, CLS = E.TASK_REGRESSION, E.TASK_CLASSIFICATION
POST_FUNCTIONS = ["fmx_post_begin", "fmx_post_accumulate", "fmx_post_evaluate_ex", "fmx_post_get", "fmx_post_end"]


# ---- a hand-sized case: 4 rows, 7 draws, burn_in = 5, regression with targets clamped to [-2, 2], dyadic numbers ---------------
def hand_draw(d):
    return [0.5 * d - 1.0, 3.0, -0.25, 0.125 * (d + 1)]           # row 1 is always clamped to 2


HAND_Y = [1.0, 2.0, 0.0, 0.5]


def test_hand_sized_case():
    pa = PosteriorAverage(REG, -2.0, 2.0, burn_in=5)
    for d in range(4):
        pa.accumulate(hand_draw(d))
    assert (pa.draws, pa.late_draws) == (4, 0)
    late = pa.metric(POST_LATE, HAND_Y)                               # no late draw yet: rows = 0, every metric NaN
    assert late["rows"] == 0 and all(math.isnan(late[k]) for k in ("rmse", "mae", "accuracy", "ll_ref"))
    assert pa.evaluate_ex(POST_LATE, HAND_Y)["rows"] == 0 and pa.mean(POST_LATE) is None
    assert list(pa.get(POST_LATE)) == [0.0] * 4
    assert list(pa.get(POST_ALL)) == [-1.0, 8.0, -1.0, 1.25]          # -1 - .5 + 0 + .5; 4 * 2; 4 * -.25; .125 * (1 + 2 + 3 + 4)
    m = pa.metric(POST_ALL, HAND_Y)                                   # means -.25, 2, -.25, .3125 (1 / 4 is exact)
    assert m["rows"] == 4 and m["nan_rows"] == 0
    assert m["mae"] == (1.25 + 0 + 0.25 + 0.1875) / 4
    assert m["rmse"] == math.sqrt((1.5625 + 0 + 0.0625 + 0.03515625) / 4)
    for d in range(4, 7):
        pa.accumulate(hand_draw(d))
    assert (pa.draws, pa.late_draws) == (7, 2)
    assert list(pa.get(POST_THIS)) == [2.0, 3.0, -0.25, 0.875]        # the raw draw: the clamp belongs to the sums and the metric
    assert list(pa.get(POST_ALL)) == [3.5, 14.0, -1.75, 3.5]
    assert list(pa.get(POST_LATE)) == [3.5, 4.0, -0.5, 1.625]         # draws 5 and 6
    assert (pa.count(POST_THIS), pa.count(POST_ALL), pa.count(POST_LATE)) == (1, 7, 2)
    this = pa.metric(POST_THIS, HAND_Y)                               # clamped: 2, 2, -.25, .875 -> errors 1, 0, -.25, .375
    assert this["mae"] == 1.625 / 4 and this["rmse"] == math.sqrt(1.203125 / 4)
    late = pa.metric(POST_LATE, HAND_Y)                               # means 1.75, 2, -.25, .8125 -> errors .75, 0, -.25, .3125
    assert late["rows"] == 4 and late["mae"] == 1.3125 / 4 and late["rmse"] == math.sqrt(0.72265625 / 4)
    m = pa.metric(POST_ALL, HAND_Y)                                   # means .5, 2, -.25, .5 up to the rounding of 1 / 7
    assert m["mae"] == pytest.approx(0.75 / 4, rel=1e-15) and m["rmse"] == pytest.approx(math.sqrt(0.3125 / 4), rel=1e-15)
    assert list(pa.mean(POST_ALL)) == [3.5 * (1.0 / 7), 14.0 * (1.0 / 7), -1.75 * (1.0 / 7), 3.5 * (1.0 / 7)]   # a product, not a division
    ex = pa.evaluate_ex(POST_ALL, HAND_Y)
    assert ex["rows"] == 4 and ex["rmse"] == m["rmse"] and ex["mae"] == m["mae"]
    assert math.isnan(ex["auc"]) and math.isnan(ex["logloss"]) and (ex["pos"], ex["neg"], ex["correct"], ex["auc_num2"]) == (0, 0, 0, 0)
    assert m["accuracy"] == 0.0 and m["ll_ref"] == 0.0 and m["correct"] == 0     # the other task's metrics are 0


def test_eval_rows_cover_a_prefix():
    pa = PosteriorAverage(REG, -2.0, 2.0, burn_in=0, eval_rows=2)
    pa.accumulate(hand_draw(2))                                       # 0, 3 -> 2, -.25, .375
    m = pa.metric(POST_LATE, HAND_Y)
    assert m["rows"] == 2 and m["mae"] == (1.0 + 0.0) / 2 and pa.late_draws == 1
    assert len(pa.get(POST_ALL)) == 4                                 # the sums cover every row


# ---- the reference's loops, written out ------------------------------------------------------------------------------------------
def py_cdf(x):
    x = 0.707106781 * x
    t = 1.0 / (1.0 + 0.3275911 * x) if x >= 0 else 1.0 / (1.0 - 0.3275911 * x)
    r = 1.0 - (t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))) * math.exp(-x * x)
    return 0.5 + 0.5 * (r if x >= 0 else -r)


def loop_reference(task, draws, y, lo, hi, burn_in, n_eval):
    """pred_this / pred_sum_all / pred_sum_all_but5 and the metrics of the three, loop by loop"""
    n = len(y)
    this, s_all, s_late, late_draws = [0.0] * n, [0.0] * n, [0.0] * n, 0
    for i, p32 in enumerate(draws):
        for c in range(n):
            p = float(p32[c])
            if task == REG:
                this[c] = p
                p = max(lo, min(hi, p))
            else:
                p = this[c] = py_cdf(p)
            s_all[c] += p
            if i >= burn_in:
                s_late[c] += p
        late_draws += i >= burn_in
    out = {}
    for which, vec, cnt in ((POST_THIS, this, 1), (POST_ALL, s_all, len(draws)), (POST_LATE, s_late, late_draws)):
        if cnt == 0:
            out[which] = None
            continue
        norm, se, ae, ll, ok = 1.0 / cnt, 0.0, 0.0, 0.0, 0
        for c in range(n_eval):
            p = vec[c] * norm
            if task == REG:
                err = max(lo, min(hi, p)) - y[c]
                se += err * err
                ae += abs(err)
            else:
                ok += (p >= 0.5 and y[c] > 0) or (p < 0.5 and y[c] < 0)
                m = (y[c] + 1.0) * 0.5
                pll = min(0.99, max(0.01, p))
                ll -= m * math.log10(pll) + (1 - m) * math.log10(1 - pll)
        out[which] = {"vec": vec, "rmse": math.sqrt(se / n_eval), "mae": ae / n_eval, "ll_ref": ll / n_eval, "correct": ok}
    return out


@pytest.mark.parametrize("task", [REG, CLS])
@pytest.mark.parametrize("seed", range(6))
def test_against_the_double_loop(task, seed):
    rng = np.random.default_rng(100 * task + seed)
    n, n_draws, burn_in = int(rng.integers(1, 40)), int(rng.integers(1, 10)), int(rng.integers(0, 7))
    n_eval = int(rng.integers(1, n + 1))
    draws = [rng.normal(0, 1.5, n).astype(np.float32) for _ in range(n_draws)]
    y = [float(t) for t in (rng.normal(0, 1, n).astype(np.float32) if task == REG else np.where(rng.random(n) < 0.5, 1.0, -1.0))]
    pa = PosteriorAverage(task, -1.0, 1.0, burn_in=burn_in, eval_rows=n_eval)
    for p in draws:
        pa.accumulate(p)
    want = loop_reference(task, draws, y, -1.0, 1.0, burn_in, n_eval)
    sum_tol = 0.0 if task == REG else n_draws * 4 * 2.0 ** -53        # numpy's exp against math's inside the same polynomial
    for which in (POST_THIS, POST_ALL, POST_LATE):
        got = pa.metric(which, y)
        if want[which] is None:
            assert got["rows"] == 0 and math.isnan(got["rmse"])
            continue
        assert np.max(np.abs(pa.get(which) - np.array(want[which]["vec"]))) <= sum_tol
        assert got["rows"] == n_eval and got["nan_rows"] == 0
        if task == REG:
            assert got["rmse"] == pytest.approx(want[which]["rmse"], rel=1e-14)
            assert got["mae"] == pytest.approx(want[which]["mae"], rel=1e-14)
        else:
            assert got["correct"] == want[which]["correct"] and got["accuracy"] == want[which]["correct"] / n_eval
            assert got["ll_ref"] == pytest.approx(want[which]["ll_ref"], rel=1e-13)
            ex = pa.evaluate_ex(which, y)
            m = pa.mean(which)[:n_eval]
            brute = sum(2 * (m[i] > m[j]) + (m[i] == m[j]) for i in range(n_eval) if y[i] >= 0 for j in range(n_eval) if y[j] < 0)
            assert ex["auc_num2"] == brute and ex["correct"] == got["correct"] and ex["pos"] + ex["neg"] == n_eval
            nat = -sum(math.log(m[i]) if y[i] >= 0 else math.log(1.0 - m[i]) for i in range(n_eval)) / n_eval
            assert ex["logloss"] == pytest.approx(nat, rel=1e-13)


# ---- ref_cdf_gaussian: the device's sort keys are the bit patterns of sums of its values -----------------------------------------
def test_ref_cdf_gaussian_stays_in_the_unit_interval_and_is_monotone():
    """every fp32 whose low 8 mantissa bits are zero, both signs, in ascending order of magnitude"""
    last_pos, last_neg = None, None
    step = 1 << 20
    for lo in range(0, 0x7F800000 + 256, step * 256):
        bits = np.arange(lo, min(lo + step * 256, 0x7F800000 + 256), 256, dtype=np.uint32)
        for sign, last in ((0, last_pos), (0x80000000, last_neg)):
            x = (bits | np.uint32(sign)).view(np.float32)
            v = ref_cdf_gaussian(x)
            assert v.min() >= 0.0 and v.max() <= 1.0
            chain = v if last is None else np.concatenate([[last], v])
            d = np.diff(chain)
            assert np.all(d >= 0) if sign == 0 else np.all(d <= 0)
            if sign == 0:
                last_pos = v[-1]
            else:
                last_neg = v[-1]
    assert last_pos == 1.0 and last_neg == 0.0                        # +inf and -inf
    edge = np.array([0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF], dtype=np.uint32)     # the denormals' ends, the normals' ends
    for x in (edge.view(np.float32), (edge | np.uint32(0x80000000)).view(np.float32)):
        v = ref_cdf_gaussian(x)
        assert np.all((v >= 0.0) & (v <= 1.0)) and np.all(np.diff(v) * np.sign(x[0]) >= 0)
    z = ref_cdf_gaussian(np.array([0.0, -0.0], dtype=np.float32))
    assert z[0] == z[1] and 0.5 <= z[0] < 0.5 + 1e-8 and not np.signbit(z).any()
    assert math.isnan(float(ref_cdf_gaussian(np.float32(NAN))))


def test_the_learner_uses_the_same_function():
    from libfm_amd import learner
    assert learner.cdf_gaussian is ref_cdf_gaussian


# ---- edge cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", [REG, CLS])
def test_nan_propagates_and_is_counted(task):
    y = [1.0, -1.0, 1.0]
    pa = PosteriorAverage(task, -5.0, 5.0, burn_in=1)
    pa.accumulate([0.5, -0.5, 1.0])
    pa.accumulate([0.5, NAN, 1.0])                                     # draw 1: the first late draw
    pa.accumulate([0.5, -0.5, -0.5])
    assert math.isnan(pa.get(POST_ALL)[1]) and math.isnan(pa.get(POST_LATE)[1]) and not math.isnan(pa.get(POST_THIS)[1])
    for which, nan_rows in ((POST_THIS, 0), (POST_ALL, 1), (POST_LATE, 1)):
        m, ex = pa.metric(which, y), pa.evaluate_ex(which, y)
        assert m["rows"] == ex["rows"] == 3 and m["nan_rows"] == ex["nan_rows"] == nan_rows
        bad = [m["rmse"], m["mae"], ex["rmse"], ex["mae"]] if task == REG else [m["ll_ref"], ex["logloss"], ex["auc"]]
        assert all(math.isnan(v) == bool(nan_rows) for v in bad)
        if task == CLS:
            # the last draw: .69, .31, .31 -> rows 0 and 1; the means: row 1 is NaN and never correct, row 2 is .66 / .57
            assert (ex["pos"], ex["neg"]) == (2, 1) and m["correct"] == ex["correct"] == 2 and m["accuracy"] == 2 / 3
            assert ex["auc_num2"] == (0 if nan_rows else 3)           # positives .69 and .31 against the negative .31: 2 + 1


def test_one_class_only():
    for y in ([1.0] * 3, [-1.0] * 3):
        pa = PosteriorAverage(CLS, burn_in=0)
        pa.accumulate([0.5, -0.5, 2.0])
        ex = pa.evaluate_ex(POST_ALL, y)
        assert math.isnan(ex["auc"]) and ex["auc_num2"] == 0 and math.isfinite(ex["logloss"])
        assert ex["pos"] + ex["neg"] == 3 and ex["pos"] * ex["neg"] == 0


def test_all_means_equal_give_half():
    y = [1, -1, -1, 1, -1, -1, -1]
    pa = PosteriorAverage(CLS, burn_in=1)
    for p in (0.375, -1.0, 0.0):
        pa.accumulate([p] * 7)
    for which in (POST_THIS, POST_ALL, POST_LATE):
        ex = pa.evaluate_ex(which, y)
        assert ex["auc_num2"] == ex["pos"] * ex["neg"] == 10 and ex["auc"] == 0.5
    zero = PosteriorAverage(CLS)                                      # a zero model: every mean is cdf(0)
    zero.accumulate([0.0] * 7)
    assert np.all(zero.mean(POST_ALL) == ref_cdf_gaussian(0.0)) and abs(float(ref_cdf_gaussian(0.0)) - 0.5) < 1e-8


def test_saturation():
    pa = PosteriorAverage(CLS)
    pa.accumulate([40.0, 40.0])
    assert list(pa.get(POST_ALL)) == [1.0, 1.0]
    assert pa.evaluate_ex(POST_ALL, [1.0, -1.0])["logloss"] == INF    # the negative row: -ln(1 - 1)
    assert pa.evaluate_ex(POST_ALL, [1.0, 1.0])["logloss"] == 0.0
    m = pa.metric(POST_ALL, [1.0, -1.0])                              # the reference clamps to [.01, .99] and takes log10
    assert m["ll_ref"] == pytest.approx(-(math.log10(0.99) + math.log10(1 - 0.99)) / 2, rel=1e-15) and math.isfinite(m["ll_ref"])


# ---- the learner's default and the CLI's refusals (no device is touched) ---------------------------------------------------------
def test_default_keeps_refusing():
    from libfm_amd import learner as L
    for cls in (L.FMLearnALS, L.FMLearnMCMC):
        assert cls().device_average is False
    l = L.FMLearnMCMC()
    with pytest.raises(NotImplementedError):
        l.evaluate_ex(None)
    l.extra_metrics = ("auc",)
    with pytest.raises(NotImplementedError):
        l.learn(None, None)


def test_cli_refusals(capsys, tmp_path):
    from libfm_amd import cli
    missing = str(tmp_path / "no_such_file.libfm")
    argv = ["-task", "c", "-train", missing, "-test", missing, "-dim", "1,1,2", "-iter", "2", "-method", "mcmc", "-init_stdev", "0.1"]

    def err_of(extra):
        assert cli.main(argv + extra) == 0
        cap = capsys.readouterr()
        assert "ERROR:" in cap.err and "#Iter=" not in cap.out
        return cap.err

    assert "-metrics is not supported with -method mcmc" in err_of(["-metrics", "auc"])
    assert "-metrics is not supported with -method mcmc" in err_of(["-metrics", "auc", "-device_average", "0"])
    accepted = err_of(["-metrics", "auc,logloss", "-device_average", "1"])        # past the flags: it fails on the missing file
    assert "-metrics" not in accepted and "-device_average" not in accepted
    assert "-metrics needs -task c" in err_of(["-metrics", "auc", "-device_average", "1", "-task", "r"])
    assert "not 'f1'" in err_of(["-metrics", "f1", "-device_average", "1"])
    assert "-device_average takes 0 or 1" in err_of(["-device_average", "yes"])
    for method in ("sgd", "sgda"):
        assert "-device_average belongs to -method als and mcmc" in err_of(["-device_average", "1", "-method", method, "-learn_rate", "0.1"])
    assert "-device_average" not in err_of(["-device_average", "1", "-method", "als"])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from libfm_amd import build, capi
    build.build()
    return capi.load()


def test_the_library_exports_the_new_functions(lib):
    from libfm_amd import capi
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "libfm_amd", "libfmx.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    hdr = open(os.path.join(ROOT, "include", "fmx.h")).read().replace(" (", "(")
    bound = {n for n, _, _ in capi.SYMBOLS}
    for name in POST_FUNCTIONS + [n.replace("fmx_", "fmx_group_", 1) for n in POST_FUNCTIONS]:
        assert name in exported and name in bound and "int " + name + "(" in hdr and hasattr(lib, name), name
    assert (capi.POST_THIS, capi.POST_ALL, capi.POST_LATE) == (0, 1, 2) == (POST_THIS, POST_ALL, POST_LATE)
    assert C.sizeof(capi.PostOpts) == 16 and C.sizeof(capi.PostMetric) == 56 and C.sizeof(capi.PostStats) == 16 + 3 * 56 + 8


def test_null_handles_are_refused(lib):
    for prefix in ("fmx_post_", "fmx_group_post_"):
        assert getattr(lib, prefix + "begin")(None, 0, None) == -1                 # FMX_E_ARG
        assert getattr(lib, prefix + "accumulate")(None, 0, None) == -1
        assert getattr(lib, prefix + "evaluate_ex")(None, 0, 1, None) == -1
        assert getattr(lib, prefix + "get")(None, 0, 1, None, None) == -1
        assert getattr(lib, prefix + "end")(None, 0) == -1
