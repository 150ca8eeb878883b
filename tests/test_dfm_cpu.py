"""CPU: DeepFM's float64 restatement (libfm_amd/dfm.py) against a brute-force loop, the plain FM at a zero net and finite differences;
the kink condition of every training case of tests/test_gpu_dfm.py; the seven fmx_dfm_* symbols in the header, the binding and the
library; the command line's and the learner's refusals before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dfm_cases
from conftest import ROOT

SYMS = ["fmx_dfm_begin", "fmx_dfm_set_net", "fmx_dfm_get_net", "fmx_dfm_predict", "fmx_dfm_evaluate", "fmx_dfm_epoch", "fmx_dfm_end"]


def brute(m, net, groups, d):
    """pairs of entries, and the MLP unit by unit"""
    W1, b1, w2 = net
    k, F = m.v.shape[0], W1.shape[0] // m.v.shape[0]
    out = np.zeros(d.n_rows)
    for e in range(d.n_rows):
        ent = d.entries[int(d.row_ptr[e]):int(d.row_ptr[e + 1])]
        y = m.w0 + sum(m.w[int(j)] * float(x) for j, x in ent)
        s = np.zeros(F * k)
        for a, (i, xa) in enumerate(ent):
            s[groups[i] * k:groups[i] * k + k] += m.v[:, int(i)] * float(xa)
            for j, xb in ent[a + 1:]:
                y += float(m.v[:, int(i)] @ m.v[:, int(j)]) * float(xa) * float(xb)
        for u in range(len(b1)):
            y += w2[u] * max(float(s @ W1[:, u]) + b1[u], 0.0)
        out[e] = y
    return out


@pytest.mark.parametrize("k, F, H", [(1, 1, 1), (4, 3, 8), (5, 17, 24)])
def test_predict_against_the_brute_force_loop_and_the_plain_fm(oracle, k, F, H):
    from libfm_amd import dfm
    m, groups, net, d = dfm_cases.make(oracle, k, F, H)
    assert (np.diff(d.row_ptr) == 0).any()
    np.testing.assert_allclose(dfm.predict(m, net, groups, d), brute(m, net, groups, d), rtol=0, atol=1e-12)
    np.testing.assert_allclose(dfm.predict(m, dfm.zero_net(F, k, H), groups, d), oracle.predict_raw(m, d), rtol=0, atol=1e-12)


def test_gradient_against_central_differences(oracle):
    """d sum_e mult_e y_e / d theta for w, v, W1, b1 and w2 -- rows with a repeated id included"""
    from libfm_amd import dfm, fwfm
    k, F, H = 4, 3, 8
    m, groups, net, d = dfm_cases.make(oracle, k, F, H)
    mult = np.random.default_rng(1).normal(size=d.n_rows)
    ids, xs, ex, fld, S, D = fwfm.field_sums(m, groups, d, 0, d.n_rows, F)
    _, pre, a, Stot = dfm.forward(m, net, ids, xs, ex, S, D, np.float64)
    assert np.abs(pre).min() > 1e-4                               # (no unit within the step of a difference of its kink)
    feats, _, gw, gv, gW1, gb1, gw2 = dfm.batch_gradients(m, net, mult, ids, xs, ex, fld, S, pre, a, Stot)
    total = lambda: float(mult @ dfm.predict(m, net, groups, d))
    h = 1e-6

    def fd(arr, idx):
        old, res = arr[idx], []
        for step in (h, -h):
            arr[idx] = old + step
            res.append(total())
        arr[idx] = old
        return (res[0] - res[1]) / (2 * h)
    at = {int(j): i for i, j in enumerate(feats)}
    for j in [int(feats[0]), int(feats[7]), int(d.entries["id"][0]), int(feats[-1])]:
        assert fd(m.w, j) == pytest.approx(gw[at[j]], rel=1e-6, abs=1e-7)
        for f in range(k):
            assert fd(m.v, (f, j)) == pytest.approx(gv[at[j], f], rel=1e-6, abs=1e-7)
    for u in (0, 3, 7):
        assert fd(net[1], u) == pytest.approx(gb1[u], rel=1e-6, abs=1e-7) and fd(net[2], u) == pytest.approx(gw2[u], rel=1e-6, abs=1e-7)
        for r in (0, 5, F * k - 1):
            assert fd(net[0], (r, u)) == pytest.approx(gW1[r, u], rel=1e-6, abs=1e-7)


@pytest.mark.parametrize("case", dfm_cases.TRAIN)
def test_no_training_case_meets_the_kink(oracle, case):
    """a condition on the inputs: a unit within 1e-4 of its kink may flip between fp32 and fp64, and AdaGrad turns a flip into a full step"""
    assert dfm_cases.train_reference(oracle, case)[-1] >= 1e-4


BASE = ["-train", "x", "-test", "y", "-task", "c", "-model", "dfm"]
ADA = ["-method", "sgd", "-optimizer", "adagrad"]


@pytest.mark.parametrize("argv, text", [
    (BASE + ["-method", "als", "-meta", "m"], "ERROR: -model dfm belongs to -method sgd with -optimizer adagrad, not -method als"),
    (BASE + ["-method", "sgd", "-meta", "m"], "ERROR: -model dfm belongs to -method sgd with -optimizer adagrad, not -method sgd -optimizer sgd"),
    (BASE + ADA, "ERROR: -model dfm needs -meta"),
    (BASE + ADA + ["-meta", "m", "-devices", "0,0"], "ERROR: -devices is not supported with -model dfm"),
    (BASE + ADA + ["-meta", "m", "-r_out", "f", "-m_out", "f"], "ERROR: -r_out belongs to -model fwfm"),
    (BASE + ADA + ["-meta", "m", "-m_out", "f"], "ERROR: -m_out belongs to -model fmfm"),
    (BASE + ADA + ["-meta", "m", "-hidden", "0"], "ERROR: -hidden needs H >= 1"),
    (BASE[:-1] + ["fmfm"] + ADA + ["-meta", "m", "-hidden", "8"], "ERROR: -hidden belongs to -model dfm"),
    (BASE[:-2] + ADA + ["-net_out", "f"], "ERROR: -net_out belongs to -model dfm"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    assert cli.main(argv) == 0
    assert text in capsys.readouterr().err


def test_learner_refuses_before_any_device():
    from libfm_amd import learner as L
    l = L.FMLearnSGD()
    l.learn_rate, l.model = 0.1, "dfm"
    for fields, exc, text in ((dict(), ValueError, "optimizer adagrad"), (dict(optimizer="adagrad", num_hidden=0), ValueError, "num_hidden"),
                              (dict(num_hidden=8), ValueError, "needs groups"),
                              (dict(groups=np.zeros(4, dtype=np.uint32), devices=[0, 0]), NotImplementedError, "feature shards")):
        vars(l).update(fields)
        with pytest.raises(exc, match=text):
            l.init()
    l.devices = None
    with pytest.raises(NotImplementedError, match="not supported with model dfm"):
        l.evaluate_ex(None)


def test_symbols_and_null_handles():
    from libfm_amd import build, capi
    build.build()
    lib = capi.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    bound = {name for name, _, _ in capi.SYMBOLS}
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, hdr) and s in bound and hasattr(lib, s), s
    assert lib.fmx_abi_version() == 11
    p = np.zeros(4).ctypes.data
    assert lib.fmx_dfm_begin(None, C.byref(capi.DfmOpts(8, 0.0, 0.0, 0.0, 0))) == -1 and lib.fmx_dfm_set_net(None, p, p, p) == -1
    assert lib.fmx_dfm_get_net(None, p, None, None, None, None, None) == -1 and lib.fmx_dfm_predict(None, 0, p) == -1
    assert lib.fmx_dfm_evaluate(None, 0, None) == -1 and lib.fmx_dfm_epoch(None, 0, 0, 0, None) == -1 and lib.fmx_dfm_end(None) == -1
