"""CPU: the field-weighted FM's float64 restatement (libfm_amd/fwfm.py) against a brute-force double loop and finite differences,
its reduction to the plain FM at r == 1, and the seven fmx_fwfm_* symbols in the header, the binding and the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fwfm_cases
from conftest import ROOT

SYMS = ["fmx_fwfm_begin", "fmx_fwfm_set_r", "fmx_fwfm_get_r", "fmx_fwfm_predict", "fmx_fwfm_evaluate", "fmx_fwfm_epoch", "fmx_fwfm_end"]


def brute(m, r, groups, d):
    out = np.zeros(d.n_rows)
    for e in range(d.n_rows):
        ent = d.entries[int(d.row_ptr[e]):int(d.row_ptr[e + 1])]
        y = m.w0 + sum(m.w[int(j)] * float(x) for j, x in ent)
        for a in range(len(ent)):
            for b in range(a + 1, len(ent)):
                i, j = int(ent[a]["id"]), int(ent[b]["id"])
                y += r[groups[i], groups[j]] * float(m.v[:, i] @ m.v[:, j]) * float(ent[a]["value"]) * float(ent[b]["value"])
        out[e] = y
    return out


@pytest.mark.parametrize("k, F", [(1, 1), (8, 5), (20, 17)])
def test_predict_against_the_double_loop(oracle, k, F):
    from libfm_amd import fwfm
    m, groups, r, d = fwfm_cases.make(oracle, k, F)
    np.testing.assert_allclose(fwfm.predict(m, r, groups, d), brute(m, r, groups, d), rtol=0, atol=1e-12)


def test_r_of_ones_is_the_plain_fm(oracle):
    from libfm_amd import fwfm
    m, groups, _, d = fwfm_cases.make(oracle, 8, 5)
    np.testing.assert_allclose(fwfm.predict(m, np.ones((5, 5)), groups, d), oracle.predict_raw(m, d), rtol=0, atol=1e-12)


def test_gradient_against_central_differences(oracle):
    """d sum_e y_e / d theta for v, w and r -- the diagonal r_gg and a repeated id (row 4 names feature 3 twice) included"""
    from libfm_amd import fwfm
    k, F = 4, 3
    m, groups, r, d = fwfm_cases.make(oracle, k, F)
    nb = d.n_rows
    ids, xs, ex, fld, S, D = fwfm.field_sums(m, groups, d, 0, nb, F)
    _, T = fwfm._rest(m, r, ids, xs, ex, S, D, nb, np.float64)
    feats, _, gw, gv, gr = fwfm.batch_gradients(m, r, groups, np.ones(nb), ids, xs, ex, fld, S, D, T)
    total = lambda: float(fwfm.predict(m, r, groups, d).sum())
    h = 1e-6

    def fd(arr, *idx):                                           # central difference in the entries idx of arr moved together
        old, res = arr[idx[0]], []
        for step in (h, -h):
            for i in idx:
                arr[i] = old + step
            res.append(total())
        for i in idx:
            arr[i] = old
        return (res[0] - res[1]) / (2 * h)
    at = {int(j): i for i, j in enumerate(feats)}
    for j in (3, 17, 40, int(feats[-1])):
        assert fd(m.w, j) == pytest.approx(gw[at[j]], rel=1e-6, abs=1e-7)
        for f in range(k):
            assert fd(m.v, (f, j)) == pytest.approx(gv[at[j], f], rel=1e-6, abs=1e-7)
    for g in range(F):
        for q in range(g, F):                                     # (r_gq and r_qg are one parameter)
            assert fd(r, (g, q), (q, g)) == pytest.approx(gr[g, q], rel=1e-6, abs=1e-7)


BASE = ["-train", "x", "-test", "y", "-task", "c", "-model", "fwfm"]


@pytest.mark.parametrize("argv, text", [
    (BASE + ["-method", "als", "-meta", "m"], "ERROR: -model fwfm belongs to -method sgd with -optimizer adagrad, not -method als"),
    (BASE + ["-method", "sgd", "-meta", "m"], "ERROR: -model fwfm belongs to -method sgd with -optimizer adagrad, not -method sgd -optimizer sgd"),
    (BASE + ["-method", "sgd", "-optimizer", "adagrad"], "ERROR: -model fwfm needs -meta"),
    (BASE + ["-method", "sgd", "-optimizer", "adagrad", "-meta", "m", "-devices", "0,0"], "ERROR: -devices is not supported with -model fwfm"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    assert cli.main(argv) == 0
    assert text in capsys.readouterr().err


def test_learner_refuses_before_any_device():
    from libfm_amd import learner as L
    l = L.FMLearnSGD()
    l.learn_rate, l.model = 0.1, "fwfm"
    for fields, exc, text in ((dict(), ValueError, "optimizer adagrad"), (dict(optimizer="adagrad"), ValueError, "needs groups"),
                              (dict(groups=np.zeros(4, dtype=np.uint32), devices=[0, 0]), NotImplementedError, "feature shards")):
        vars(l).update(fields)
        with pytest.raises(exc, match=text):
            l.init()


def test_symbols_and_abi():
    from libfm_amd import build, capi
    build.build()
    lib = capi.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    bound = {name for name, _, _ in capi.SYMBOLS}
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, hdr) and s in bound and hasattr(lib, s), s
    assert lib.fmx_abi_version() == 11
    opts = capi.FwfmOpts(0, 0, 0.0, 0.0, 0.0)
    out = np.zeros(4)
    assert lib.fmx_fwfm_begin(None, C.byref(opts)) == -1 and lib.fmx_fwfm_set_r(None, out.ctypes.data) == -1
    assert lib.fmx_fwfm_get_r(None, out.ctypes.data, None) == -1 and lib.fmx_fwfm_predict(None, 0, out.ctypes.data) == -1
    assert lib.fmx_fwfm_evaluate(None, 0, None) == -1 and lib.fmx_fwfm_epoch(None, 0, 0, 0, None) == -1 and lib.fmx_fwfm_end(None) == -1
