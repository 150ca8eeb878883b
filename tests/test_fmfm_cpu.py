"""CPU: the field-matrixed FM's float64 restatement (libfm_amd/fmfm.py) against a brute-force double loop, the plain FM at M == I, the
field-weighted FM at M_gh = r_gh I, and finite differences; the seven fmx_fmfm_* symbols in the header, the binding and the library;
the command line's and the learner's refusals before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fwfm_cases
from conftest import ROOT

SYMS = ["fmx_fmfm_begin", "fmx_fmfm_set_m", "fmx_fmfm_get_m", "fmx_fmfm_predict", "fmx_fmfm_evaluate", "fmx_fmfm_epoch", "fmx_fmfm_end"]


def brute(m, M, groups, d):
    out = np.zeros(d.n_rows)
    for e in range(d.n_rows):
        ent = d.entries[int(d.row_ptr[e]):int(d.row_ptr[e + 1])]
        y = m.w0 + sum(m.w[int(j)] * float(x) for j, x in ent)
        for a in range(len(ent)):
            for b in range(a + 1, len(ent)):
                i, j = int(ent[a]["id"]), int(ent[b]["id"])
                y += float(m.v[:, i] @ M[groups[i], groups[j]] @ m.v[:, j]) * float(ent[a]["value"]) * float(ent[b]["value"])
        out[e] = y
    return out


@pytest.mark.parametrize("k, F", [(1, 1), (4, 3), (5, 17)])
def test_predict_against_the_double_loop(oracle, k, F):
    """fwfm_cases' rows: an empty row, a row with all entries in one field, a repeated id"""
    from libfm_amd import fmfm
    m, groups, _, d = fwfm_cases.make(oracle, k, F)
    M = fmfm.random_m(F, k, np.random.default_rng(3 + 7 * F + k))
    np.testing.assert_allclose(fmfm.predict(m, M, groups, d), brute(m, M, groups, d), rtol=0, atol=1e-12)


def test_identity_is_the_plain_fm_and_scaled_identities_the_fwfm(oracle):
    from libfm_amd import fmfm, fwfm
    k, F = 4, 5
    m, groups, r, d = fwfm_cases.make(oracle, k, F)
    np.testing.assert_allclose(fmfm.predict(m, fmfm.identity(F, k), groups, d), oracle.predict_raw(m, d), rtol=0, atol=1e-12)
    r[np.diag_indices(F)] = 1.0
    M = r[:, :, None, None] * np.eye(k)
    np.testing.assert_allclose(fmfm.predict(m, M, groups, d), fwfm.predict(m, r, groups, d), rtol=0, atol=1e-12)


def test_gradient_against_central_differences(oracle):
    """d sum_e y_e / d theta for w, v and elements of the upper blocks of M -- a repeated id (row 4 names feature 3 twice) included"""
    from libfm_amd import fmfm, fwfm
    k, F = 4, 3
    m, groups, _, d = fwfm_cases.make(oracle, k, F)
    M = fmfm.random_m(F, k, np.random.default_rng(3 + 7 * F + k))
    ids, xs, ex, fld, S, D = fwfm.field_sums(m, groups, d, 0, d.n_rows, F)
    _, T = fmfm._rest(m, M, ids, xs, ex, S, D, np.float64)
    feats, _, gw, gv, gm = fmfm.batch_gradients(m, groups, np.ones(d.n_rows), ids, xs, ex, fld, S, T)
    total = lambda: float(fmfm.predict(m, M, groups, d).sum())
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
    for g, q in ((0, 1), (0, 2), (1, 2)):
        for a, b in ((0, 0), (1, 3), (3, 2)):                     # (M[g][q][a][b] and M[q][g][b][a] are one parameter)
            assert fd(M, (g, q, a, b), (q, g, b, a)) == pytest.approx(gm[g, q, a, b], rel=1e-6, abs=1e-7)


BASE = ["-train", "x", "-test", "y", "-task", "c", "-model", "fmfm"]
ADA = ["-method", "sgd", "-optimizer", "adagrad"]


@pytest.mark.parametrize("argv, text", [
    (BASE + ["-method", "als", "-meta", "m"], "ERROR: -model fmfm belongs to -method sgd with -optimizer adagrad, not -method als"),
    (BASE + ["-method", "sgd", "-meta", "m"], "ERROR: -model fmfm belongs to -method sgd with -optimizer adagrad, not -method sgd -optimizer sgd"),
    (BASE + ADA, "ERROR: -model fmfm needs -meta"),
    (BASE + ADA + ["-meta", "m", "-devices", "0,0"], "ERROR: -devices is not supported with -model fmfm"),
    (BASE + ADA + ["-meta", "m", "-r_out", "f"], "ERROR: -r_out belongs to -model fwfm"),
    (BASE[:-1] + ["fwfm"] + ADA + ["-meta", "m", "-m_out", "f"], "ERROR: -m_out belongs to -model fmfm"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    assert cli.main(argv) == 0
    assert text in capsys.readouterr().err


def test_learner_refuses_before_any_device():
    from libfm_amd import learner as L
    l = L.FMLearnSGD()
    l.learn_rate, l.model = 0.1, "fmfm"
    for fields, exc, text in ((dict(), ValueError, "optimizer adagrad"), (dict(optimizer="adagrad"), ValueError, "needs groups"),
                              (dict(groups=np.zeros(4, dtype=np.uint32), devices=[0, 0]), NotImplementedError, "feature shards")):
        vars(l).update(fields)
        with pytest.raises(exc, match=text):
            l.init()
    l.devices = None
    with pytest.raises(NotImplementedError, match="not supported with model fmfm"):
        l.evaluate_ex(None)


def test_symbols_and_abi():
    from libfm_amd import build, capi
    build.build()
    lib = capi.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    bound = {name for name, _, _ in capi.SYMBOLS}
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, hdr) and s in bound and hasattr(lib, s), s
    assert lib.fmx_abi_version() == 11
    out = np.zeros(4)
    assert lib.fmx_fmfm_begin(None, C.byref(capi.FmfmOpts(0.0, 0.0, 0.0, 0))) == -1 and lib.fmx_fmfm_set_m(None, out.ctypes.data) == -1
    assert lib.fmx_fmfm_get_m(None, out.ctypes.data, None) == -1 and lib.fmx_fmfm_predict(None, 0, out.ctypes.data) == -1
    assert lib.fmx_fmfm_evaluate(None, 0, None) == -1 and lib.fmx_fmfm_epoch(None, 0, 0, 0, None) == -1 and lib.fmx_fmfm_end(None) == -1
