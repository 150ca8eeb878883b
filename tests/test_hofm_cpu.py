"""CPU: the third-order FM's float64 restatement (libfm_amd/hofm.py) against a brute-force loop over entry triples and pairs, finite
differences and the plain FM at k3 = 0; the five fmx_hofm_* symbols; the learner's and the command line's refusals before any device."""
import os
import re
from itertools import combinations

import numpy as np
import pytest

import hofm_cases
from conftest import ROOT


def brute(m, k2, d):
    out = np.zeros(d.n_rows)
    for e in range(d.n_rows):
        ent = d.entries[int(d.row_ptr[e]):int(d.row_ptr[e + 1])]
        z = np.array([m.v[:, int(j)] * float(x) for j, x in ent]).reshape(len(ent), m.k)
        out[e] = (m.w0 + sum(m.w[int(j)] * float(x) for j, x in ent) + sum(float(z[a, :k2] @ z[b, :k2]) for a, b in combinations(range(len(ent)), 2))
                  + sum(float((z[a, k2:] * z[b, k2:] * z[c, k2:]).sum()) for a, b, c in combinations(range(len(ent)), 3)))
    return out


@pytest.mark.parametrize("k2, k3", [(0, 1), (4, 0), (3, 5)])
def test_predict_against_the_triple_loop(oracle, k2, k3):
    from libfm_amd import hofm
    m, d = hofm_cases.make(oracle, k2, k3, rows=40)
    assert {0, 1, 2, 3} <= set(np.diff(d.row_ptr.astype(int)))   # empty rows, rows of 1, 2 and 3 entries; every row of >= 2 repeats an id
    np.testing.assert_allclose(hofm.predict(m, k3, d), brute(m, k2, d), rtol=0, atol=1e-12)
    if k3 == 0:                                                  # no third-order factors: the plain FM
        np.testing.assert_allclose(hofm.predict(m, 0, d), oracle.predict_raw(m, d), rtol=0, atol=1e-12)


def test_gradient_against_central_differences(oracle):
    """w, one pair column and one third-order column of v; `dup` is a feature named twice in one row"""
    from libfm_amd import hofm
    k2, k3, h = 3, 5, 1e-6
    m, d = hofm_cases.make(oracle, k2, k3, rows=40)
    rp = d.row_ptr.astype(int)
    dup = int(d.entries["id"][rp[np.flatnonzero(np.diff(rp) >= 3)[0]]])
    ids, xs, ex, p1, p2, p3 = hofm.power_sums(m, d, 0, d.n_rows)
    e2 = hofm._rest(m, k2, ids, xs, ex, p1, p2, p3, np.float64)[1]
    feats, _, gw, gv = hofm.batch_gradients(m, k3, np.ones(d.n_rows), ids, xs, ex, p1, e2)

    def fd(arr, idx):
        old, res = arr[idx], []
        for step in (h, -h):
            arr[idx] = old + step
            res.append(float(hofm.predict(m, k3, d).sum()))
        arr[idx] = old
        return (res[0] - res[1]) / (2 * h)
    at = {int(j): i for i, j in enumerate(feats)}
    for j in (dup, int(feats[0]), int(feats[-1])):
        assert fd(m.w, j) == pytest.approx(gw[at[j]], rel=1e-6, abs=1e-7)
        for c in (1, k2 + 2):
            assert fd(m.v, (c, j)) == pytest.approx(gv[at[j], c], rel=1e-6, abs=1e-7)


BASE = ["-train", "x", "-test", "y", "-task", "c", "-dim", "1,1,4,2", "-method"]


@pytest.mark.parametrize("argv, text", [
    (BASE + ["sgd", "-optimizer", "adagrad"], "ERROR: -dim needs k0,k1,k2"),
    (BASE + ["sgd", "-optimizer", "adagrad", "-model", "fwfm", "-meta", "m"], "ERROR: -dim needs k0,k1,k2"),
    (BASE + ["als", "-model", "hofm"], "ERROR: -model hofm belongs to -method sgd with -optimizer adagrad, not -method als"),
    (BASE + ["sgd", "-model", "hofm"], "ERROR: -model hofm belongs to -method sgd with -optimizer adagrad, not -method sgd -optimizer sgd"),
    (BASE + ["sgd", "-optimizer", "adagrad", "-model", "hofm", "-devices", "0,0"], "ERROR: -devices is not supported with -model hofm"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    assert cli.main(argv) == 0
    assert text in capsys.readouterr().err


def test_learner_refuses_before_any_device():
    from libfm_amd import learner as L
    l = L.FMLearnSGD()
    l.learn_rate, l.model, l.num_factor3 = 0.1, "hofm", 2
    for fields, exc, text in ((dict(), ValueError, "model hofm trains with optimizer adagrad"),
                              (dict(optimizer="adagrad", devices=[0, 0]), NotImplementedError, "feature shards"),
                              (dict(devices=None, extra_metrics=("auc",)), NotImplementedError, "extra_metrics is not supported with model hofm")):
        vars(l).update(fields)
        with pytest.raises(exc, match=text):
            l.init()
    for call in (lambda: l.save_checkpoint("x"), lambda: l.evaluate_ex(None), lambda: l.compact()):
        with pytest.raises(NotImplementedError, match="is not supported with model hofm: it scores the plain FM"):
            call()


def test_symbols_and_abi():
    from libfm_amd import build, capi
    build.build()
    lib = capi.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    bound = {name for name, _, _ in capi.SYMBOLS}
    for s in ("fmx_hofm_begin", "fmx_hofm_predict", "fmx_hofm_evaluate", "fmx_hofm_epoch", "fmx_hofm_end"):
        assert re.search(r"\b%s\s*\(" % s, hdr) and s in bound and hasattr(lib, s), s
    assert lib.fmx_abi_version() == 11
    assert lib.fmx_hofm_begin(None, None) == -1 and lib.fmx_hofm_epoch(None, 0, 0, 0, None) == -1 and lib.fmx_hofm_end(None) == -1
