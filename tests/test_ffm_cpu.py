"""CPU: the field-aware FM's float64 restatement (libfm_amd/ffm.py) against a brute-force double loop and finite differences, its
reduction to the plain FM at one field, and the five fmx_ffm_* symbols in the header, the binding and the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fwfm_cases
from conftest import ROOT

SYMS = ["fmx_ffm_begin", "fmx_ffm_predict", "fmx_ffm_evaluate", "fmx_ffm_epoch", "fmx_ffm_end"]


def brute(m, groups, kf, d):
    blk = lambda j, h: m.v[h * kf:(h + 1) * kf, j]
    out = np.zeros(d.n_rows)
    for e in range(d.n_rows):
        ent = d.entries[int(d.row_ptr[e]):int(d.row_ptr[e + 1])]
        y = m.w0 + sum(m.w[int(j)] * float(x) for j, x in ent)
        for a in range(len(ent)):
            for b in range(a + 1, len(ent)):
                i, j = int(ent[a]["id"]), int(ent[b]["id"])
                y += float(blk(i, groups[j]) @ blk(j, groups[i])) * float(ent[a]["value"]) * float(ent[b]["value"])
        out[e] = y
    return out


@pytest.mark.parametrize("kf, F", [(1, 1), (8, 1), (4, 3), (5, 17)])
def test_predict_against_the_double_loop(oracle, kf, F):
    from libfm_amd import ffm
    m, groups, _, d = fwfm_cases.make(oracle, F * kf, F)
    np.testing.assert_allclose(ffm.predict(m, groups, kf, d), brute(m, groups, kf, d), rtol=0, atol=1e-12)
    if F == 1:                                                   # one field is the plain FM
        np.testing.assert_allclose(ffm.predict(m, groups, kf, d), oracle.predict_raw(m, d), rtol=0, atol=1e-12)


def test_gradient_against_central_differences(oracle):
    """w and every column of v, inside and outside the own block, the repeated id included (row 4 names feature 3 twice)"""
    from libfm_amd import ffm
    kf, F = 4, 3
    m, groups, _, d = fwfm_cases.make(oracle, F * kf, F)
    ids, xs, ex, fld, Q, _ = ffm.field_tiles(m, groups, kf, d, 0, d.n_rows, F)
    feats, _, gw, gv = ffm.batch_gradients(m, groups, kf, np.ones(d.n_rows), ids, xs, ex, fld, Q)
    total = lambda: float(ffm.predict(m, groups, kf, d).sum())
    h = 1e-6

    def fd(arr, idx):
        old, res = arr[idx], []
        for step in (h, -h):
            arr[idx] = old + step
            res.append(total())
        arr[idx] = old
        return (res[0] - res[1]) / (2 * h)
    at = {int(j): i for i, j in enumerate(feats)}
    for j in (3, 17, 40, int(feats[-1])):
        assert fd(m.w, j) == pytest.approx(gw[at[j]], rel=1e-6, abs=1e-7)
        for c in range(F * kf):                                  # (columns [g(j) kf, (g(j) + 1) kf) are the own block)
            assert fd(m.v, (c, j)) == pytest.approx(gv[at[j], c], rel=1e-6, abs=1e-7)


BASE = ["-train", "x", "-test", "y", "-task", "c", "-model", "ffm"]


@pytest.mark.parametrize("argv, text", [
    (BASE + ["-method", "als", "-meta", "m"], "ERROR: -model ffm belongs to -method sgd with -optimizer adagrad, not -method als"),
    (BASE + ["-method", "sgd", "-meta", "m"], "ERROR: -model ffm belongs to -method sgd with -optimizer adagrad, not -method sgd -optimizer sgd"),
    (BASE + ["-method", "sgd", "-optimizer", "adagrad"], "ERROR: -model ffm needs -meta"),
    (BASE + ["-method", "sgd", "-optimizer", "adagrad", "-meta", "m", "-devices", "0,0"], "ERROR: -devices is not supported with -model ffm"),
    (BASE + ["-method", "sgd", "-optimizer", "adagrad", "-meta", "m", "-r_out", "r"], "ERROR: -r_out belongs to -model fwfm"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    assert cli.main(argv) == 0
    assert text in capsys.readouterr().err


def test_learner_refuses_before_any_device():
    from libfm_amd import learner as L
    l = L.FMLearnSGD()
    l.learn_rate, l.model = 0.1, "ffm"
    for fields, exc, text in ((dict(), ValueError, "model ffm trains with optimizer adagrad"), (dict(optimizer="adagrad"), ValueError, "model ffm needs groups"),
                              (dict(groups=np.zeros(4, dtype=np.uint32), devices=[0, 0]), NotImplementedError, "feature shards")):
        vars(l).update(fields)
        with pytest.raises(exc, match=text):
            l.init()
    l.devices = None
    for call in (lambda: l.save_checkpoint("x"), lambda: l.evaluate_ex(None), lambda: l.compact()):
        with pytest.raises(NotImplementedError, match="is not supported with model ffm: it scores the plain FM"):
            call()


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
    assert lib.fmx_ffm_begin(None, C.byref(capi.FfmOpts(4, 0))) == -1 and lib.fmx_ffm_predict(None, 0, out.ctypes.data) == -1
    assert lib.fmx_ffm_evaluate(None, 0, None) == -1 and lib.fmx_ffm_epoch(None, 0, 0, 0, None) == -1 and lib.fmx_ffm_end(None) == -1
