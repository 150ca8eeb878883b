"""CPU: the top-K retrieval surface (fmx_topk) and its fp64 oracle (tests/topk_oracle.py): the C-ABI declaration, binding and
export (without an ABI version change), the decomposed score against the explicit join through oracle.predict_raw, the list
rules on hand-built cases, and libfm_amd.ranking.metrics on hand-computed values."""
import os
import re
import subprocess

import numpy as np
import pytest

import datagen
import topk_oracle as T
from conftest import ROOT


def test_symbol_declared_bound_exported_abi_unchanged():
    from libfm_amd import build, capi
    build.build()
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "fmx.h")).read()
    assert int(re.search(r"#define\s+FMX_ABI_VERSION\s+(\d+)", hdr).group(1)) == 11 == lib.fmx_abi_version()
    assert "int fmx_topk(" in hdr
    assert int(re.search(r"#define\s+FMX_TOPK_MAX\s+(\d+)u", hdr).group(1)) == capi.TOPK_MAX == 1024
    assert "fmx_topk" in {n for n, _, _ in capi.SYMBOLS} and hasattr(lib, "fmx_topk")
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "libfm_amd", "libfmx.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "fmx_topk" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    # the structures as the header lays them out
    import ctypes as C
    assert C.sizeof(capi.TopkOpts) == 40 and capi.TopkOpts.exclude_ptr.offset == 24
    assert C.sizeof(capi.TopkStats) == 32


def _model(O, n, k, seed, k0=True, k1=True, w0=0.3):
    rng = np.random.default_rng(seed)
    m = O.Model(n, k, k0, k1)
    m.w0 = w0
    m.w[:] = rng.normal(0, 0.5, n)
    m.v[:] = rng.normal(0, 0.3, (k, n))
    return m


CASES = [  # (name, k, k0, k1, same_slot)
    ("ml_k8", 8, True, True, False),
    ("ragged_dup_k5", 5, True, True, False),
    ("nolin_k4", 4, False, False, False),
    ("k0", 0, True, True, False),
    ("k1", 1, True, False, False),
    ("same_slot_k3", 3, True, True, True),
]


@pytest.mark.parametrize("name,k,k0,k1,same", CASES)
def test_decomposed_equals_explicit(oracle, name, k, k0, k1, same):
    if name.startswith("ml"):
        ent, rp, _ = datagen.movielens_shaped(20, 30, 24, seed=3)
        n = 50
    else:
        ent, rp, _ = datagen.ragged_real(40, 18, 6, seed=len(name), empty_every=5, duplicates=True)
        n = 40
    m = _model(oracle, n, k, seed=k + 11, k0=k0, k1=k1)
    if same:
        cent, crp = ent, rp
        qent, qrp = ent, rp
    else:
        cent, crp, _ = datagen.ragged_real(n, 13, 5, seed=99, empty_every=4, duplicates=True)
        qent, qrp = ent, rp
    e = T.scores_explicit(oracle, m, qent, qrp, cent, crp)
    d = T.scores_decomposed(m, qent, qrp, cent, crp)
    assert e.shape == d.shape == (len(qrp) - 1, len(crp) - 1)
    np.testing.assert_allclose(d, e, rtol=1e-12, atol=1e-12)
    # a query row's ids also occur in the candidate rows (ids across the two rows), and some rows repeat an id
    assert np.isin(qent["id"], cent["id"]).any()
    # a subset of the queries gives the same rows
    sub = [2, 0, 5]
    np.testing.assert_allclose(T.scores_decomposed(m, qent, qrp, cent, crp, sub), e[sub], rtol=1e-12, atol=1e-12)


def test_select_ties_padding_nan_exclusion():
    s = np.array([[1.0, 3.0, 3.0, np.nan, 2.0, 3.0],
                  [np.nan, np.nan, 0.5, np.nan, np.nan, np.nan],
                  [-np.inf, 1.0, -np.inf, 0.0, 0.0, 1.0]])
    idx, sc = T.select(s, 4)
    assert idx[0].tolist() == [1, 2, 5, 4] and sc[0].tolist() == [3.0, 3.0, 3.0, 2.0]
    assert idx[1].tolist() == [2, T.NONE, T.NONE, T.NONE] and sc[1, 0] == 0.5 and np.all(np.isneginf(sc[1, 1:]))
    assert idx[2].tolist() == [1, 5, 3, 4]
    idx, sc = T.select(s, 6)
    assert idx[2].tolist() == [1, 5, 3, 4, 0, 2] and np.all(np.isneginf(sc[2, 4:]))   # -inf scores are eligible, before padding
    ex = [[2, 2, 1], [], [5, 1, 0, 2, 3, 4]]
    idx, sc = T.select(s, 3, ex)
    assert idx[0].tolist() == [5, 4, 0]
    assert idx[1].tolist() == [2, T.NONE, T.NONE]
    assert idx[2].tolist() == [T.NONE] * 3 and np.all(np.isneginf(sc[2]))


def test_ranking_metrics_hand_computed():
    from libfm_amd import ranking
    none = 0xFFFFFFFF
    idx = np.array([[3, 1, 7], [2, 5, none], [9, 8, 4], [0, 1, 2]], dtype=np.uint32)
    ptr = [0, 2, 4, 5, 5]              # query 3 has no relevant candidates: left out
    rel = [1, 7, 5, 6, 4]
    m = ranking.metrics(idx, ptr, rel)
    d = [1.0, 1 / np.log2(3), 0.5]     # discounts of positions 0, 1, 2
    recall = (2 / 2 + 1 / 2 + 1 / 1) / 3
    precision = (2 / 3 + 1 / 3 + 1 / 3) / 3
    ndcg = ((d[1] + d[2]) / (d[0] + d[1]) + d[1] / (d[0] + d[1]) + d[2] / d[0]) / 3
    assert m["queries"] == 3
    assert m["recall"] == pytest.approx(recall, abs=1e-15)
    assert m["precision"] == pytest.approx(precision, abs=1e-15)
    assert m["ndcg"] == pytest.approx(ndcg, abs=1e-15)
    assert m["hit_rate"] == 1.0
    m = ranking.metrics(np.full((1, 2), none, dtype=np.uint32), [0, 3], [0, 0, 1])   # padding only: misses; repeats count once
    assert m["recall"] == 0.0 and m["ndcg"] == 0.0 and m["hit_rate"] == 0.0 and m["queries"] == 1


def test_cli_exclude_file_and_topk_out(tmp_path):
    from libfm_amd import cli
    p = tmp_path / "ex.txt"
    p.write_text("1 4\n# comment\n0 2\n1 0\n\n1 4\n")
    ptr, idx = cli.read_exclude(str(p), 3, 5)
    assert ptr.tolist() == [0, 1, 4, 4] and idx.tolist() == [2, 4, 0, 4]
    with pytest.raises(ValueError):
        cli.read_exclude(str(p), 3, 4)
    out = tmp_path / "top.txt"
    cli.write_topk(str(out), np.array([[3, 0xFFFFFFFF], [1, 2]], dtype=np.uint32), np.array([[1.5, -np.inf], [0.25, -3e-7]]))
    assert out.read_text() == "3:1.5\n1:0.25 2:-3e-07\n"


def test_cli_refuses_topk_with_mcmc(capsys):
    from libfm_amd import cli
    assert cli.main(["-task", "r", "-train", "a", "-test", "b", "-method", "mcmc", "-topk", "5", "-candidates", "c"]) == 0
    assert "ERROR: -topk is not supported with -method mcmc" in capsys.readouterr().err
