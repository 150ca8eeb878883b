"""CPU: libfm_amd.evalmetrics.rank_metrics, the restatement the device's fmx_evaluate_rank is held to, checked
by itself -- against brute force over every order inside the tie runs, a hand-computed case and libfm_amd.ranking.metrics on
tie-free scores -- and fmx_rank_discounts, which is host arithmetic inside libfmx.so and needs no device.  Then the checks of the
command line's -rank_at that need no device."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from libfm_amd.evalmetrics import rank_discounts, rank_metrics

U = 2.0 ** -52


def test_hand_sized_case():
    """one query, scores 3 | 2 2 2 | 1 with labels + | + - + | -: the runs occupy the ranks [0, 1), [1, 4), [4, 5) with 1, 2 and 0
    relevant rows.  At K = 2 the mixed run straddles the cutoff: one of its three rows is above it, so it adds 2 * 1 / 3 hits and
    2 * (D[2] - D[1]) / 3 = 2 / (3 log2 3) to the DCG.  The second query has no relevant row and takes no part."""
    scores = [2.0, 3.0, 2.0, 1.0, 2.0, 9.0, 9.0]
    target = [1, 1, -1, -1, 1, -1, -1]
    qid = [0, 0, 0, 0, 0, 1, 1]
    m = rank_metrics(scores, target, qid, 3, (1, 2, 4, 8))
    assert m["relevant_queries"] == 1 and m["n_cutoffs"] == 4 and [a["k"] for a in m["at"]] == [1, 2, 4, 8]
    assert m["by_query"]["queries"] == 3 and m["by_query"]["empty_queries"] == 1 and m["by_query"]["one_class_queries"] == 1
    assert m["hits_q"][0] == [1.0, 1.6666666666666665, 3.0, 3.0]
    d2 = 1.0 + 2.0 * (1.0 / math.log2(3.0)) / 3.0
    d4 = 1.0 + 2.0 * (1.0 / math.log2(3.0) + 0.5 + 1.0 / math.log2(5.0)) / 3.0
    assert m["dcg_q"][0][0] == 1.0
    assert abs(m["dcg_q"][0][1] - d2) <= 4 * U and abs(m["dcg_q"][0][1] - 1.420619835714305) < 1e-15    # 1 + 2 * 0.63092975357145743 / 3
    assert abs(m["dcg_q"][0][2] - d4) <= 8 * U and m["dcg_q"][0][3] == m["dcg_q"][0][2]
    assert m["hits_q"][1] == [0.0] * 4 and m["dcg_q"][1] == [0.0] * 4 and m["hits_q"][2] == [0.0] * 4
    assert [a["tied_queries"] for a in m["at"]] == [0, 1, 1, 1]           # at K = 1 only the run [0, 1) begins above the cutoff
    assert [a["hits"] for a in m["at"]] == [1.0, 1.6666666666666665, 3.0, 3.0]
    D = rank_discounts(8)
    assert m["at"][1]["ndcg"] == m["dcg_q"][0][1] / D[2] and m["at"][3]["ndcg"] == m["dcg_q"][0][3] / D[3]
    assert m["at"][1]["recall"] == 1.6666666666666665 / 3.0 and m["at"][1]["precision"] == 1.6666666666666665 / 2.0
    assert m["at"][3]["recall"] == 1.0 and m["at"][3]["precision"] == 3.0 / 8.0          # / K although the query has 5 rows


def _brute(scores, positive, K):
    """(mean hits, mean DCG) at K over every order of the rows that is sorted by descending score"""
    runs = {}
    for i, s in enumerate(scores):
        runs.setdefault(s, []).append(i)
    blocks = [list(itertools.permutations(runs[s])) for s in sorted(runs, reverse=True)]
    hits, dcgs = [], []
    for choice in itertools.product(*blocks):
        order = [i for block in choice for i in block][:K]
        hits.append(float(sum(1 for i in order if positive[i])))
        dcgs.append(math.fsum(1.0 / math.log2(r + 2.0) for r, i in enumerate(order) if positive[i]))
    return math.fsum(hits) / len(hits), math.fsum(dcgs) / len(dcgs)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_against_every_order_inside_the_tie_runs(seed):
    rng = np.random.default_rng(seed)
    cutoffs = (1, 2, 3, 5)
    for ks in (cutoffs, (8,)):                                           # K in {1, 2, 3, 5, 8}: at most four cutoffs a call
        nq = 100
        sizes = rng.integers(1, 7, nq)
        qid = np.repeat(np.arange(nq), sizes)
        scores = rng.integers(0, 3, len(qid)).astype(np.float32)
        target = np.where(rng.random(len(qid)) < 0.5, 1.0, -1.0)
        perm = rng.permutation(len(qid))
        qid, scores, target = qid[perm], scores[perm], target[perm]
        m = rank_metrics(scores, target, qid, nq, ks)
        worst, relevant = 0.0, 0
        sums = [[0.0, 0.0, 0.0] for _ in ks]
        for q in range(nq):
            rows = np.flatnonzero(qid == q)
            pos = [bool(target[i] >= 0) for i in rows]
            relevant += 1 if any(pos) else 0
            for j, K in enumerate(ks):
                h, d = _brute([float(scores[i]) for i in rows], pos, K)
                worst = max(worst, abs(m["hits_q"][q][j] - h), abs(m["dcg_q"][q][j] - d))
                if any(pos):
                    ideal = math.fsum(1.0 / math.log2(r + 2.0) for r in range(min(sum(pos), K)))
                    sums[j][0] += d / ideal
                    sums[j][1] += h / sum(pos)
                    sums[j][2] += h / K
        assert m["relevant_queries"] == relevant and relevant > 50
        for j in range(len(ks)):
            for name, s in zip(("ndcg", "recall", "precision"), sums[j]):
                worst = max(worst, abs(m["at"][j][name] - s / relevant))
        print("worst difference", worst)
        assert worst <= 1e-12
        assert any(a["tied_queries"] for a in m["at"])


@pytest.mark.parametrize("K", [1, 3, 8])
def test_tie_free_scores_against_ranking_metrics(K):
    """without ties every run is one row: the three means are those of libfm_amd.ranking.metrics fed with each query's own top-K
    list (padded like fmx_topk's where the query has fewer rows)"""
    from libfm_amd import ranking
    rng = np.random.default_rng(10 + K)
    nq, rows = 40, 400
    qid = rng.integers(0, nq, rows)
    scores = rng.permutation(rows).astype(np.float32) / 8.0              # all distinct
    target = np.where(rng.random(rows) < 0.3, 1.0, -1.0)
    m = rank_metrics(scores, target, qid, nq, (K,))
    idx = np.full((nq, K), 0xFFFFFFFF, dtype=np.uint32)
    ptr, rel = [0], []
    for q in range(nq):
        r = np.flatnonzero(qid == q)
        top = r[np.argsort(-scores[r], kind="stable")][:K]
        idx[q, :len(top)] = top
        rel += [int(i) for i in r if target[i] >= 0]
        ptr.append(len(rel))
    want = ranking.metrics(idx, ptr, rel)
    R = m["relevant_queries"]
    assert R == want["queries"] and R > 30 and m["at"][0]["tied_queries"] == 0
    for name in ("ndcg", "recall", "precision"):
        print(name, m["at"][0][name], want[name])
        assert abs(m["at"][0][name] - want[name]) <= abs(want[name]) * (R + K + 8) * U, name


def test_states_of_the_restatement():
    nan_scores = rank_metrics([0.5, float("nan")], [1, -1], [0, 0], 2, (3,))
    assert nan_scores["relevant_queries"] == 0 and math.isnan(nan_scores["at"][0]["ndcg"]) and nan_scores["hits_q"] == [[0.0], [0.0]]
    assert nan_scores["at"][0]["hits"] == 0.0 and nan_scores["by_query"]["pooled"]["nan_rows"] == 1
    none = rank_metrics([0.5, 0.25], [-1, -1], [0, 1], 2, (3,), per_query=False)
    assert none["relevant_queries"] == 0 and math.isnan(none["at"][0]["recall"]) and none["at"][0]["tied_queries"] == 0
    assert none["hits_q"] is None and none["dcg_q"] is None
    empty = rank_metrics([], [], [], 4, (1, 2))
    assert empty["by_query"]["empty_queries"] == 4 and math.isnan(empty["at"][1]["precision"]) and len(empty["dcg_q"]) == 4
    zero = rank_metrics([0.0, -0.0, 0.0, 0.0], [1, -1, -1, 1], [0] * 4, 1, (1, 3, 9))     # +0 == -0: one run of four
    assert zero["hits_q"][0] == [(2.0 * 1.0) / 4.0, (2.0 * 3.0) / 4.0, 2.0] and [a["tied_queries"] for a in zero["at"]] == [1, 1, 1]
    for bad in ((), (1, 2, 3, 4, 5), (0,), (2, 2), (3, 1), (65537,)):
        with pytest.raises(ValueError):
            rank_metrics([1.0], [1], [0], 1, bad)
    with pytest.raises(ValueError):
        rank_metrics([1.0], [1], [0], 1, (4,), discounts=[0.0, 1.0])
    table = [0.0, 1.0, 1.5]                                              # the caller's table is the one that is used
    assert rank_metrics([2.0, 1.0], [1, 1], [0, 0], 1, (2,), discounts=table)["dcg_q"][0] == [1.5]


@pytest.fixture(scope="module")
def lib():
    from libfm_amd import build, capi
    build.build()
    return capi.load()


def test_discount_table_of_the_library(lib):
    from libfm_amd import capi
    D = capi.rank_discounts(4096)
    assert D.dtype == np.float64 and len(D) == 4097 and D[0] == 0.0 and D[1] == 1.0
    want = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(4096) + 2.0))])
    r = np.arange(4097)
    assert np.all(np.abs(D - want) <= want * (r + 1) * U)
    assert np.all(np.abs(D - np.asarray(rank_discounts(4096))) <= want * (r + 1) * U)     # the restatement's own table
    assert np.array_equal(capi.rank_discounts(10), D[:11]) and len(capi.rank_discounts(0)) == 1
    assert len(capi.rank_discounts(65536)) == 65537
    assert lib.fmx_rank_discounts(4, None) == -1 and b"fmx_rank_discounts" in lib.fmx_last_error(None)
    out = np.zeros(4, dtype=np.float64)
    assert lib.fmx_rank_discounts(65537, out.ctypes.data) == -1 and b"k_max" in lib.fmx_last_error(None) and not out.any()
    with pytest.raises(capi.FmxError) as ei:
        capi.rank_discounts(65537)
    assert ei.value.code == -1 and "fmx_rank_discounts" in ei.value.text


def test_struct_sizes(lib):
    from libfm_amd import capi
    assert C.sizeof(capi.RankOpts) == 32 and C.sizeof(capi.RankAt) == 48
    assert C.sizeof(capi.EvalRank) == C.sizeof(capi.EvalQuery) + 16 + 4 * 48 + 16
    from libfm_amd import evalmetrics, learner
    hdr = open(os.path.join(ROOT, "include", "fmx.h")).read()
    want = (int(re.search(r"#define\s+FMX_RANK_MAX_CUTOFFS\s+(\d+)", hdr).group(1)), int(re.search(r"#define\s+FMX_RANK_MAX_K\s+(\d+)u", hdr).group(1)))
    assert want == (4, 65536)
    for mod in (capi, evalmetrics, learner):                 # the header's two limits, restated in the binding and in the oracle
        assert (mod.RANK_MAX_CUTOFFS, mod.RANK_MAX_K) == want, mod.__name__


def _files(tmp_path):
    tr, te = str(tmp_path / "tr.libfm"), str(tmp_path / "te.libfm")
    for path in (tr, te):
        with open(path, "w") as f:
            for r in range(6):
                f.write("%d %d:1 %d:0.5\n" % (r % 2, r % 3, 3 + r % 2))
    return tr, te


def _refused(capsys, argv, *needles):
    from libfm_amd import cli
    assert cli.main(argv) == 0                               # the reference's convention: "ERROR: ..." on stderr, status 0
    cap = capsys.readouterr()
    assert "ERROR:" in cap.err and "#Iter=" not in cap.out
    for n in needles:
        assert n in cap.err, cap.err


def test_cli_refusals(tmp_path, capsys):
    tr, te = _files(tmp_path)
    qf = str(tmp_path / "q.txt")
    with open(qf, "w") as f:
        f.write("0\n0\n1\n1\n2\n2\n")
    base = ["-train", tr, "-test", te, "-dim", "1,1,2", "-iter", "1", "-learn_rate", "0.05"]
    sgd = base + ["-task", "c", "-method", "sgd", "-test_queries", qf]
    _refused(capsys, base + ["-task", "c", "-method", "sgd", "-rank_at", "5"], "-rank_at needs -test_queries")
    _refused(capsys, sgd + ["-rank_at", "10,5"], "-rank_at", "ascending")
    _refused(capsys, sgd + ["-rank_at", "5,5"], "-rank_at", "ascending")
    _refused(capsys, sgd + ["-rank_at", "0,5"], "-rank_at", "1 .. 65536")
    _refused(capsys, sgd + ["-rank_at", "5,65537"], "-rank_at", "1 .. 65536")
    _refused(capsys, sgd + ["-rank_at", "1,2,3,4,5"], "-rank_at", "1 .. 4 cutoffs")
    _refused(capsys, sgd + ["-rank_at", ""], "-rank_at", "1 .. 4 cutoffs")
    _refused(capsys, sgd + ["-rank_at", "five"], "-rank_at", "integers")
    _refused(capsys, base + ["-task", "c", "-method", "mcmc", "-rank_at", "5"], "-rank_at", "mcmc", "averages the draws")
    _refused(capsys, base + ["-task", "c", "-method", "mcmc", "-rank_at", "5", "-test_queries", qf], "-test_queries", "mcmc")
    _refused(capsys, base + ["-task", "c", "-method", "bpr", "-train_pairs", "x", "-test_pairs", "y", "-rank_at", "5"], "-rank_at", "bpr")
    _refused(capsys, base + ["-task", "r", "-method", "sgd", "-rank_at", "5"], "-rank_at", "-task c")
    _refused(capsys, base + ["-task", "r", "-method", "sgd", "-rank_at", "5", "-test_queries", qf], "-test_queries", "-task c")


def test_cli_help_lists_the_flag(capsys):
    from libfm_amd import cli
    assert cli.main(["-help"]) == 0
    assert "-rank_at" in capsys.readouterr().out
    assert "-rank_at K1,K2" in cli.__doc__
