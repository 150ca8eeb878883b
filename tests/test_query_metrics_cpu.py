"""CPU: libfm_amd.evalmetrics.query_metrics -- the restatement of fmx_evaluate_by_query (include/fmx.h) the GPU
tests hold the device to -- against a hand-sized case pinned to literals, the O(n^2) double loop per query, the degenerate cases
and its identities with classification_metrics; and the command line's refusals of -test_queries / -train_queries that need no
device."""
import math

import numpy as np
import pytest

from libfm_amd.evalmetrics import classification_metrics, query_metrics

MEANS = ("auc_within", "gauc", "auc_macro")


def test_hand_sized_case():
    # query 0: a three-way tie at 0.5 across both classes (+, -, -), a +0 / -0 pair of opposite classes, 2.0 and 3.0 positive,
    #          -1.0 negative: pos 4, neg 4.  Per positive, 2 [p > n] + [p == n] over the negatives {0.5, 0.5, -0.0, -1.0}:
    #          0.5 -> 1 + 1 + 2 + 2 = 6;  +0.0 -> 0 + 0 + 1 + 2 = 3;  2.0 -> 8;  3.0 -> 8.  num2 = 25 of 2 * 4 * 4 = 32.
    # query 1: positives only (2 rows).  query 2: empty.
    rows = [(0, 0.5, +1), (1, 7.0, +1), (0, 0.5, -1), (0, -0.0, -1), (0, 3.0, +1), (0, 0.5, -1), (1, -7.0, +1), (0, 0.0, +1),
            (0, -1.0, -1), (0, 2.0, +1)]
    q, p, y = (np.array(c) for c in zip(*rows))
    m = query_metrics(p.astype(np.float32), y.astype(np.float32), q, 3)
    assert m["num2_q"] == [25, 0, 0] and m["pos_q"] == [4, 2, 0] and m["neg_q"] == [4, 0, 0]
    assert (m["queries"], m["valid_queries"], m["one_class_queries"], m["empty_queries"], m["valid_rows"]) == (3, 1, 1, 1, 8)
    assert (m["num2_within"], m["den2_within"]) == (25, 32)
    assert m["auc_within"] == 0.78125 and m["gauc"] == 0.78125 and m["auc_macro"] == 0.78125
    # pooled: pos 6, neg 4; the two rows of query 1 add 7.0 -> 8 and -7.0 -> 0
    assert (m["pooled"]["pos"], m["pooled"]["neg"], m["pooled"]["auc_num2"]) == (6, 4, 33)
    assert m["pooled"] == classification_metrics(p.astype(np.float32), y.astype(np.float32))


def test_two_valid_queries_are_weighted_by_their_rows():
    # query 0: 1 positive above 1 negative (auc 1, 2 rows); query 1: 1 positive below 3 negatives, tied with 1 (auc 1 / 8, 5 rows)
    q = [0, 0, 1, 1, 1, 1, 1]
    p = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 2.0, 3.0], dtype=np.float32)
    y = np.array([1, -1, 1, -1, -1, -1, -1], dtype=np.float32)
    m = query_metrics(p, y, q, 2)
    assert m["num2_q"] == [2, 1] and m["pos_q"] == [1, 1] and m["neg_q"] == [1, 4]
    assert (m["num2_within"], m["den2_within"], m["valid_rows"]) == (3, 10, 7)
    assert m["auc_within"] == 0.3 and m["auc_macro"] == 0.5625 and m["gauc"] == (2 * 1.0 + 5 * 0.125) / 7


def brute(p, y, q, n_queries):
    num2, pos, neg = [0] * n_queries, [0] * n_queries, [0] * n_queries
    for i in range(len(p)):
        if y[i] >= 0:
            pos[q[i]] += 1
        else:
            neg[q[i]] += 1
    for i in range(len(p)):
        for j in range(len(p)):
            if q[i] == q[j] and y[i] >= 0 and y[j] < 0:
                num2[q[i]] += 2 * (p[i] > p[j]) + (p[i] == p[j])
    return num2, pos, neg


@pytest.mark.parametrize("seed", range(20))
def test_against_the_double_loop(seed):
    rng = np.random.default_rng(seed)
    rows, nq = int(rng.integers(1, 301)), int(rng.integers(1, 41))
    p = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 2.0], dtype=np.float32), rows)      # ties dominate; +0 == -0
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    q = rng.integers(0, nq, rows)
    m = query_metrics(p, y, q, nq)
    num2, pos, neg = brute([float(x) for x in p], [float(t) for t in y], [int(g) for g in q], nq)
    assert (m["num2_q"], m["pos_q"], m["neg_q"]) == ([n if a and b else 0 for n, a, b in zip(num2, pos, neg)], pos, neg)
    valid = [g for g in range(nq) if pos[g] and neg[g]]
    assert m["valid_queries"] == len(valid) and m["valid_rows"] == sum(pos[g] + neg[g] for g in valid)
    assert m["one_class_queries"] == sum(1 for g in range(nq) if (pos[g] == 0) != (neg[g] == 0))
    assert m["empty_queries"] == sum(1 for g in range(nq) if pos[g] + neg[g] == 0)
    assert m["num2_within"] == sum(num2[g] for g in valid) and m["den2_within"] == sum(2 * pos[g] * neg[g] for g in valid)
    if not valid:
        assert all(math.isnan(m[f]) for f in MEANS)
        return
    aucs = [num2[g] / (2.0 * pos[g] * neg[g]) for g in valid]
    assert m["auc_within"] == m["num2_within"] / m["den2_within"]
    assert m["gauc"] == math.fsum((pos[g] + neg[g]) * a for g, a in zip(valid, aucs)) / m["valid_rows"]
    assert m["auc_macro"] == math.fsum(aucs) / len(valid)
    assert 0.0 <= m["gauc"] <= 1.0 and 0.0 <= m["auc_macro"] <= 1.0


def test_nan_scores():
    p = np.array([0.5, np.nan, 1.0, -1.0], dtype=np.float32)
    y = np.array([1, -1, -1, 1], dtype=np.float32)
    m = query_metrics(p, y, [0, 0, 1, 1], 2)
    assert all(math.isnan(m[f]) for f in MEANS)
    assert (m["num2_within"], m["den2_within"], m["valid_queries"], m["one_class_queries"], m["empty_queries"], m["valid_rows"]) == (0,) * 6
    assert m["queries"] == 2 and m["num2_q"] == [0, 0] and m["pos_q"] == [0, 0] and m["neg_q"] == [0, 0]
    assert m["pooled"]["nan_rows"] == 1 and math.isnan(m["pooled"]["auc"]) and (m["pooled"]["pos"], m["pooled"]["neg"]) == (2, 2)


def test_every_query_of_one_class():
    p = np.array([0.5, 0.25, 1.0, -1.0, 3.0], dtype=np.float32)
    y = np.array([1, 1, -1, -1, 1], dtype=np.float32)
    m = query_metrics(p, y, [0, 0, 2, 2, 3], 5)
    assert all(math.isnan(m[f]) for f in MEANS)
    assert (m["valid_queries"], m["one_class_queries"], m["empty_queries"], m["valid_rows"]) == (0, 3, 2, 0)
    assert (m["num2_within"], m["den2_within"]) == (0, 0)
    assert m["pos_q"] == [2, 0, 0, 1, 0] and m["neg_q"] == [0, 0, 2, 0, 0] and m["num2_q"] == [0] * 5
    assert m["pooled"]["auc_num2"] > 0                       # the pooled metric still ranks the classes against each other


def test_n_queries_larger_than_any_id():
    p = np.array([1.0, 0.0, 0.0, 1.0], dtype=np.float32)
    y = np.array([1, -1, 1, -1], dtype=np.float32)
    m = query_metrics(p, y, [5, 5, 9, 9], 2 ** 31 - 1, per_query=False)        # stays cheap: only queries 5 and 9 are visited
    assert m["num2_q"] is None and m["pos_q"] is None and m["neg_q"] is None
    assert (m["queries"], m["valid_queries"], m["one_class_queries"], m["empty_queries"]) == (2 ** 31 - 1, 2, 0, 2 ** 31 - 3)
    assert (m["num2_within"], m["den2_within"], m["gauc"], m["auc_macro"], m["auc_within"]) == (2, 4, 0.5, 0.5, 0.5)
    m = query_metrics(p, y, [5, 5, 9, 9], 12)
    assert m["num2_q"] == [0] * 5 + [2] + [0] * 6 and m["pos_q"][9] == 1 and m["neg_q"][5] == 1 and m["empty_queries"] == 10
    with pytest.raises(ValueError):
        query_metrics(p, y, [5, 5, 9, 9], 9)
    with pytest.raises(ValueError):
        query_metrics(p, y, [5, 5, 9], 12)
    m = query_metrics(p[:0], y[:0], [], 4)                     # no rows: every query is empty
    assert (m["queries"], m["empty_queries"], m["valid_queries"]) == (4, 4, 0) and math.isnan(m["gauc"]) and m["pos_q"] == [0] * 4


@pytest.mark.parametrize("link", ["logistic", "probit"])
def test_identities(link):
    rng = np.random.default_rng(7)
    p = rng.choice(np.array([-1.0, 0.0, 0.5, 0.75], dtype=np.float32), 200)
    y = np.where(rng.random(200) < 0.3, 1.0, -1.0).astype(np.float32)
    m = query_metrics(p, y, rng.integers(0, 9, 200), 9, link)
    assert m["pooled"] == classification_metrics(p, y, link)
    one = query_metrics(p, y, np.zeros(200, dtype=np.uint32), 1, link)
    assert one["num2_within"] == one["pooled"]["auc_num2"] == one["num2_q"][0]
    assert one["gauc"] == one["auc_macro"] == one["auc_within"] == one["pooled"]["auc"]
    assert (one["valid_queries"], one["valid_rows"]) == (1, 200)


# ---- the command line's refusals that need no device -----------------------------------------------------------------------------
def _files(tmp_path, rows=6):
    tr, te = str(tmp_path / "tr.libfm"), str(tmp_path / "te.libfm")
    for path in (tr, te):
        with open(path, "w") as f:
            for r in range(rows):
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
    base = ["-train", tr, "-test", te, "-dim", "1,1,2", "-iter", "1", "-learn_rate", "0.05", "-test_queries", qf]
    _refused(capsys, base + ["-task", "c", "-method", "mcmc"], "-test_queries", "mcmc")
    _refused(capsys, base + ["-task", "c", "-method", "bpr", "-train_pairs", "x", "-test_pairs", "y"], "-test_queries", "bpr")
    _refused(capsys, base + ["-task", "r", "-method", "sgd"], "-test_queries", "-task c")
    _refused(capsys, ["-train", tr, "-test", te, "-task", "c", "-method", "sgd", "-learn_rate", "0.05", "-train_queries", qf],
             "-train_queries needs -test_queries")
    short = str(tmp_path / "short.txt")
    with open(short, "w") as f:
        f.write("0\n0\n1\n1\n2\n")
    _refused(capsys, base[:-1] + [short, "-task", "c", "-method", "sgd"], "5 lines", "6 rows")
    _refused(capsys, base + ["-task", "c", "-method", "sgd", "-train_queries", short], "5 lines", "6 rows")
    neg = str(tmp_path / "neg.txt")
    with open(neg, "w") as f:
        f.write("0\n0\n-1\n1\n2\n2\n")
    _refused(capsys, base[:-1] + [neg, "-task", "c", "-method", "sgd"], "line 3", "query id")


def test_cli_help_lists_the_flags(capsys):
    from libfm_amd import cli
    assert cli.main(["-help"]) == 0
    out = capsys.readouterr().out
    assert "-test_queries" in out and "-train_queries" in out
