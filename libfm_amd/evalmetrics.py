"""CPU restatement of fmx_evaluate_ex's classification metrics (include/fmx.h): what the tests hold the
device to.  Pure Python on purpose -- the AUC numerator is counted with Python integers, the log loss summed with `math` in fp64.

    classification_metrics(scores, target, link="logistic") -> dict with the fields of fmx_eval_ex

`scores` are taken as the fp32 raw y-hat the device returns (they are rounded to float32 first, which is the identity on
fmx_predict's output); s_i = +1 if target_i >= 0 else -1.
"""
import math

import numpy as np

LINKS = ("logistic", "probit")


def loss_term(z, link="logistic"):
    """l(z) of one row, z = s * p: -ln sigmoid(z) (logistic) or -ln Phi(z) as computed through erfc (probit: +inf where erfc
    underflows)"""
    if link == "logistic":
        return max(-z, 0.0) + math.log1p(math.exp(-abs(z)))
    if link == "probit":
        q = 0.5 * math.erfc(-z / math.sqrt(2.0))
        return -math.log(q) if q > 0.0 else math.inf
    raise ValueError("unknown link %r (want one of %s)" % (link, ", ".join(LINKS)))


def auc_numerator2(scores, positive):
    """sum over (positive i, negative j) of 2 [p_i > p_j] + [p_i == p_j] as a Python integer: one sort, then run counting on the
    float values (+0 == -0).  No NaN among the scores."""
    order = sorted(range(len(scores)), key=lambda i: scores[i])
    num2, neg_below, i = 0, 0, 0
    while i < len(order):
        j, pos_run, neg_run = i, 0, 0
        while j < len(order) and scores[order[j]] == scores[order[i]]:
            if positive[order[j]]:
                pos_run += 1
            else:
                neg_run += 1
            j += 1
        num2 += pos_run * (2 * neg_below + neg_run)
        neg_below += neg_run
        i = j
    return num2


def classification_metrics(scores, target, link="logistic"):
    if link not in LINKS:
        raise ValueError("unknown link %r (want one of %s)" % (link, ", ".join(LINKS)))
    p = [float(x) for x in np.asarray(scores, dtype=np.float32).reshape(-1)]
    y = [float(x) for x in np.asarray(target, dtype=np.float32).reshape(-1)]
    if len(p) != len(y):
        raise ValueError("%d scores for %d targets" % (len(p), len(y)))
    rows = len(p)
    positive = [t >= 0 for t in y]                                    # fm_learn.h:118
    pos = sum(positive)
    neg = rows - pos
    nan_rows = sum(1 for x in p if x != x)
    correct = sum(1 for x, t in zip(p, y) if (x >= 0 and t >= 0) or (x < 0 and t < 0))   # a NaN score is never correct
    out = {"rows": rows, "nan_rows": nan_rows, "pos": pos, "neg": neg, "correct": correct, "auc_num2": 0,
           "auc": math.nan, "logloss": math.nan, "rmse": 0.0, "mae": 0.0, "accuracy": correct / rows if rows else 0.0,
           "device_seconds": 0.0, "rank_seconds": 0.0, "flags": 0}
    if rows == 0 or nan_rows:
        return out
    out["auc_num2"] = auc_numerator2(p, positive)
    if pos and neg:
        out["auc"] = out["auc_num2"] / (2 * pos * neg)
    out["logloss"] = math.fsum(loss_term(x if s else -x, link) for x, s in zip(p, positive)) / rows
    return out

