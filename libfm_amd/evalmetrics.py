"""CPU restatement of fmx_evaluate_ex's classification metrics (include/fmx.h): what the tests hold the
device to.  Pure Python on purpose -- the AUC numerator is counted with Python integers, the log loss summed with `math` in fp64.

    classification_metrics(scores, target, link="logistic") -> dict with the fields of fmx_eval_ex
    query_metrics(scores, target, qid, n_queries, link="logistic") -> dict with the fields of fmx_eval_query
    rank_metrics(scores, target, qid, n_queries, cutoffs, link="logistic") -> dict with the fields of fmx_eval_rank (section 20)
    weighted_metrics(scores, target, weights, link="logistic", task=1, ...) -> dict with the fields of fmx_eval_weighted (section 23)

... and of the posterior accumulator (fmx_post_*): PosteriorAverage keeps the three prediction vectors of
fm_learn_mcmc_simultaneous in numpy fp64; posterior_metric / posterior_evaluate_ex score a vector of means.

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


def weighted_metrics(scores, target, weights, link="logistic", task=1, min_target=-math.inf, max_target=math.inf):
    """CPU restatement of fmx_evaluate_weighted (include/fmx.h): a dict with the fields of fmx_eval_weighted.
    weights: one finite weight >= 0 per row, rounded to float32 first (what fmx_set_row_weights stores).  task 1 (classification):
    weight_sum, pos_weight, neg_weight, correct_weight, loss_sum and logloss / accuracy; task 0 (regression): sq_sum, abs_sum and
    rmse / mae of the score clamped to [min_target, max_target] in fp32.  Every sum is math.fsum over fp64 terms c_i * term_i; a
    row of weight 0 adds exactly 0, also where its loss is +inf or its score NaN.  nan_rows > 0 (classification) or
    weight_sum == 0 makes the ratios NaN; the sums and counts stay right."""
    if link not in LINKS:
        raise ValueError("unknown link %r (want one of %s)" % (link, ", ".join(LINKS)))
    p32 = np.asarray(scores, dtype=np.float32).reshape(-1)
    y32 = np.asarray(target, dtype=np.float32).reshape(-1)
    c32 = np.asarray(weights, dtype=np.float64).reshape(-1).astype(np.float32)
    if not (len(p32) == len(y32) == len(c32)):
        raise ValueError("%d scores, %d targets, %d weights" % (len(p32), len(y32), len(c32)))
    if not (np.isfinite(c32).all() and (c32 >= 0).all()):
        raise ValueError("weights must be finite and >= 0")
    c = [float(x) for x in c32]
    y = [float(x) for x in y32]
    rows = len(c)
    wsum = math.fsum(c)
    out = {"rows": rows, "nan_rows": 0, "weight_sum": wsum, "pos_weight": 0.0, "neg_weight": 0.0, "correct_weight": 0.0,
           "loss_sum": 0.0, "sq_sum": 0.0, "abs_sum": 0.0, "logloss": math.nan, "rmse": math.nan, "mae": math.nan,
           "accuracy": math.nan, "device_seconds": 0.0}
    if task == 0:
        pc = np.maximum(np.float32(min_target), np.minimum(np.float32(max_target), p32))     # fm_learn.h:138-139 (a NaN score clamps to max_target)
        pc = np.where(p32 != p32, np.float32(max_target), pc)
        err = [float(a) - b for a, b in zip(pc, y)]
        out["sq_sum"] = math.fsum(w * e * e if w else 0.0 for w, e in zip(c, err))
        out["abs_sum"] = math.fsum(w * abs(e) if w else 0.0 for w, e in zip(c, err))
        if wsum > 0:
            out["rmse"] = math.sqrt(out["sq_sum"] / wsum)
            out["mae"] = out["abs_sum"] / wsum
        return out
    p = [float(x) for x in p32]
    positive = [t >= 0 for t in y]                                    # fm_learn.h:118
    out["nan_rows"] = sum(1 for x in p if x != x)
    out["pos_weight"] = math.fsum(w for w, s in zip(c, positive) if s)
    out["neg_weight"] = math.fsum(w for w, s in zip(c, positive) if not s)
    out["correct_weight"] = math.fsum(w for w, x, t in zip(c, p, y) if (x >= 0 and t >= 0) or (x < 0 and t < 0))
    # (a NaN score of positive weight makes the sum NaN, as on the device; the ratios are NaN then anyway)
    out["loss_sum"] = math.fsum(0.0 if not w else (math.nan if x != x else w * loss_term(x if s else -x, link))
                                for w, x, s in zip(c, p, positive))
    if out["nan_rows"] == 0 and wsum > 0:
        out["logloss"] = out["loss_sum"] / wsum
        out["accuracy"] = out["correct_weight"] / wsum
    return out


def query_metrics(scores, target, qid, n_queries, link="logistic", per_query=True):
    """CPU restatement of fmx_evaluate_by_query (include/fmx.h): a dict with the fields of fmx_eval_query
    (`pooled` is classification_metrics' dict) plus the per-query lists num2_q, pos_q, neg_q [n_queries].  The numerators are
    auc_numerator2 per query in Python integers, the two fp64 sums math.fsum; only the queries that are present are visited, so a
    large n_queries with few rows stays cheap (per_query=False leaves the three lists out: None)."""
    n_queries = int(n_queries)
    q = [int(x) for x in np.asarray(qid).reshape(-1)]
    pooled = classification_metrics(scores, target, link)
    if len(q) != pooled["rows"]:
        raise ValueError("%d query ids for %d rows" % (len(q), pooled["rows"]))
    if not 1 <= n_queries <= 2 ** 31 - 1:
        raise ValueError("n_queries must be in 1 .. 2^31 - 1")
    if q and not 0 <= min(q) <= max(q) < n_queries:
        raise ValueError("a query id outside 0 .. n_queries - 1")
    out = {"pooled": pooled, "queries": n_queries, "valid_queries": 0, "one_class_queries": 0, "empty_queries": 0, "valid_rows": 0,
           "num2_within": 0, "den2_within": 0, "auc_within": math.nan, "gauc": math.nan, "auc_macro": math.nan,
           "device_seconds": 0.0, "rank_seconds": 0.0,
           "num2_q": None, "pos_q": None, "neg_q": None}
    if per_query:
        out["num2_q"], out["pos_q"], out["neg_q"] = [0] * n_queries, [0] * n_queries, [0] * n_queries
    if pooled["rows"] == 0:
        out["empty_queries"] = n_queries
        return out
    if pooled["nan_rows"]:                                            # nothing is sorted: counts 0, arrays zero
        return out
    p = [float(x) for x in np.asarray(scores, dtype=np.float32).reshape(-1)]
    positive = [float(t) >= 0 for t in np.asarray(target, dtype=np.float32).reshape(-1)]
    members = {}
    for i, g in enumerate(q):
        members.setdefault(g, []).append(i)
    weighted, plain = [], []
    for g in sorted(members):
        rows = members[g]
        pos = sum(1 for i in rows if positive[i])
        neg = len(rows) - pos
        if per_query:
            out["pos_q"][g], out["neg_q"][g] = pos, neg
        if not (pos and neg):
            out["one_class_queries"] += 1
            continue
        num2 = auc_numerator2([p[i] for i in rows], [positive[i] for i in rows])
        if per_query:
            out["num2_q"][g] = num2
        auc_q = num2 / (2.0 * float(pos) * float(neg))
        weighted.append(float(len(rows)) * auc_q)
        plain.append(auc_q)
        out["valid_queries"] += 1
        out["valid_rows"] += len(rows)
        out["num2_within"] += num2
        out["den2_within"] += 2 * pos * neg
    out["empty_queries"] = n_queries - len(members)
    if out["valid_queries"]:
        out["auc_within"] = out["num2_within"] / out["den2_within"]
        out["gauc"] = math.fsum(weighted) / out["valid_rows"]
        out["auc_macro"] = math.fsum(plain) / out["valid_queries"]
    return out


# FMX_RANK_MAX_CUTOFFS, FMX_RANK_MAX_K of include/fmx.h, restated: this module is the oracle of the binding and imports none of it
# (tests/test_rank_metrics_cpu.py holds the two pairs equal)
RANK_MAX_CUTOFFS, RANK_MAX_K = 4, 65536


def rank_discounts(k_max):
    """D[0 .. k_max] as fmx_rank_discounts computes it: D[r + 1] = D[r] + 1.0 / log2(r + 2.0), sequentially in fp64"""
    d = [0.0] * (int(k_max) + 1)
    for r in range(int(k_max)):
        d[r + 1] = d[r] + 1.0 / math.log2(float(r) + 2.0)
    return d


def rank_runs(scores, positive):
    """the tie runs of one query by descending score: (a, b, p) with the 0-based ranks [a, b) and p relevant rows among them"""
    order = sorted(range(len(scores)), key=lambda i: -scores[i])
    runs, i = [], 0
    while i < len(order):
        j = i
        while j < len(order) and scores[order[j]] == scores[order[i]]:
            j += 1
        runs.append((i, j, sum(1 for x in order[i:j] if positive[x])))
        i = j
    return runs


def rank_metrics(scores, target, qid, n_queries, cutoffs, link="logistic", discounts=None, per_query=True):
    """CPU restatement of fmx_evaluate_rank (include/fmx.h): a dict with the fields of fmx_eval_rank
    (`by_query` is query_metrics' dict, `at` a list of dicts, one per cutoff) plus the per-query lists dcg_q and hits_q
    [n_queries][n_cutoffs] (per_query=False leaves them out: None).  A tie run at the ranks [a, b) with p relevant rows among its
    t = b - a adds ((double)p * (double)(b' - a')) / (double)t to hits_q and ((double)p * (D[b'] - D[a'])) / (double)t to dcg_q in
    exactly that operation order; a query's sum over its runs and the means over the relevant queries are math.fsum.
    `discounts` is the table D (libfm_amd.capi.rank_discounts gives the library's bits); None computes it here."""
    ks = [int(k) for k in cutoffs]
    if not 1 <= len(ks) <= RANK_MAX_CUTOFFS:
        raise ValueError("1 .. %d cutoffs" % RANK_MAX_CUTOFFS)
    if any(not 1 <= k <= RANK_MAX_K for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError("the cutoffs are strictly ascending integers in 1 .. %d" % RANK_MAX_K)
    D = rank_discounts(ks[-1]) if discounts is None else [float(x) for x in discounts]
    if len(D) < ks[-1] + 1:
        raise ValueError("the discount table has %d entries, the largest cutoff needs %d" % (len(D), ks[-1] + 1))
    n_queries = int(n_queries)
    by_query = query_metrics(scores, target, qid, n_queries, link, per_query=False)
    nan = math.nan
    out = {"by_query": by_query, "relevant_queries": 0, "n_cutoffs": len(ks),
           "at": [{"k": k, "tied_queries": 0, "hits": 0.0, "ndcg": nan, "recall": nan, "precision": nan} for k in ks],
           "device_seconds": 0.0, "topk_seconds": 0.0, "dcg_q": None, "hits_q": None}
    if per_query:
        out["dcg_q"] = [[0.0] * len(ks) for _ in range(n_queries)]
        out["hits_q"] = [[0.0] * len(ks) for _ in range(n_queries)]
    pooled = by_query["pooled"]
    if pooled["rows"] == 0 or pooled["nan_rows"]:                     # nothing is sorted
        return out
    p = [float(x) for x in np.asarray(scores, dtype=np.float32).reshape(-1)]
    positive = [float(t) >= 0 for t in np.asarray(target, dtype=np.float32).reshape(-1)]
    members = {}
    for i, g in enumerate(int(x) for x in np.asarray(qid).reshape(-1)):
        members.setdefault(g, []).append(i)
    sums = [{"hits": [], "ndcg": [], "recall": [], "precision": []} for _ in ks]
    for g in sorted(members):
        rows = members[g]
        pos = sum(1 for i in rows if positive[i])
        if not pos:
            continue
        out["relevant_queries"] += 1
        runs = rank_runs([p[i] for i in rows], [positive[i] for i in rows])
        for j, K in enumerate(ks):
            hit_terms, dcg_terms, tied = [], [], False
            for a, b, rel in runs:
                if a >= K:
                    break
                t, b1 = b - a, min(b, K)
                hit_terms.append((float(rel) * float(b1 - a)) / float(t))
                dcg_terms.append((float(rel) * (D[b1] - D[a])) / float(t))
                tied = tied or 0 < rel < t
            hits_q, dcg_q = math.fsum(hit_terms), math.fsum(dcg_terms)
            if per_query:
                out["hits_q"][g][j], out["dcg_q"][g][j] = hits_q, dcg_q
            sums[j]["hits"].append(hits_q)
            sums[j]["ndcg"].append(dcg_q / D[min(pos, K)])
            sums[j]["recall"].append(hits_q / float(pos))
            sums[j]["precision"].append(hits_q / float(K))
            out["at"][j]["tied_queries"] += 1 if tied else 0
    R = out["relevant_queries"]
    if R:
        for j in range(len(ks)):
            out["at"][j]["hits"] = math.fsum(sums[j]["hits"])
            for name in ("ndcg", "recall", "precision"):
                out["at"][j][name] = math.fsum(sums[j][name]) / float(R)
    return out


# ---- the posterior accumulator (include/fmx.h "fmx_post_*") ---------------------------------------------------------------------
POST_THIS, POST_ALL, POST_LATE = 0, 1, 2
TASK_REGRESSION, TASK_CLASSIFICATION = 0, 1


def _ref_erf(x):
    """the reference's 5-term erf polynomial (random.h:45-59), vectorised."""
    x = np.asarray(x, dtype=np.float64)
    t = np.where(x >= 0, 1.0 / (1.0 + 0.3275911 * x), 1.0 / (1.0 - 0.3275911 * x))
    r = 1.0 - (t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))) * np.exp(-x * x)
    return np.where(x >= 0, r, -r)


def ref_cdf_gaussian(x):
    """random.h:65-67"""
    return 0.5 + 0.5 * _ref_erf(0.707106781 * np.asarray(x, dtype=np.float64))


def posterior_mean(total, count):
    """sum * (1.0 / count): the product with the reciprocal of fm_learn_mcmc_simultaneous.h:278, :296, not a division"""
    return np.asarray(total, dtype=np.float64) * (1.0 / count)


def _clamp(p, lo, hi):
    """std::min / std::max of :132-133 with a NaN let through (numpy's minimum / maximum)"""
    return np.maximum(lo, np.minimum(hi, p))


def _correct(m, y):
    return int(np.count_nonzero(((m >= 0.5) & (y > 0)) | ((m < 0.5) & (y < 0))))               # :297


def posterior_metric(task, mean, target, min_target=0.0, max_target=0.0):
    """fmx_post_metric of a vector of means (None: a vector without draws) against its targets: _evaluate (:272-289) and
    _evaluate_class (:291-309)"""
    nan = math.nan
    if mean is None or len(mean) == 0:
        return {"rows": 0, "nan_rows": 0, "correct": 0, "rmse": nan, "mae": nan, "accuracy": nan, "ll_ref": nan}
    m = np.asarray(mean, dtype=np.float64)
    y = np.asarray(target, dtype=np.float32)[:len(m)].astype(np.float64)
    rows = len(m)
    out = {"rows": rows, "nan_rows": int(np.count_nonzero(m != m)), "correct": 0, "rmse": 0.0, "mae": 0.0, "accuracy": 0.0, "ll_ref": 0.0}
    with np.errstate(all="ignore"):
        if task == TASK_REGRESSION:
            err = _clamp(m, min_target, max_target) - y
            out["rmse"] = math.sqrt(float(np.sum(err * err)) / rows)
            out["mae"] = float(np.sum(np.abs(err))) / rows
        else:
            out["correct"] = _correct(m, y)
            out["accuracy"] = out["correct"] / rows
            w = (y + 1.0) * 0.5
            q = np.where(m > 0.99, 0.99, m)
            q = np.where(q < 0.01, 0.01, q)                               # (a NaN passes both comparisons, :302-303)
            out["ll_ref"] = -float(np.sum(w * np.log10(q) + (1.0 - w) * np.log10(1.0 - q))) / rows
    return out


def posterior_evaluate_ex(task, mean, target, min_target=0.0, max_target=0.0):
    """fmx_eval_ex of a vector of means (None: a vector without draws), as fmx_post_evaluate_ex fills it"""
    out = {"rows": 0, "nan_rows": 0, "pos": 0, "neg": 0, "correct": 0, "auc_num2": 0, "auc": math.nan, "logloss": math.nan,
           "rmse": 0.0, "mae": 0.0, "accuracy": 0.0, "device_seconds": 0.0, "rank_seconds": 0.0, "flags": 0}
    if mean is None or len(mean) == 0:
        return out
    m = np.asarray(mean, dtype=np.float64)
    y = np.asarray(target, dtype=np.float32)[:len(m)].astype(np.float64)
    rows = out["rows"] = len(m)
    out["nan_rows"] = int(np.count_nonzero(m != m))
    with np.errstate(all="ignore"):
        if task == TASK_REGRESSION:
            err = _clamp(m, min_target, max_target) - y
            out["rmse"] = math.sqrt(float(np.sum(err * err)) / rows)
            out["mae"] = float(np.sum(np.abs(err))) / rows
            return out
        positive = y >= 0
        out["pos"] = int(np.count_nonzero(positive))
        out["neg"] = rows - out["pos"]
        out["correct"] = _correct(m, y)
        out["accuracy"] = out["correct"] / rows
        if out["nan_rows"]:
            return out
        out["logloss"] = float(np.sum(np.where(positive, -np.log(m), -np.log(1.0 - m)))) / rows
    if out["pos"] and out["neg"]:
        out["auc_num2"] = auc_numerator2([float(x) for x in m], [bool(b) for b in positive])
        out["auc"] = out["auc_num2"] / (2 * out["pos"] * out["neg"])
    return out


class PosteriorAverage:
    """the accumulator of fmx_post_begin / fmx_post_accumulate on the host: pred_this, pred_sum_all and pred_sum_all_but5 of
    fm_learn_mcmc_simultaneous (:129-161) in numpy fp64, one add per row per draw in draw order"""

    def __init__(self, task, min_target=0.0, max_target=0.0, burn_in=5, eval_rows=0):
        if task not in (TASK_REGRESSION, TASK_CLASSIFICATION):
            raise ValueError("unknown task")
        self.task, self.min_target, self.max_target = task, float(min_target), float(max_target)
        self.burn_in, self.eval_rows = int(burn_in), int(eval_rows)
        self.draws = self.late_draws = 0
        self.this = self.sum_all = self.sum_late = None

    def accumulate(self, p):
        """add one draw: p is the fp32 raw y-hat of every row (fmx_predict's output)"""
        p = np.asarray(p, dtype=np.float32).reshape(-1).astype(np.float64)
        if self.sum_all is None:
            self.sum_all, self.sum_late = np.zeros(len(p)), np.zeros(len(p))
        if len(p) != len(self.sum_all):
            raise ValueError("%d predictions for %d rows" % (len(p), len(self.sum_all)))
        with np.errstate(all="ignore"):
            if self.task == TASK_REGRESSION:
                self.this, v = p, _clamp(p, self.min_target, self.max_target)
            else:
                self.this = v = ref_cdf_gaussian(p)
            self.sum_all = self.sum_all + v
            if self.draws >= self.burn_in:
                self.sum_late = self.sum_late + v
                self.late_draws += 1
        self.draws += 1

    def count(self, which):
        return {POST_THIS: min(self.draws, 1), POST_ALL: self.draws, POST_LATE: self.late_draws}[which]

    def get(self, which):
        """what fmx_post_get copies out: the sum (POST_ALL, POST_LATE) or the last draw itself (POST_THIS)"""
        v = {POST_THIS: self.this, POST_ALL: self.sum_all, POST_LATE: self.sum_late}[which]
        if v is None:
            raise ValueError("no draw has been accumulated")
        return v if self.draws else np.zeros(len(v))

    def mean(self, which):
        """the means of a vector, or None before its first draw"""
        if self.count(which) == 0:
            return None
        return self.this if which == POST_THIS else posterior_mean(self.get(which), self.count(which))

    def _rows(self, m):
        return m if m is None or not self.eval_rows else m[:self.eval_rows]

    def metric(self, which, target):
        return posterior_metric(self.task, self._rows(self.mean(which)), target, self.min_target, self.max_target)

    def evaluate_ex(self, which, target):
        return posterior_evaluate_ex(self.task, self._rows(self.mean(which)), target, self.min_target, self.max_target)
