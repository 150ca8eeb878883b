"""Ranking metrics of top-K lists (host side): what fmx_topk / Handle.topk / learner recommend() return, scored against the
relevant candidates of every query with binary relevance.

    metrics(idx, relevant_ptr, relevant_idx) -> {"recall", "precision", "ndcg", "hit_rate", "queries"}

idx is [n_query, K] (padding entries, capi.TOPK_NONE, count as misses); relevant_ptr [n_query + 1] / relevant_idx are a CSR of
the relevant candidate rows per query (repeats count once).  Per query with at least one relevant candidate:
    precision@K = hits / K,  recall@K = hits / |relevant|,  hit = (hits > 0),
    NDCG@K = sum_{hit at position i} 1 / log2(i + 2)  /  sum_{i < min(|relevant|, K)} 1 / log2(i + 2)
and the four are averaged over those queries ("queries" counts them; queries without relevant candidates are left out).

    sample_negatives(seed, epoch, q_row, c_row, n_neg, n_cand, exclude=None, draws=1, query_sums=None, cand_sums=None,
                     cand_scal=None) -> (neg uint32 [n * n_neg], forced)

The negatives fmx_pair_epoch_sampled draws on the device for (seed, epoch), restated on the CPU draw for draw (include/fmx.h,
"BPR on query x candidate interactions"); with draws = M > 1 the hardest of the first M accepted draws (FMX_NEG_HARDEST |
FMX_NEG_DRAWS(M)), scored in float64 from the rows' factor sums.
"""
import numpy as np

NEG_ATTEMPTS = 16            # FMX_NEG_ATTEMPTS
_M64 = (1 << 64) - 1


def _mix64(x):
    """the splitmix64 finaliser on uint64 arrays (arithmetic mod 2^64)"""
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _mulhi(u, c):
    """(u * c) >> 64 for uint64 arrays u and an integer 0 <= c < 2^32, without a 128-bit type"""
    c = np.uint64(c)
    hi, lo = u >> np.uint64(32), u & np.uint64(0xFFFFFFFF)
    return (hi * c + ((lo * c) >> np.uint64(32))) >> np.uint64(32)


def _exclude_csr(exclude, n_query):
    if isinstance(exclude, tuple) and len(exclude) == 2:
        return np.asarray(exclude[0], dtype=np.int64), np.asarray(exclude[1], dtype=np.int64)
    lists = [np.asarray(list(e), dtype=np.int64) for e in exclude]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(e) for e in lists])
    return ptr, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64))


def sample_negatives(seed, epoch, q_row, c_row, n_neg, n_cand, exclude=None, draws=1, query_sums=None, cand_sums=None,
                     cand_scal=None):
    """The negatives of one epoch: for pair p = t * n_neg + s of interaction t = (q_row[t], c_row[t]),
        draw(a) = (mix64(seed ^ epoch * 0x9E3779B97F4A7C15 ^ (p * 0xD6E8FEB86659FD93 + a * 0xA24BAED4963EE407 + 0x9FB21C651E98DF25))
                   * n_cand) >> 64
    for the first attempt a < 16 whose draw is neither c_row[t] nor excluded for q_row[t]; when all 16 are rejected the 16th
    draw is used and the pair counts as forced.  exclude: None, a CSR (ptr, idx) over the query rows, or a list of iterables.
    draws = M > 1 (hardest of M): the attempts are walked in order until M draws are accepted (neither c_row[t] nor excluded);
    the negative is the accepted draw d with the highest r = cand_scal[d] + query_sums[q_row[t]] @ cand_sums[d] (float64), where a
    later draw replaces the best only with a strictly greater r, or when the best's r is NaN and its own is not.  query_sums
    [Q, k], cand_sums [n_cand, k] and cand_scal [n_cand] are the rows' factor sums S and the candidates' b = linear term +
    1/2 sum_f (S^2 - sum of squares) of the current model; they are needed for draws > 1 and ignored for draws = 1.
    Returns (neg uint32 [n * n_neg], forced)."""
    draws = int(draws)
    if not 1 <= draws <= NEG_ATTEMPTS:
        raise ValueError("sample_negatives: draws must be in 1 .. %d" % NEG_ATTEMPTS)
    if draws > 1 and (query_sums is None or cand_sums is None or cand_scal is None):
        raise ValueError("sample_negatives: draws > 1 needs query_sums, cand_sums and cand_scal")
    q_row = np.asarray(q_row, dtype=np.int64)
    c_row = np.asarray(c_row, dtype=np.int64)
    n_neg, n_cand = int(n_neg), int(n_cand)
    if q_row.shape != c_row.shape or q_row.ndim != 1:
        raise ValueError("sample_negatives: q_row and c_row must be 1-d arrays of one length")
    if n_neg < 1:
        raise ValueError("sample_negatives: n_neg must be at least 1")
    P = len(q_row) * n_neg
    if P == 0:
        return np.zeros(0, dtype=np.uint32), 0
    if not 0 < n_cand < (1 << 32):
        raise ValueError("sample_negatives: n_cand must be in 1 .. 2^32 - 1")
    p = np.arange(P, dtype=np.uint64)
    qp, cp = np.repeat(q_row, n_neg), np.repeat(c_row, n_neg)
    keys = None
    if exclude is not None:
        ptr, idx = _exclude_csr(exclude, None)
        if len(ptr) - 1 <= int(q_row.max()):
            raise ValueError("sample_negatives: the exclusion lists do not cover every query row")
        idx = idx[ptr[0]:ptr[-1]]
        if len(idx) and not (0 <= int(idx.min()) and int(idx.max()) < n_cand):
            raise ValueError("sample_negatives: an excluded candidate row is outside 0 .. n_cand - 1")   # (FMX_E_ARG on the device)
        owner = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
        keys = np.unique(owner * n_cand + idx)
    base = np.uint64(((int(seed) & _M64) ^ ((int(epoch) * 0x9E3779B97F4A7C15) & _M64)) & _M64)
    if draws > 1:
        Sq = np.asarray(query_sums, dtype=np.float64)
        Sc = np.asarray(cand_sums, dtype=np.float64)
        b = np.asarray(cand_scal, dtype=np.float64)
        if Sq.ndim != 2 or Sc.ndim != 2 or Sq.shape[1] != Sc.shape[1] or Sc.shape[0] != n_cand or b.shape != (n_cand,) \
                or Sq.shape[0] <= int(q_row.max()):
            raise ValueError("sample_negatives: want query_sums [Q, k], cand_sums [n_cand, k] and cand_scal [n_cand]")
        neg = np.zeros(P, dtype=np.uint32)
        best = np.zeros(P)
        have = np.zeros(P, dtype=bool)
        accepted = np.zeros(P, dtype=np.int64)
        Sqp = Sq[qp]
        with np.errstate(over="ignore", invalid="ignore"):
            for a in range(NEG_ATTEMPTS):
                ctr = p * np.uint64(0xD6E8FEB86659FD93) + np.uint64((a * 0xA24BAED4963EE407 + 0x9FB21C651E98DF25) & _M64)
                d = _mulhi(_mix64(base ^ ctr), n_cand).astype(np.int64)
                ok = d != cp
                if keys is not None and len(keys):
                    k = qp * n_cand + d
                    at = np.searchsorted(keys, k)
                    ok &= keys[np.minimum(at, len(keys) - 1)] != k
                ok &= accepted < draws                             # the walk stops after the M-th accepted draw
                accepted += ok
                r = b[d] + np.einsum("pf,pf->p", Sqp, Sc[d])
                take = ok & (~have | (r > best) | (np.isnan(best) & ~np.isnan(r)))
                neg[take] = d[take]
                best[take] = r[take]
                have |= ok
            neg[~have] = d[~have]                                  # nothing accepted: the last draw as it is
        return neg, int((~have).sum())
    neg = np.zeros(P, dtype=np.uint32)
    todo = np.arange(P)
    with np.errstate(over="ignore"):
        for a in range(NEG_ATTEMPTS):
            ctr = p[todo] * np.uint64(0xD6E8FEB86659FD93) + np.uint64((a * 0xA24BAED4963EE407 + 0x9FB21C651E98DF25) & _M64)
            d = _mulhi(_mix64(base ^ ctr), n_cand).astype(np.int64)
            neg[todo] = d
            bad = d == cp[todo]
            if keys is not None and len(keys):
                k = qp[todo] * n_cand + d
                at = np.searchsorted(keys, k)
                bad |= keys[np.minimum(at, len(keys) - 1)] == k
            todo = todo[bad]
            if len(todo) == 0:
                break
    return neg, int(len(todo))


def metrics(idx, relevant_ptr, relevant_idx):
    idx = np.asarray(idx)
    if idx.ndim != 2:
        raise ValueError("metrics: idx must be [n_query, K]")
    n, K = idx.shape
    ptr = np.asarray(relevant_ptr, dtype=np.int64)
    rel = np.asarray(relevant_idx, dtype=np.int64)
    if len(ptr) != n + 1:
        raise ValueError("metrics: relevant_ptr must hold n_query + 1 = %d offsets" % (n + 1))
    disc = 1.0 / np.log2(np.arange(K) + 2.0)
    ideal = np.concatenate([[0.0], np.cumsum(disc)])          # ideal[m] = DCG of m hits at the top
    tot = {"recall": 0.0, "precision": 0.0, "ndcg": 0.0, "hit_rate": 0.0}
    counted = 0
    for q in range(n):
        r = np.unique(rel[ptr[q]:ptr[q + 1]])
        if len(r) == 0:
            continue
        hit = np.isin(idx[q].astype(np.int64), r)                # a padding index (2^32 - 1) is never a candidate row
        h = int(hit.sum())
        tot["recall"] += h / len(r)
        tot["precision"] += h / K if K else 0.0
        tot["ndcg"] += float(disc[hit].sum()) / ideal[min(len(r), K)] if K else 0.0
        tot["hit_rate"] += 1.0 if h else 0.0
        counted += 1
    out = {k: (v / counted if counted else 0.0) for k, v in tot.items()}
    out["queries"] = counted
    return out
