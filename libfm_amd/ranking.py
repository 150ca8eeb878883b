"""Ranking metrics of top-K lists (host side): what fmx_topk / Handle.topk / learner recommend() return, scored against the
relevant candidates of every query with binary relevance.

    metrics(idx, relevant_ptr, relevant_idx) -> {"recall", "precision", "ndcg", "hit_rate", "queries"}

idx is [n_query, K] (padding entries, capi.TOPK_NONE, count as misses); relevant_ptr [n_query + 1] / relevant_idx are a CSR of
the relevant candidate rows per query (repeats count once).  Per query with at least one relevant candidate:
    precision@K = hits / K,  recall@K = hits / |relevant|,  hit = (hits > 0),
    NDCG@K = sum_{hit at position i} 1 / log2(i + 2)  /  sum_{i < min(|relevant|, K)} 1 / log2(i + 2)
and the four are averaged over those queries ("queries" counts them; queries without relevant candidates are left out).
"""
import numpy as np


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
