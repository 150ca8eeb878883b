"""fp64 restatement of top-K retrieval (include/fmx.h, fmx_topk).

score(q, c) is fm_model::predict (fm_model.h:105-127) of the joined row x_q ++ x_c, in two forms:
  explicit   : the joined rows written out and predicted by oracle.predict_raw (the pinned restatement of the reference)
  decomposed : a_q + b_c + S_q . S_c from per-row factor sums, for shapes where the join does not fit
Model: an object with w0, w[n], v[k][n] (float64) and k0, k1 -- oracle.Model fits.  Rows: (entries, row_ptr) as oracle.Data keeps
them (entries: structured id / value, values float32).
select() applies the list rules: descending score, equal scores by the lower candidate index, NaN never returned, excluded
candidates never returned, padding (NONE, -inf) when fewer than K are eligible.
"""
import numpy as np

NONE = 0xFFFFFFFF


def join_rows(q_ent, q_rp, c_ent, c_rp, queries=None):
    """the joined rows x_q ++ x_c for every (q, c) (queries: the subset of query rows, default all), query-major"""
    q_rp = np.asarray(q_rp, dtype=np.int64)
    c_rp = np.asarray(c_rp, dtype=np.int64)
    qs = range(len(q_rp) - 1) if queries is None else queries
    nc = len(c_rp) - 1
    parts, sizes = [], []
    for q in qs:
        xq = q_ent[q_rp[q]:q_rp[q + 1]]
        for c in range(nc):
            xc = c_ent[c_rp[c]:c_rp[c + 1]]
            parts.append(xq)
            parts.append(xc)
            sizes.append(len(xq) + len(xc))
    ent = np.concatenate(parts) if parts else q_ent[:0]
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return ent, rp


def scores_explicit(O, m, q_ent, q_rp, c_ent, c_rp, queries=None):
    """[Q][C] scores through oracle.predict_raw on the materialised joined rows"""
    ent, rp = join_rows(q_ent, q_rp, c_ent, c_rp, queries)
    nq = (len(q_rp) - 1) if queries is None else len(queries)
    nc = len(c_rp) - 1
    d = O.Data(ent, rp, np.zeros(nq * nc, dtype=np.float32))
    return O.predict_raw(m, d).reshape(nq, nc)


def row_sums(m, ent, rp):
    """per row: S [rows][k], lin [rows], 1/2 sum_f (S^2 - SS) [rows]"""
    rp = np.asarray(rp, dtype=np.int64)
    n = len(rp) - 1
    k = m.v.shape[0]
    ids = ent["id"].astype(np.int64)
    xs = ent["value"].astype(np.float32).astype(np.float64)
    row = np.repeat(np.arange(n), np.diff(rp))
    lin = np.bincount(row, weights=m.w[ids] * xs, minlength=n)
    S = np.zeros((n, k))
    SS = np.zeros((n, k))
    for f in range(k):                                            # one factor at a time: [entries] vectors, never [entries][k]
        d = m.v[f, ids] * xs
        S[:, f] = np.bincount(row, weights=d, minlength=n)
        SS[:, f] = np.bincount(row, weights=d * d, minlength=n)
    return S, lin, 0.5 * (S * S - SS).sum(axis=1)


def scores_decomposed(m, q_ent, q_rp, c_ent, c_rp, queries=None):
    """[Q][C] scores as a_q + b_c + S_q . S_c"""
    Sq, lq, hq = row_sums(m, q_ent, q_rp)
    Sc, lc, hc = row_sums(m, c_ent, c_rp)
    if queries is not None:
        Sq, lq, hq = Sq[queries], lq[queries], hq[queries]
    a = (m.w0 if m.k0 else 0.0) + (lq if m.k1 else 0.0) + hq
    b = (lc if m.k1 else 0.0) + hc
    return a[:, None] + b[None, :] + Sq @ Sc.T


def select(scores, K, exclude=None):
    """(idx uint32 [Q][K], score float64 [Q][K]) under the list rules; exclude: per query an iterable of candidate rows"""
    scores = np.asarray(scores, dtype=np.float64)
    Q, C = scores.shape
    idx = np.full((Q, K), NONE, dtype=np.uint32)
    out = np.full((Q, K), -np.inf)
    cand = np.arange(C)
    for q in range(Q):
        s = scores[q]
        ok = ~np.isnan(s)
        if exclude is not None:
            ex = np.asarray(list(exclude[q]), dtype=np.int64)
            ok[ex[(ex >= 0) & (ex < C)]] = False
        c = cand[ok]
        order = np.lexsort((c, -s[ok]))[:K]                     # score descending, then the lower index
        idx[q, :len(order)] = c[order]
        out[q, :len(order)] = s[ok][order]
    return idx, out


def csr_to_lists(ptr, idx):
    ptr = np.asarray(ptr, dtype=np.int64)
    return [np.asarray(idx[ptr[i]:ptr[i + 1]], dtype=np.int64) for i in range(len(ptr) - 1)]
