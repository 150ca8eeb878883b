"""The yardstick of fmx_pair_epoch_sampled: the joined rows x_q ++ x_c written out on the host, the negatives of
ranking.sample_negatives, and tests/bpr_oracle.py (the loop around fm_pairSGD / the batch rule) on those rows."""
import numpy as np

import bpr_oracle as B
from libfm_amd.ranking import sample_negatives


def join_rows(q_ent, q_rp, c_ent, c_rp, q, c, neg, n_neg):
    """pair p = t * n_neg + s as two materialised rows: row 2p = x_q[t] ++ x_c[t], row 2p + 1 = x_q[t] ++ x_neg[p] (query
    entries first).  Returns (entries, row_ptr, pair_a, pair_b)."""
    parts, sizes = [], []
    for p, d in enumerate(neg):
        t = p // n_neg
        xq = q_ent[int(q_rp[q[t]]):int(q_rp[q[t] + 1])]
        for r in (int(c[t]), int(d)):
            xc = c_ent[int(c_rp[r]):int(c_rp[r + 1])]
            parts += [xq, xc]
            sizes.append(len(xq) + len(xc))
    ent = np.concatenate(parts) if parts else np.zeros(0, dtype=q_ent.dtype)
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    P = len(neg)
    return ent, rp, np.arange(0, 2 * P, 2, dtype=np.uint32), np.arange(1, 2 * P, 2, dtype=np.uint32)


def epoch_pairs(q_ent, q_rp, c_ent, c_rp, q, c, n_neg, seed, epoch, exclude=None):
    """the joined rows and pairs of one epoch with the specification's negatives: (entries, row_ptr, pair_a, pair_b, neg, forced)"""
    neg, forced = sample_negatives(seed, epoch, q, c, n_neg, len(c_rp) - 1, exclude)
    return join_rows(q_ent, q_rp, c_ent, c_rp, q, c, neg, n_neg) + (neg, forced)


def epoch(m, q_ent, q_rp, c_ent, c_rp, q, c, n_neg, seed, ep, lr, batch=None, exclude=None):
    """one epoch on model m: batch None = the loop (FMX_SGD_SEQUENTIAL), else the batch rule with B = batch; returns forced"""
    ent, rp, pa, pb, _, forced = epoch_pairs(q_ent, q_rp, c_ent, c_rp, q, c, n_neg, seed, ep, exclude)
    if batch is None:
        B.pair_epoch_loop(m, ent, rp, pa, pb, lr)
    else:
        B.pair_epoch_batch(m, ent, rp, pa, pb, lr, batch)
    return forced
