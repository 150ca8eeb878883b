"""One BPR epoch with fresh negatives on the MI355X: the route through fmx_upload_pairs against fmx_pair_epoch_sampled.

    python scripts/bpr_sampled_rate.py [--queries 1048576] [--cands 1048576] [--pairs 2097152] [--batch 65536]
                                       [--draws M[,M..]] [--no-pairs-route] [--quality E]

Shape of scripts/bpr_rate.py: n = 1e7 features, k = 64, query and candidate rows of 16 one-hot entries each (fmx_synth_rows), so a
joined row has 32; one negative per interaction.  Both routes run in this process on one handle each, one warm-up epoch, then the
median wall time of --epochs epochs:

  (a) pairs route: the joined rows x_q ++ x_c+ (row 2p) and x_q ++ x_c- (row 2p + 1) of every pair are written into a slot ONCE,
      outside the timing (which favours this route: new negatives would need new joined rows).  Timed per epoch: the host draw
      (numpy, one re-draw of the negatives equal to the positive), fmx_upload_pairs, fmx_pair_epoch including its bucketing.
  (b) fmx_pair_epoch_sampled on the query and candidate slots; its setup_seconds (sampling, key expansion, sort) and
      device_seconds (sums + apply) are reported separately.

--draws M: after (b), the same epochs with every negative the hardest of M accepted draws
(FMX_NEG_HARDEST | FMX_NEG_DRAWS(M)) on a fresh handle in the same process: wall, setup_seconds (now with the row tables and
k_neg_pick) and device_seconds next to the uniform sampler's.  --no-pairs-route leaves (a) out.
--quality E: instead of the timing, recall@20 (Handle.topk + ranking.metrics, training interactions excluded) on the held-out
10 % of a planted data set after E epochs of the uniform sampler and of each M: users and items as one-hot rows, a user's
interactions = its --q-top best items under a hidden rank-8 model plus Gumbel noise (a draw from the softmax of the scores).

Prints one JSON line.  Device memory of (b): 20 B per pair + 40 B per expanded entry (|x_q| + |x_c+| + |x_c-| = 48 per pair here)
+ the radix sort's temporary; (a) holds the joined rows (8 B x 64 per pair) and 36 B per expanded entry (64 per pair).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libfm_amd import capi  # noqa: E402


def quality(a, draws, seed=5, K=20):
    """recall@K on the held-out tenth of a planted data set after a.quality epochs of each sampler (1 = uniform)"""
    from libfm_amd import ranking
    nu, ni, top = a.q_users, a.q_items, a.q_top
    rng = np.random.default_rng(seed)
    pu, qi = rng.normal(0, 1.0, (nu, 8)), rng.normal(0, 1.0, (ni, 8))
    liked = np.empty((nu, top), dtype=np.int64)
    for u0 in range(0, nu, 1024):                                  # top items of score + Gumbel noise: a softmax draw without replacement
        sc = pu[u0:u0 + 1024] @ qi.T + rng.gumbel(0, 1, (len(pu[u0:u0 + 1024]), ni))
        liked[u0:u0 + 1024] = np.argsort(-sc, axis=1)[:, :top]
    held = np.zeros((nu, top), bool)
    held[:, :max(top // 10, 1)] = True                             # (argsort order is by noisy score; shuffle which are held out)
    held = rng.permuted(held, axis=1)
    users = np.repeat(np.arange(nu), top).reshape(nu, top)
    tr_q, tr_c, te_q, te_c = users[~held], liked[~held], users[held], liked[held]
    order = rng.permutation(len(tr_q))
    tr_q, tr_c = tr_q[order].astype(np.uint32), tr_c[order].astype(np.uint32)
    n = nu + ni
    ent_q = np.zeros(nu, dtype=capi.ENTRY_DTYPE)
    ent_q["id"], ent_q["value"] = np.arange(nu), 1.0
    ent_c = np.zeros(ni, dtype=capi.ENTRY_DTYPE)
    ent_c["id"], ent_c["value"] = nu + np.arange(ni), 1.0
    ex_ptr = np.concatenate([[0], np.cumsum(np.bincount(tr_q, minlength=nu))]).astype(np.uint64)
    ex_idx = tr_c[np.argsort(tr_q, kind="stable")]
    rel_ptr = np.concatenate([[0], np.cumsum(np.bincount(te_q, minlength=nu))])
    rel_idx = te_c[np.argsort(te_q, kind="stable")]
    out = dict(users=nu, items=ni, interactions=int(len(tr_q)), held_out=int(len(te_q)), k=a.q_k, batch=a.q_batch, lr=a.q_lr,
               epochs=a.quality, seed=seed, K=K)
    for M in [1] + [m for m in draws if m != 1]:
        h = capi.Handle(n, a.q_k, False, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.002, a.q_lr, -1.0, 1.0, device=0)
        h.init_params(0.0, 0.1, 1)
        h.upload_rows(0, ent_q, np.arange(nu + 1, dtype=np.uint64), None)
        h.upload_rows(1, ent_c, np.arange(ni + 1, dtype=np.uint64), None)
        h.upload_interactions(0, 1, tr_q, tr_c, (ex_ptr, ex_idx))
        t0 = time.perf_counter()
        for ep in range(a.quality):
            h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, a.q_batch, 1, seed, ep, draws=M)
        h.synchronize()
        t1 = time.perf_counter()
        ev = h.pair_evaluate_sampled(0, 1, seed, 1 << 32)         # uniform negatives on one fixed epoch, for every sampler
        idx, _ = h.topk(0, 1, K, exclude=(ex_ptr, ex_idx))
        h.close()
        m = ranking.metrics(idx, rel_ptr, rel_idx)
        out["draws%d" % M] = dict(recall=m["recall"], ndcg=m["ndcg"], train_seconds=t1 - t0, uniform_pair_accuracy=ev.accuracy,
                                  uniform_pair_loss=ev.loss)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--nnz", type=int, default=16)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--cands", type=int, default=1 << 20)
    ap.add_argument("--pairs", type=int, default=1 << 21)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--draws", type=str, default="", help="hardest of M: one M or a comma-separated list (2 .. 16)")
    ap.add_argument("--no-pairs-route", action="store_true")
    ap.add_argument("--quality", type=int, default=0, help="epochs of the quality run (0: the timing run)")
    ap.add_argument("--q-users", type=int, default=20000)
    ap.add_argument("--q-items", type=int, default=5000)
    ap.add_argument("--q-top", type=int, default=30)
    ap.add_argument("--q-k", type=int, default=16)
    ap.add_argument("--q-batch", type=int, default=4096)
    ap.add_argument("--q-lr", type=float, default=0.05)
    a = ap.parse_args()
    draws = [int(x) for x in a.draws.split(",") if x]
    if a.quality:
        print(json.dumps(quality(a, draws)))
        return
    rng = np.random.default_rng(5)
    q = rng.integers(0, a.queries, a.pairs).astype(np.uint32)
    c = rng.integers(0, a.cands, a.pairs).astype(np.uint32)
    out = dict(n=a.n, k=a.k, nnz=a.nnz, queries=a.queries, cands=a.cands, pairs=a.pairs, batch=a.batch)

    def make():
        h = capi.Handle(a.n, a.k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0, device=0)
        h.init_params(0.0, 0.01, 1)
        h.synth_rows(0, 7, 0, a.queries, a.nnz)
        h.synth_rows(1, 8, 0, a.cands, a.nnz)
        return h

    # (b) ----------------------------------------------------------------------------------------------------------------
    h = make()
    h.upload_interactions(0, 1, q, c)
    neg0, forced = h.pair_sample(0, 1, 1, 0)
    assert forced == 0
    h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, a.batch, 1, 1, 0)
    wall, setup, dev = [], [], []
    for ep in range(1, a.epochs + 1):
        h.synchronize()
        t0 = time.perf_counter()
        st, forced = h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, a.batch, 1, 1, ep)
        wall.append(time.perf_counter() - t0)
        setup.append(st.setup_seconds)
        dev.append(st.device_seconds)
        assert forced == 0
    out["b_sampled_seconds"] = float(np.median(wall))
    out["b_setup_seconds"] = float(np.median(setup))
    out["b_device_seconds"] = float(np.median(dev))
    out["b_all_wall"] = wall
    if not a.no_pairs_route:
        qe, qrp, _ = h.download_rows(0)
        ce, crp, _ = h.download_rows(1)
    h.close()

    # hardest of M: the same epochs on a fresh handle ------------------------------------------------------------------------
    for M in draws:
        h = make()
        h.upload_interactions(0, 1, q, c)
        h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, a.batch, 1, 1, 0, draws=M)
        wall, setup, dev = [], [], []
        for ep in range(1, a.epochs + 1):
            h.synchronize()
            t0 = time.perf_counter()
            st, forced = h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, a.batch, 1, 1, ep, draws=M)
            wall.append(time.perf_counter() - t0)
            setup.append(st.setup_seconds)
            dev.append(st.device_seconds)
            assert forced == 0
        h.close()
        out["hard%d_seconds" % M] = float(np.median(wall))
        out["hard%d_setup_seconds" % M] = float(np.median(setup))
        out["hard%d_device_seconds" % M] = float(np.median(dev))
        out["hard%d_over_b" % M] = out["hard%d_seconds" % M] / out["b_sampled_seconds"]
    if a.no_pairs_route:
        print(json.dumps(out))
        return

    # (a): the join for the negatives of epoch 0, materialised once ---------------------------------------------------------------
    qe, ce = qe.reshape(a.queries, a.nnz), ce.reshape(a.cands, a.nnz)
    join = np.empty((a.pairs, 2, 2 * a.nnz), dtype=capi.ENTRY_DTYPE)
    join[:, 0, :a.nnz] = qe[q]
    join[:, 1, :a.nnz] = qe[q]
    join[:, 0, a.nnz:] = ce[c]
    join[:, 1, a.nnz:] = ce[neg0]
    h = capi.Handle(a.n, a.k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0, device=0)
    h.init_params(0.0, 0.01, 1)
    h.upload_rows(0, join.reshape(-1), np.arange(2 * a.pairs + 1, dtype=np.uint64) * np.uint64(2 * a.nnz), None)
    del join
    pa = np.arange(0, 2 * a.pairs, 2, dtype=np.uint32)
    pb = pa + np.uint32(1)
    wall, parts = [], []
    for ep in range(a.epochs + 1):
        h.synchronize()
        t0 = time.perf_counter()
        neg = rng.integers(0, a.cands, a.pairs).astype(np.uint32)        # the host draw: uniform, the positive re-drawn once
        same = neg == c
        neg[same] = rng.integers(0, a.cands, int(same.sum()))
        t1 = time.perf_counter()
        h.upload_pairs(0, pa, pb)                                         # (the rows of this draw would be 2p, 2p + 1 again)
        t2 = time.perf_counter()
        st = h.pair_epoch(0, capi.SGD_MINIBATCH, a.batch)
        t3 = time.perf_counter()
        if ep:                                                            # epoch 0 is the warm-up
            wall.append(t3 - t0)
            parts.append((t1 - t0, t2 - t1, t3 - t2, st.setup_seconds, st.device_seconds))
    h.close()
    med = np.median(np.array(parts), axis=0)
    out["a_pairs_route_seconds"] = float(np.median(wall))
    out["a_draw_seconds"], out["a_upload_pairs_seconds"], out["a_pair_epoch_seconds"] = float(med[0]), float(med[1]), float(med[2])
    out["a_setup_seconds"], out["a_device_seconds"] = float(med[3]), float(med[4])
    out["a_all_wall"] = wall
    out["b_over_a"] = out["b_sampled_seconds"] / out["a_pairs_route_seconds"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
