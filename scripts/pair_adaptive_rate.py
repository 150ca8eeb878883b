"""The pair epochs stepped by a session's rule (fmx_adapt_pair_epoch*, fmx_ftrl_pair_epoch*) next to the plain ones on the MI355X.

    python scripts/pair_adaptive_rate.py [--stored] [--sampled] [--converge]        (none given: all three)

--stored    scripts/bpr_rate.py's shape (n = 1e7, k = 64, 32 one-hot entries per row, 2^21 rows and pairs, B = 65 536): pairs/s of
            fmx_pair_epoch, fmx_adapt_pair_epoch and fmx_ftrl_pair_epoch in one process on one handle (median device_seconds of
            --epochs epochs after a warm-up epoch each).
--sampled   scripts/bpr_sampled_rate.py's shape (query and candidate rows of 16 entries, 2^20 each, 2^21 interactions, one negative):
            the same for fmx_pair_epoch_sampled and its two rule forms; device_seconds (sums + owner) and wall seconds per epoch.
--converge  popularity-skewed implicit feedback (users and items as one-hot rows; a user's interactions are its --top best items under
            a hidden rank-8 model plus an item bias that falls with the item's rank plus Gumbel noise; a tenth held out): plain BPR over
            a grid of rates and AdaGrad at two etas, at B = 1 024 and B = 65 536, --conv-epochs epochs each; per run the held-out and
            train pair loss and accuracy of fmx_pair_evaluate_sampled (uniform negatives of one fixed epoch, all of a user's
            interactions excluded).
Byte model of the owner per (batch, feature) segment: the plain owner reads and writes one V row (2 rows); a rule's owner reads and
writes the V row and NT state rows (2 + 2 NT rows: 4 for AdaGrad, 6 for FTRL), plus 8 B / 8 NT B more for w_j.  Prints one JSON line
per part."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libfm_amd import capi  # noqa: E402

FTRL = dict(alpha=0.01, beta=1.0, l1_w=0.0, l1_v=0.0, l2_w=0.0, l2_v=0.001)


def timed(fn, epochs):
    fn()
    dev, wall = [], []
    for _ in range(epochs):
        t0 = time.perf_counter()
        st = fn()
        wall.append(time.perf_counter() - t0)
        dev.append(st.device_seconds)
    return float(np.median(dev)), float(np.median(wall))


def stored(a):
    n, k, nnz, rows, pairs = 10_000_000, 64, 32, 1 << 21, 1 << 21
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0, device=0)
    h.init_params(0.0, 0.01, 1)
    h.synth_rows(0, 7, 0, rows, nnz)
    rng = np.random.default_rng(5)
    h.upload_pairs(0, rng.integers(0, rows, pairs).astype(np.uint32), rng.integers(0, rows, pairs).astype(np.uint32))
    out = dict(part="stored", n=n, k=k, nnz=nnz, rows=rows, pairs=pairs, batch=a.batch)
    d, _ = timed(lambda: h.pair_epoch(0, capi.SGD_MINIBATCH, a.batch), a.epochs)
    out["plain_pairs_per_s"] = pairs / d
    h.adapt_begin("adagrad", 1.0, 0.01)
    d, _ = timed(lambda: h.adapt_pair_epoch(0, a.batch), a.epochs)
    out["adagrad_pairs_per_s"] = pairs / d
    h.adapt_end()
    h.ftrl_begin(**FTRL)
    d, _ = timed(lambda: h.ftrl_pair_epoch(0, a.batch), a.epochs)
    out["ftrl_pairs_per_s"] = pairs / d
    h.close()
    out["adagrad_over_plain"] = out["adagrad_pairs_per_s"] / out["plain_pairs_per_s"]
    out["ftrl_over_plain"] = out["ftrl_pairs_per_s"] / out["plain_pairs_per_s"]
    # bytes per pair: scripts/bpr_rate.py's model, the owner's D segments per pair moving 2 + 2 NT rows instead of 2
    E, row = 2 * nnz, 4 * k
    for name, nt in (("plain", 0), ("adagrad", 1), ("ftrl", 2)):
        b = E * (8 + row + 4) + 2 * row + 8 + E * (8 + row) + E * ((2 + 2 * nt) * row + 8 * (1 + nt))
        out[name + "_bytes_per_pair"] = b
        out[name + "_roofline_fraction"] = b * out[name + "_pairs_per_s"] / 8.0e12
    print(json.dumps(out), flush=True)


def sampled(a):
    n, k, nnz, Q, C, pairs = 10_000_000, 64, 16, 1 << 20, 1 << 20, 1 << 21
    rng = np.random.default_rng(5)
    q, c = rng.integers(0, Q, pairs).astype(np.uint32), rng.integers(0, C, pairs).astype(np.uint32)
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0, device=0)
    h.init_params(0.0, 0.01, 1)
    h.synth_rows(0, 7, 0, Q, nnz)
    h.synth_rows(1, 8, 0, C, nnz)
    h.upload_interactions(0, 1, q, c)
    out = dict(part="sampled", n=n, k=k, nnz=nnz, queries=Q, cands=C, pairs=pairs, batch=a.batch)
    ep = [0]

    def run(fn):
        def one():
            ep[0] += 1
            return fn(ep[0])[0]
        return timed(one, a.epochs)
    d, w = run(lambda e: h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, a.batch, 1, 1, e))
    out["plain_device_pairs_per_s"], out["plain_wall_pairs_per_s"] = pairs / d, pairs / w
    h.adapt_begin("adagrad", 1.0, 0.01)
    d, w = run(lambda e: h.adapt_pair_epoch_sampled(0, a.batch, 1, 1, e))
    out["adagrad_device_pairs_per_s"], out["adagrad_wall_pairs_per_s"] = pairs / d, pairs / w
    h.adapt_end()
    h.ftrl_begin(**FTRL)
    d, w = run(lambda e: h.ftrl_pair_epoch_sampled(0, a.batch, 1, 1, e))
    out["ftrl_device_pairs_per_s"], out["ftrl_wall_pairs_per_s"] = pairs / d, pairs / w
    h.close()
    out["adagrad_over_plain_device"] = out["adagrad_device_pairs_per_s"] / out["plain_device_pairs_per_s"]
    out["ftrl_over_plain_device"] = out["ftrl_device_pairs_per_s"] / out["plain_device_pairs_per_s"]
    print(json.dumps(out), flush=True)


def converge(a):
    nu, ni, top, k, seed = a.users, a.items, a.top, 16, 5
    rng = np.random.default_rng(seed)
    pu, qi = rng.normal(0, 1.0, (nu, 8)), rng.normal(0, 1.0, (ni, 8))
    bias = 3.0 * np.log(1.0 / (1.0 + np.arange(ni)) ** 1.2)              # popularity: the item's rank
    bias -= bias.mean()
    liked = np.empty((nu, top), dtype=np.int64)
    for u0 in range(0, nu, 1024):
        sc = pu[u0:u0 + 1024] @ qi.T + bias + rng.gumbel(0, 1, (len(pu[u0:u0 + 1024]), ni))
        liked[u0:u0 + 1024] = np.argsort(-sc, axis=1)[:, :top]
    held = np.zeros((nu, top), bool)
    held[:, :max(top // 10, 1)] = True
    held = rng.permuted(held, axis=1)
    users = np.repeat(np.arange(nu), top).reshape(nu, top)
    tr_q, tr_c, te_q, te_c = users[~held], liked[~held], users[held], liked[held]
    order = rng.permutation(len(tr_q))
    tr_q, tr_c = tr_q[order].astype(np.uint32), tr_c[order].astype(np.uint32)
    te_q, te_c = te_q.astype(np.uint32), te_c.astype(np.uint32)
    share = np.sort(np.bincount(tr_c, minlength=ni))[::-1]
    ent_q = np.zeros(nu, dtype=capi.ENTRY_DTYPE)
    ent_q["id"], ent_q["value"] = np.arange(nu), 1.0
    ent_c = np.zeros(ni, dtype=capi.ENTRY_DTYPE)
    ent_c["id"], ent_c["value"] = nu + np.arange(ni), 1.0
    all_q, all_c = users.reshape(-1), liked.reshape(-1)
    ex_ptr = np.concatenate([[0], np.cumsum(np.bincount(all_q, minlength=nu))]).astype(np.uint64)
    ex_idx = all_c[np.argsort(all_q, kind="stable")].astype(np.uint32)
    head = dict(part="converge", users=nu, items=ni, interactions=int(len(tr_q)), held_out=int(len(te_q)), k=k, epochs=a.conv_epochs,
                top_item_share=float(share[0] / len(tr_c)), top_1pct_items_share=float(share[:max(ni // 100, 1)].sum() / len(tr_c)))
    runs = []
    for B in (1024, 65536):
        for rule, rate in [("plain", r) for r in (0.4, 0.2, 0.1, 0.05, 0.025, 0.0125, 0.00625)] + [("adagrad", 0.1), ("adagrad", 0.05)]:
            h = capi.Handle(nu + ni, k, False, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.002, rate, -1.0, 1.0, device=0)
            h.init_params(0.0, 0.1, 1)
            h.upload_rows(0, ent_q, np.arange(nu + 1, dtype=np.uint64), None)
            h.upload_rows(1, ent_c, np.arange(ni + 1, dtype=np.uint64), None)
            h.upload_rows(2, ent_q, np.arange(nu + 1, dtype=np.uint64), None)
            h.upload_interactions(0, 1, tr_q, tr_c, (ex_ptr, ex_idx))
            h.upload_interactions(2, 1, te_q, te_c, (ex_ptr, ex_idx))
            if rule == "adagrad":
                h.adapt_begin("adagrad", 1.0, rate)
            curve = []
            for ep in range(a.conv_epochs):
                if rule == "adagrad":
                    h.adapt_pair_epoch_sampled(0, B, 1, seed, ep)
                else:
                    h.pair_epoch_sampled(0, capi.SGD_MINIBATCH, B, 1, seed, ep)
                curve.append(h.pair_evaluate_sampled(0, 1, seed, 1 << 32).loss)
            tr, te = h.pair_evaluate_sampled(0, 1, seed, 1 << 32), h.pair_evaluate_sampled(2, 1, seed, 1 << 32)
            h.close()
            finite = bool(np.all(np.isfinite(curve)))
            runs.append(dict(batch=B, rule=rule, rate=rate, train_loss=tr.loss, train_accuracy=tr.accuracy, heldout_loss=te.loss,
                             heldout_accuracy=te.accuracy, train_loss_curve=[float("%.4g" % x) if np.isfinite(x) else None for x in curve],
                             stable=finite and all(y <= x * 1.02 for x, y in zip(curve, curve[1:]))))
    head["runs"] = runs
    print(json.dumps(head), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stored", action="store_true")
    ap.add_argument("--sampled", action="store_true")
    ap.add_argument("--converge", action="store_true")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--items", type=int, default=5000)
    ap.add_argument("--top", type=int, default=30)
    ap.add_argument("--conv-epochs", type=int, default=10)
    a = ap.parse_args()
    every = not (a.stored or a.sampled or a.converge)
    if a.stored or every:
        stored(a)
    if a.sampled or every:
        sampled(a)
    if a.converge or every:
        converge(a)


if __name__ == "__main__":
    main()
