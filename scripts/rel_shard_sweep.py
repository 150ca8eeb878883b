"""Kept `-relation` blocks against the joined table on feature shards: memory, exchange and sweep time (a measurement, not a test).

    python scripts/rel_shard_sweep.py [--rows 2000000] [--users 100000] [--items 20000] [--implicit 50] [--vocab 2000] [--k 8] [--shards 1,2,4]

A seeded block-structured set where the join dominates: main rows = a context one-hot (16 values) mapped to a USER block (user
one-hot + `implicit` implicit-feedback items per user out of `vocab`, values 1/sqrt(implicit)) and an ITEM block (item one-hot + one of 20 genres).
For P loopback shards on device 0 x {keep, expand} one JSON line each:
  entries_per_shard     main (+ kept block) entries every shard holds after the upload (fmx_rows_info + the block rows it owns)
  device_bytes          device memory in use after the upload, over what was in use before the handles were made (tables included)
  main_levels / block_levels   dependency levels of the main columns (fmx_als_stats::levels) / of each kept block's attributes
  exchange_bytes_per_sweep     what the sweep all-reduces: 2 N doubles per (family, main level), 4 B doubles per (family, block level),
                        the re-prediction's (k + 1) (N + sum B) doubles; 0 on one shard (the pattern of fmx_als.hip, counted here)
  als_ms / mcmc_ms      wall time of one ALS sweep / one sampled sweep (after one warm-up sweep)
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_data(a, seed=1):
    from libfm_amd.capi import ENTRY_DTYPE
    rng = np.random.default_rng(seed)
    N, U, I, M = a.rows, a.users, a.items, a.implicit
    n_ctx, n_imp, n_genre = 16, a.vocab, 20
    main = np.zeros(N, dtype=ENTRY_DTYPE)
    main["id"] = rng.integers(0, n_ctx, N)
    main["value"] = 1.0
    main_rp = np.arange(N + 1, dtype=np.uint64)
    y = rng.integers(1, 6, N).astype(np.float32)
    # USER block: user one-hot (id u) then M distinct implicit items (ids U + item)
    ue = np.zeros(U * (1 + M), dtype=ENTRY_DTYPE).reshape(U, 1 + M)
    ue["id"][:, 0] = np.arange(U)
    ue["value"][:, 0] = 1.0
    # M distinct items per user: an arithmetic walk mod n_imp with a stride coprime to it (random start and stride)
    strides = np.array([s for s in range(1, 200, 2) if math.gcd(s, n_imp) == 1])
    walk = rng.integers(0, n_imp, (U, 1)) + rng.choice(strides, (U, 1)) * np.arange(M)[None, :]
    imp = np.sort(walk % n_imp, axis=1)
    ue["id"][:, 1:] = U + imp
    ue["value"][:, 1:] = 1.0 / math.sqrt(M)
    user = (ue.reshape(-1), np.arange(0, U * (1 + M) + 1, 1 + M, dtype=np.uint64), U + n_imp)
    ie = np.zeros(2 * I, dtype=ENTRY_DTYPE).reshape(I, 2)
    ie["id"][:, 0] = np.arange(I)
    ie["id"][:, 1] = I + rng.integers(0, n_genre, I)
    ie["value"] = 1.0
    item = (ie.reshape(-1), np.arange(0, 2 * I + 1, 2, dtype=np.uint64), I + n_genre)
    maps = [rng.integers(0, U, N).astype(np.uint32), rng.integers(0, I, N).astype(np.uint32)]
    rel, off = [], n_ctx
    for (be, bp, nf), mp in zip((user, item), maps):
        rel.append((be, bp, mp, off))
        off += nf
    return (main, main_rp, y), rel, off


def block_levels(be, bp, nf):
    """the dependency levels of a block's attributes over its rows (what fmx_group_als_begin computes, global id order)"""
    rows = np.repeat(np.arange(len(bp) - 1), np.diff(bp.astype(np.int64)))
    order = np.argsort(be["id"], kind="stable")
    t_rows = rows[order]
    cp = np.concatenate([[0], np.cumsum(np.bincount(be["id"], minlength=nf))])
    rowlevel = np.zeros(len(bp) - 1, dtype=np.int64)
    n_levels = 0
    for j in range(nf):
        r = t_rows[cp[j]:cp[j + 1]]
        if len(r) == 0:
            continue
        lv = int(rowlevel[r].max()) + 1
        rowlevel[r] = lv
        n_levels = max(n_levels, lv)
    return n_levels


def used_bytes(torch):
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info(0)
    return total - free


def run(P, keep, data, rel, n, k, blevels, torch):
    from libfm_amd import capi
    (ent, rp, y) = data
    N = len(y)
    capi.release_cached_memory()
    base = used_bytes(torch)
    lo, hi = float(y.min()), float(y.max())
    kw = dict(k0=True, k1=True, task=0, reg0=0.0, regw=1.0, regv=1.0, min_target=lo, max_target=hi, device=0)
    if P == 1:
        hs = [capi.Handle(n, k, **kw)]
        drv = hs[0]
    else:
        hs = [capi.Handle(n, k, shard_rank=r, shard_world=P, shard_hash=1, **kw) for r in range(P)]
        drv = capi.Group(hs)
    rng = np.random.default_rng(3)
    v = 0.05 * rng.standard_normal((k, n))
    drv.set_params(0.0, np.zeros(n), v)
    t0 = time.perf_counter()
    drv.upload_block_rows(0, ent, rp, y, rel, keep=keep)
    upload_s = time.perf_counter() - t0
    dev = used_bytes(torch) - base
    per_shard = []
    for r, h in enumerate(hs):
        nr, nz = C.c_uint32(0), C.c_uint64(0)
        h._chk(h.lib.fmx_rows_info(h.h, 0, C.byref(nr), C.byref(nz)))
        e = int(nz.value)
        if keep:                                          # + the block entries this shard owns
            for be, bp, mp, off in rel:
                if P == 1:
                    e += len(be)
                else:
                    own, _ = capi.shard_place(n, P, 1, be["id"].astype(np.uint64) + off)
                    e += int((own == r).sum())
        per_shard.append(e)
    t0 = time.perf_counter()
    drv.als_begin(0)
    begin_s = time.perf_counter() - t0
    st = drv.als_sweep(1.0, 1.0)                          # warm-up
    main_levels = int(st.levels)
    t0 = time.perf_counter()
    drv.als_sweep(1.0, 1.0)
    als_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    drv.als_sweep(1.0, 1.0, do_sample=True, seed=7)
    mcmc_ms = 1e3 * (time.perf_counter() - t0)
    drv.als_end()
    B = [len(bp) - 1 for _, bp, _, _ in rel]
    xb = 0
    if P > 1:
        xb = 8 * ((1 + k) * main_levels * 2 * N + (k + 1) * N)
        if keep:
            xb += 8 * sum((1 + k) * L * 4 * b + (k + 1) * b for L, b in zip(blevels, B))
    out = {"shards": P, "blocks": "keep" if keep else "expand", "main_rows": N, "k": k,
           "entries_per_shard": per_shard, "device_bytes": int(dev), "main_levels": main_levels,
           "block_levels": blevels if keep else None, "exchange_bytes_per_sweep": xb,
           "upload_s": round(upload_s, 3), "begin_s": round(begin_s, 3), "als_ms": round(als_ms, 2), "mcmc_ms": round(mcmc_ms, 2)}
    if P > 1:
        drv.close()
    for h in hs:
        h.close()
    capi.release_cached_memory()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000000)
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--implicit", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=2000)      # implicit items: they conflict almost pairwise, ~ one block level each
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--shards", default="1,2,4")
    a = ap.parse_args()
    import torch
    data, rel, n = make_data(a)
    blevels = [block_levels(be, bp, int(be["id"].max()) + 1) for be, bp, _, _ in rel]
    for P in [int(x) for x in a.shards.split(",")]:
        for keep in (True, False):
            print(json.dumps(run(P, keep, data, rel, n, a.k, blevels, torch)), flush=True)


if __name__ == "__main__":
    main()
