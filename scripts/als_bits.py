"""The bits an ALS / MCMC session leaves behind: one SHA-256 per case over the raw bytes of get_params(), als_moments(), predict() on
the training slot and the sum_e_sqr, train_metric and levels of every sweep (never device_seconds) -- to be run on two builds of the
library (before and after a change to the session's set-up, its re-prediction or the sweep's host side in fmx_als.hip) and compared
line by line.  Not a test and no hash is an expected value: a compiler update may move them.

sha256 covers all of that, and two runs of ONE build already differ in it: w0, sum_e_sqr, train_metric and the moments are fp64 sums
that the kernels accumulate with atomic adds in the order the wavefronts arrive (k_als_sum_e, k_als_targets, k_group_moments), so
their last bits move from run to run (measured: a few 1e-16 relative, 1e-13 where a sum is close to zero).  sha256_stored covers what is stored as fp32 or counted
-- w, V, the predictions, the levels -- and is the same in every run of a build: that is the line-by-line comparison between two
builds; --dump keeps the fp64 sums for a numerical one.

    python scripts/als_bits.py [--cases plain,blocks,shards,single] [--out FILE] [--label NAME] [--dump FILE.npz]     (another build: FMX_LIB=<its libfmx.so>)

Every case starts from seeded values and runs three sweeps, once deterministic (ALS) and once with do_sample = 1 and a fixed seed:
  plain  : one handle, no blocks -- datagen.onehot_fields, 3 200 features in 16 fields, 2 000 rows, k 0, 1, 8, 17, 64, k 8 with k1 off
           and k 8 with three attribute groups; each with fused draws and with the split step forced for every level (capi.ALS_SPLIT_MIN,
           the switch of the tests' _split helper)
  blocks : one handle, kept blocks -- _random_relational(seed, n_rel) of tests/test_gpu_relations_sharded.py at its six EDGE rows
           (400 main rows, 1 - 3 blocks, empty and unmapped block rows, a block of one attribute), fused and split
  shards : the EDGE rows over loopback shards on device 0 with their own world and shard_hash; the plain k 8 case over 2, 3 and 5
           shards with both shard hashes (five shards over 16 fields: levels that are empty on some shard)
  single : a group of one around an unsharded handle, the plain k 8 case; its sha256_stored must equal the one-handle one of the
           same run (checked here)
Prints one JSON line per case (and appends them to --out)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from libfm_amd import capi  # noqa: E402

FORMS = (("fused", capi.ALS_SPLIT_NEVER), ("split", 1))
DUMP = []               # the fp64 sums of every printed line, in that order (--dump: by how much two runs differ in them)


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + a.tobytes())
    return h.hexdigest()


def start_values(n, k, seed):
    rng = np.random.default_rng(seed)
    return 0.25, rng.normal(0.0, 0.1, n), rng.normal(0.0, 0.1, (k, n)) if k > 0 else None


def session(x, rows, params, sample):
    """three sweeps from the start values on slot 0 of a handle or a group -> the hash of what they leave behind"""
    x.set_params(*params)
    x.als_begin(0)
    sums, levels = [], []
    for _ in range(3):
        st = x.als_sweep(1.5, 2.5, alpha=1.0, do_sample=sample, seed=1234)
        sums += [np.float64(st.sum_e_sqr), np.float64(st.train_metric)]
        levels.append(np.uint32(st.levels))
    sums += list(x.als_moments())
    x.als_end()
    w0, w, v = x.get_params()
    stored = [w, v, x.predict(0, rows)] + levels
    sums = [np.float64(w0)] + sums
    DUMP.append(np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in sums]))
    return digest(stored + sums), digest(stored)


def both(emit, tag, x, rows, params):
    shas = []
    for name, sample in (("als", False), ("mcmc", True)):
        sha, sha_stored = session(x, rows, params, sample)
        emit("%s %s" % (tag, name), sha, sha_stored)
        shas.append(sha_stored)
    return shas


def make(n, k, kw, groups, world=1, shard_hash=0, grouped=False):
    """(what to drive, its member handles): one handle, a group of one around it, or a group of loopback shards"""
    if world == 1:
        hs = [capi.Handle(n, k, device=0, **kw)]
    else:
        hs = [capi.Handle(n, k, device=0, shard_rank=r, shard_world=world, shard_hash=shard_hash, **kw) for r in range(world)]
    for h in hs:
        h.set_groups(groups)
    return (capi.Group(hs) if world > 1 or grouped else hs[0]), hs


def close(x, hs):
    if x is not hs[0]:
        x.close()
    for h in hs:
        h.close()


def plain_rows():
    import datagen
    return datagen.onehot_fields(3200, 16, 2000, seed=21, classification=True)


PLAIN_KW = dict(k0=True, k1=True, task=capi.TASK_CLASSIFICATION, reg0=0.0, regw=0.0, regv=0.0, min_target=-1.0, max_target=1.0)


def plain(emit, grouped=False):
    n = 3200
    ent, rp, y = plain_rows()
    three = (np.arange(n) % 3).astype(np.uint32)
    cases = [("k%d" % k, k, True, None) for k in ((8,) if grouped else (0, 1, 8, 17, 64))]
    if not grouped:
        cases += [("k8 k1 off", 8, False, None), ("k8 three groups", 8, True, three)]
    shas = {}
    for name, k, k1, groups in cases:
        for form, split in FORMS:
            capi.ALS_SPLIT_MIN = split
            x, hs = make(n, k, dict(PLAIN_KW, k1=k1), groups, grouped=grouped)
            try:
                x.upload_rows(0, ent, rp, y)
                shas[(name, form)] = both(emit, "%s %s %s" % ("group of one" if grouped else "plain", name, form), x, len(y), start_values(n, k, 5 + k))
            finally:
                close(x, hs)
    capi.ALS_SPLIT_MIN = 0
    return shas


def edge_rows():
    import test_gpu_relations_sharded as T
    for seed, world, n_rel, k, k1, G in T.EDGE:
        (ent, rp, y), rel, n = T._random_relational(seed, n_rel)
        groups = None
        if G > 1:
            groups = np.random.default_rng(seed + 100).integers(0, G, n).astype(np.uint32)
            groups[:G] = np.arange(G)
        kw = dict(k0=True, k1=k1, task=0, reg0=0.1, regw=1.0, regv=2.0, min_target=float(y.min()), max_target=float(y.max()))
        yield "edge seed %d (%d blocks, k %d, k1 %d, %d groups)" % (seed, n_rel, k, k1, G), (ent, rp, y), rel, n, k, kw, groups, world, seed % 2


def blocks(emit):
    for name, (ent, rp, y), rel, n, k, kw, groups, _, _ in edge_rows():
        for form, split in FORMS:
            capi.ALS_SPLIT_MIN = split
            x, hs = make(n, k, kw, groups)
            try:
                x.upload_block_rows(0, ent, rp, y, rel, keep=True)
                both(emit, "blocks %s %s" % (name, form), x, len(y), start_values(n, k, 40 + k))
            finally:
                close(x, hs)
    capi.ALS_SPLIT_MIN = 0


def shards(emit):
    for name, (ent, rp, y), rel, n, k, kw, groups, world, shard_hash in edge_rows():
        x, hs = make(n, k, kw, groups, world, shard_hash)
        try:
            x.upload_block_rows(0, ent, rp, y, rel, keep=True)
            both(emit, "shards %s world %d hash %d" % (name, world, shard_hash), x, len(y), start_values(n, k, 40 + k))
        finally:
            close(x, hs)
    ent, rp, y = plain_rows()
    for world in (2, 3, 5):
        for shard_hash in (0, 1):
            x, hs = make(3200, 8, PLAIN_KW, None, world, shard_hash)
            try:
                x.upload_rows(0, ent, rp, y)
                both(emit, "shards plain k8 world %d hash %d" % (world, shard_hash), x, len(y), start_values(3200, 8, 13))
            finally:
                close(x, hs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="plain,blocks,shards,single")
    ap.add_argument("--out", default="")
    ap.add_argument("--label", default="", help="copied into every line (which build this is)")
    ap.add_argument("--dump", default="", help="an .npz of the fp64 sums behind sha256, one array per printed line")
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("als_bits.py needs a HIP device")

    def emit(case, sha, sha_stored):
        line = json.dumps({"label": a.label, "case": case, "sha256": sha, "sha256_stored": sha_stored})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    cases = a.cases.split(",")
    one = plain(emit) if "plain" in cases or "single" in cases else {}
    if "blocks" in cases:
        blocks(emit)
    if "shards" in cases:
        shards(emit)
    same = True
    if "single" in cases:
        for key, shas in plain(emit, grouped=True).items():
            same = same and shas == one[key]
    if a.dump:
        np.savez(a.dump, *DUMP)
    if not same:
        raise SystemExit("a group of one differs from its handle")


if __name__ == "__main__":
    main()
