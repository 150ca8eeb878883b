"""Group checkpoints (fmx_group_checkpoint_save / _load) on the MI355X: what a save and a load cost over loopback shards, dense and
sparse, against the single-handle calls on the same state in the same run.

    python scripts/group_checkpoint_rate.py DIR [--shards 8] [--features 10000000] [--factors 64] [--reps 2] [--out FILE]

DIR is where the files go; they are deleted afterwards.  The record names the file system DIR is on (from /proc/mounts).
One group of --shards loopback shards on device 0 (hashed ownership), n = --features, k = --factors, an FTRL session after one
Criteo-shaped epoch (2^19 rows of 39 entries, one field per position, skewed ids; batch 4 096).  The start parameters reach the
group as a model-only checkpoint of an unsharded handle.  Save and load through the group, dense (FMX_CKPT_DENSE_STATE) and sparse,
the fastest of --reps by fmx_ckpt_info::seconds, with the file's bytes, GB of file per second and device_seconds.  Then the
yardstick: one unsharded handle loads the group's file -- the same state -- and its own fmx_checkpoint_save / _load are timed the
same way; its files are compared with the group's byte for byte.

Loopback shards share ONE device: they run one after the other what W GPUs would run side by side, and the copies between "devices"
are copies inside one HBM.  The figures say what the filtering, zero-filling and merging cost; they say nothing about xGMI.
Prints one JSON line (and appends it to --out, default profiles/group_checkpoint_rate.jsonl)."""
import argparse
import filecmp
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libfm_amd import capi  # noqa: E402
from scripts.checkpoint_rate import best, emit, filesystem_of  # noqa: E402

ROWS, NNZ, BATCH, LR = 1 << 19, 39, 4096, 0.01
FTRL = (LR, 1.0, 0.2, 0.1, 0.0, 0.001)                       # alpha, beta, l1_w, l1_v, l2_w, l2_v: checkpoint_rate.py's session


def criteo_shaped_rows(n, seed):
    """ROWS rows of NNZ one-hot entries: position f draws from its own range of ids (n / NNZ of them), skewed towards the low ones"""
    rng = np.random.default_rng(seed)
    per = n // NNZ
    ent = np.zeros(ROWS * NNZ, dtype=capi.ENTRY_DTYPE)
    u = rng.random((ROWS, NNZ))
    ent["id"] = (np.arange(NNZ, dtype=np.int64)[None, :] * per + np.minimum((u ** 4 * per).astype(np.int64), per - 1)).reshape(-1)
    ent["value"] = 1.0
    row_ptr = np.arange(ROWS + 1, dtype=np.uint64) * NNZ
    y = np.where(rng.random(ROWS) < 0.25, 1.0, -1.0).astype(np.float32)
    return ent, row_ptr, y


def timed(drv, dense_path, sparse_path, reps):
    rec = {}
    for name, path, kw in (("dense", dense_path, dict(dense=True)), ("sparse", sparse_path, dict())):
        drv.checkpoint_save(path, **kw)                          # warm-up (the page cache of DIR, the pinned buffers' first touch)
        rec["save_" + name], rec["save_%s_all_s" % name] = best(lambda: drv.checkpoint_save(path, **kw), reps)
        drv.checkpoint_load(path)
        rec["load_" + name], rec["load_%s_all_s" % name] = best(lambda: drv.checkpoint_load(path), reps)
    return rec


def run(d, shards, n, k, reps, out):
    new = lambda **kw: capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, LR, -1.0, 1.0, **kw)  # noqa: E731
    paths = {x: os.path.join(d, "group_rate_%s.ckpt" % x) for x in ("start", "g_dense", "g_sparse", "h_dense", "h_sparse")}
    h = new()
    hs, grp = [], None
    try:
        h.init_params(0.0, 0.05, 19)
        h.checkpoint_save(paths["start"], model_only=True)
        hs = [new(device=0, shard_rank=r, shard_world=shards, shard_hash=1) for r in range(shards)]
        grp = capi.Group(hs)
        grp.checkpoint_load(paths["start"])
        ent, row_ptr, y = criteo_shaped_rows(n, 123)
        grp.upload_rows(0, ent, row_ptr, y)
        grp.ftrl_begin(*FTRL)
        grp.ftrl_epoch(0, BATCH, 0)
        rec = {"what": "group", "shards": shards, "kind": "loopback, one device", "features": n, "factors": k, "rows": ROWS, "nnz": NNZ,
               "reps": reps, "dir_mount": filesystem_of(d)[0], "dir_fstype": filesystem_of(d)[1]}
        rec["group"] = timed(grp, paths["g_dense"], paths["g_sparse"], reps)
        h.checkpoint_load(paths["g_dense"])                      # the yardstick holds the group's state
        rec["handle"] = timed(h, paths["h_dense"], paths["h_sparse"], reps)
        rec["files_identical"] = bool(filecmp.cmp(paths["g_dense"], paths["h_dense"], shallow=False)
                                      and filecmp.cmp(paths["g_sparse"], paths["h_sparse"], shallow=False))
        for key in ("save_dense", "save_sparse", "load_dense", "load_sparse"):
            rec[key + "_group_over_handle"] = rec["group"][key]["seconds"] / rec["handle"][key]["seconds"]
        emit(rec, out)
    finally:
        for p in paths.values():
            for q in (p, p + ".tmp"):
                if os.path.exists(q):
                    os.remove(q)
        if grp is not None:
            grp.close()
        for m in hs:
            m.close()
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir", help="directory for the files (deleted afterwards)")
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--features", type=int, default=10_000_000)
    ap.add_argument("--factors", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_checkpoint_rate.jsonl"))
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("group_checkpoint_rate.py needs a HIP device: nothing here is measured on a CPU")
    os.makedirs(a.dir, exist_ok=True)
    run(a.dir, a.shards, a.features, a.factors, a.reps, a.out)


if __name__ == "__main__":
    main()
