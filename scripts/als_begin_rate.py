"""Wall time of als_begin alone -- the level build (host, O(nnz)), the session's buffers and the first prediction -- for comparing
two builds of the library (FMX_LIB=<path of the other libfmx.so>).  A host clock around the call, which ends in a stream
synchronise, after one warm-up call that also builds X^T (kept by the slot, so the timed calls do not repeat it).

    python scripts/als_begin_rate.py [--reps 3] [--label NAME] [--out FILE]

  unsharded : the shape of bench.py --method als (n = 1e7, k = 64, 2^22 device-generated rows of 16 entries), one handle
  sharded   : 2^20 rows of 16 one-hot fields (n = 1.6e6, k = 8) over three loopback shards on device 0
Prints one JSON line per shape (and appends them to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from libfm_amd import capi  # noqa: E402


def timed_begins(x, reps):
    x.als_begin(0)
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        x.als_begin(0)
        out.append(round(time.perf_counter() - t0, 4))
    x.als_end()
    return out


def unsharded(reps):
    h = capi.Handle(10_000_000, 64, True, True, capi.TASK_REGRESSION, 0.0, 1.0, 10.0, 0.0, -1.0, 1.0, device=0)
    h.init_params(0.0, 0.01, 1)
    h.synth_rows(0, 123, 0, 1 << 22, 16)
    try:
        return timed_begins(h, reps)
    finally:
        h.close()


def sharded(reps):
    import datagen
    n, k, world = 1_600_000, 8, 3
    ent, rp, y = datagen.onehot_fields(n, 16, 1 << 20, seed=17, classification=False)
    hs = [capi.Handle(n, k, True, True, capi.TASK_REGRESSION, 0.0, 1.0, 10.0, 0.0, -1.0, 1.0, device=0, shard_rank=r, shard_world=world,
                      shard_hash=1) for r in range(world)]
    g = capi.Group(hs)
    try:
        for h in hs:
            h.init_params(0.0, 0.01, 1)
        g.upload_rows(0, ent, rp, y)
        return timed_begins(g, reps)
    finally:
        g.close()
        for h in hs:
            h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--label", default="", help="copied into every line (which build this is)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("als_begin_rate.py needs a HIP device")
    for shape, fn in (("unsharded", unsharded), ("sharded", sharded)):
        line = json.dumps({"label": a.label, "shape": shape, "als_begin_seconds": fn(a.reps)})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
