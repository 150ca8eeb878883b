"""Host time of fmx_create's table placement (fmx_place_info::seconds) at the bench's size (n = 1e8, k = 64: an arena of 26 chunks), for
comparing two builds of the library (FMX_LIB=<path of the other libfmx.so>), in a fresh process per round:

    python scripts/place_rate.py [--label NAME] [--out FILE]

  fresh  : after fmx_release_cached_memory(): chunks are taken, probed and classified (follows the pool, so it varies)
  cached : the next handle takes the destroyed one's arena over (no probing: pool = 0)
Prints one JSON line (and appends it to --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libfm_amd import capi  # noqa: E402


def placed(n, k):
    h = capi.Handle(n, k, device=0)
    pi = h.place_info()
    h.close()
    return {"method": pi.method, "chunks": pi.chunks, "per_class": [pi.per_class[0], pi.per_class[1]], "pool": pi.pool,
            "classes_seen": pi.classes_seen, "seconds": round(pi.seconds, 7)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="", help="copied into the line (which build this is)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("place_rate.py needs a HIP device")
    capi.release_cached_memory()
    fresh = placed(100_000_000, 64)
    cached = placed(100_000_000, 64)
    capi.release_cached_memory()
    line = json.dumps({"label": a.label, "fresh": fresh, "cached": cached})
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
