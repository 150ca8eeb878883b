"""One JSON line per route of the SGD epoch drivers (tests/schedule_routes.py): the sha256 of (w0, w, V) after the configuration's epochs, the
last epoch's batches / main_kernel_launches / deferred_features / status, and whether a second training in the same process gave the same
bytes.  Run it on two builds and compare the lines: a change to the host side of training (libfm_amd/csrc/fmx_sgd.hip, fmx_comm.hip) that
is meant to move no number must leave every line as it was (FMX_STAT_EVENT_SYNC aside where the bias lag is >= 2 at batches >= 32 768: that
bit says how the device scheduled the handle's two streams).
    python scripts/epoch_fingerprint.py [--only NAME ...] > profiles/epoch_fingerprint_<tag>.jsonl
    python scripts/epoch_fingerprint.py --compare BEFORE.jsonl AFTER.jsonl      (no device needed)
--compare: every line equal (FMX_STAT_WSTREAM aside: it says where the once-only features' linear weights were read from); where a build did not reproduce its own hash, that configuration is held to its counts and status only."""
import hashlib
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import schedule_routes as R          # noqa: E402

STAT_WSTREAM = 131072                # FMX_STAT_WSTREAM (include/fmx.h): set from a slot's second one-pass epoch on, FMX_WTRAIN=0 aside


def digest(params):
    w0, w, v = params
    hsh = hashlib.sha256(struct.pack("<d", float(w0)))
    hsh.update(w.tobytes())
    hsh.update(v.tobytes())
    return hsh.hexdigest()


def compare(before, after):
    a, b = ([json.loads(l) for l in open(f) if l.strip()] for f in (before, after))
    bad = len(a) != len(b)
    for x, y in zip(a, b):
        for z in (x, y):                              # (where the singles' linear weights were read from moves no number: not the route's)
            z["status"] = int(z["status"]) & ~STAT_WSTREAM
        if not (x.get("reproducible", True) and y.get("reproducible", True)):
            print("counts only (a build did not reproduce its own hash): %s" % x["config"])
            x, y = ({k: v for k, v in z.items() if k not in ("sha256", "reproducible")} for z in (x, y))
        if x != y:
            bad = True
            print("DIFFERENT %s\n  before %s\n  after  %s" % (x["config"], json.dumps(x), json.dumps(y)))
    print("%d configurations, %s" % (len(a), "DIFFERENCES" if bad else "all equal"))
    return 1 if bad else 0


def main():
    if "--compare" in sys.argv:
        i = sys.argv.index("--compare")
        raise SystemExit(compare(sys.argv[i + 1], sys.argv[i + 2]))
    from libfm_amd import capi
    only = sys.argv[sys.argv.index("--only") + 1:] if "--only" in sys.argv else None
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("epoch_fingerprint.py needs a HIP device")
    for c in R.CONFIGS:
        if only and c["name"] not in only:
            continue
        st, params = R.run(capi, c)
        line = {"config": c["name"], "batches": int(st.batches), "main_kernel_launches": int(st.main_kernel_launches),
                "deferred_features": int(st.deferred_features), "status": int(st.status)}
        if R.event_sync_masked(c):
            line["status"] &= ~R.STAT_EVENT_SYNC
        if c["deterministic"]:                      # (the asynchronous forms: counts only)
            line["sha256"] = digest(params)
            line["reproducible"] = digest(R.run(capi, c)[1]) == line["sha256"]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
