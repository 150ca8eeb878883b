"""Snapshot files (fmx_compact_save / _load, fmx_serve_open) on the MI355X: what a save and a load cost against the checkpoint of the
same model in the same run, and what a scoring process pays -- time to its first prediction and device memory once serving -- through
fmx_serve_open against today's route through the fp32 model.

    python scripts/snapshot_rate.py DIR [--features 10000000] [--factors 64] [--reps 5] [--starts 3] [--formats int8,bf16] [--out FILE]

DIR is where the files go; they are deleted afterwards.  The record names the file system DIR is on (from /proc/mounts).
One handle, n = --features, k = --factors, parameters from fmx_init_params; slot 0 holds 2^19 Criteo-shaped rows of 39 entries
(FMX_SYNTH_CRITEO), the keep slot of the pruned snapshots (FMX_PRUNE_DEAD | FMX_PRUNE_SEEN: the kept share is reported, as section 25
reports it).
files : a model-only checkpoint is saved and loaded first (section 24's figures, here and now); then, per format, dense and pruned:
        the snapshot is taken, saved (one warm-up, then --reps calls: the MEDIAN by fmx_snap_info::seconds is the figure, the
        fastest and the slowest stand beside it) and loaded back into the same handle (the same), with the file's bytes, GB/s,
        device_seconds, and the load's share of the checkpoint's load time (median over median).  A loaded
        snapshot must score slot 1 (4 096 further rows of the stream) bit for bit as the one that was saved, or no figure is printed.
start : per file, --starts rounds of two FRESH child processes, the two routes taking turns (median, fastest and slowest of each
        route are reported), each child timed by the parent's clock from the moment it is started to
        the moment it reports its first fmx_compact_predict result (interpreter start and imports included; the child's own phases
        are reported beside it): `serve` = fmx_serve_open of the snapshot file; `model` = fmx_create + fmx_checkpoint_load +
        [the keep slot's rows] + fmx_compact_begin[_pruned].  Both score the same 4 096 rows; their first predictions must agree bit
        for bit.  Each reports the device memory it holds once serving by the library's own count: fmx_info::bytes_params +
        the snapshot's bytes_compact (free-memory readings are not used: other tenants of a shared device disturb them).
Prints one JSON line per measurement (and appends them to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

T_IMPORT0 = time.time()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from libfm_amd import capi, compact  # noqa: E402

KEEP_ROWS, SCORE_ROWS, NNZ = 1 << 19, 4096, 39
CHILD_TIMEOUT = 600


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def filesystem_of(path):
    """(mount point, file system type) of the longest mount point that is a prefix of path"""
    path = os.path.realpath(path)
    best = ("", "?")
    try:
        with open("/proc/mounts") as f:
            for line in f:
                _, mnt, fstype = line.split()[:3]
                if (path == mnt or path.startswith(mnt.rstrip("/") + "/")) and len(mnt) > len(best[0]):
                    best = (mnt, fstype)
    except OSError:
        pass
    return best


def info_dict(i):
    return {"bytes": int(i.bytes), "seconds": i.seconds, "device_seconds": i.device_seconds, "GB_s": i.bytes / i.seconds / 1e9}


def best(fn, reps):
    """the run with the median whole-call time of `reps` calls (the lower middle one of an even count), and every call's time"""
    runs = sorted((info_dict(fn()) for _ in range(reps)), key=lambda r: r["seconds"])
    return runs[(len(runs) - 1) // 2], [r["seconds"] for r in runs]


def new_handle(n, k):
    return capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0)


def score_rows(h):
    h.synth_rows(1, 321, KEEP_ROWS, SCORE_ROWS, NNZ, capi.SYNTH_CRITEO)      # further rows of the keep slot's stream


def take(h, fmt, pruned):
    code = compact.FORMATS[fmt]
    if not pruned:
        return h.compact_begin(code), None
    return h.compact_begin_pruned(code, 0)


def files_run(d, n, k, reps, formats, out):
    """the parent's measurements; returns [(fmt, pruned, snapshot path)] and the checkpoint's path for the children"""
    h = new_handle(n, k)
    h.init_params(0.0, 0.05, 19)
    h.synth_rows(0, 123, 0, KEEP_ROWS, NNZ, capi.SYNTH_CRITEO)
    score_rows(h)
    ckpt = os.path.join(d, "rate_model.ckpt")
    base = {"features": n, "factors": k, "reps": reps, "dir_mount": filesystem_of(d)[0], "dir_fstype": filesystem_of(d)[1]}
    h.checkpoint_save(ckpt, model_only=True)                                   # warm-up (the page cache of DIR, the pinned buffers' first touch)
    rec = dict(base, what="checkpoint")
    rec["save"], rec["save_all_s"] = best(lambda: h.checkpoint_save(ckpt, model_only=True), reps)
    h.checkpoint_load(ckpt, model_only=True)
    rec["load"], rec["load_all_s"] = best(lambda: h.checkpoint_load(ckpt, model_only=True), reps)
    emit(rec, out)
    ckpt_load_s = rec["load"]["seconds"]
    made = []
    for fmt in formats:
        for pruned in (False, True):
            path = os.path.join(d, "rate_%s_%s.snap" % (fmt, "pruned" if pruned else "dense"))
            info, pinfo = take(h, fmt, pruned)
            want = h.compact_predict(1, SCORE_ROWS).tobytes()
            h.compact_save(path)
            rec = dict(base, what="files", format=fmt, pruned=pruned, bytes_compact=int(info.bytes_compact), bytes_params=int(info.bytes_params),
                       kept_share=(pinfo.kept / n) if pruned else 1.0)
            rec["save"], rec["save_all_s"] = best(lambda: h.compact_save(path), reps)
            h.compact_load(path)
            rec["load"], rec["load_all_s"] = best(lambda: h.compact_load(path), reps)
            if h.compact_predict(1, SCORE_ROWS).tobytes() != want:
                raise SystemExit("snapshot_rate: the loaded %s snapshot does not score as the saved one: no figure is reported" % fmt)
            rec["load_over_checkpoint_load"] = rec["load"]["seconds"] / ckpt_load_s
            rec["bytes_over_checkpoint_bytes"] = rec["load"]["bytes"] / os.path.getsize(ckpt)
            emit(rec, out)
            made.append((fmt, pruned, path))
    h.close()
    return made, ckpt


def child(route, n, k, fmt, pruned, snap, ckpt):
    """a fresh process: to its first compact_predict result by `route`; prints one JSON line"""
    t = {"imports_s": time.time() - T_IMPORT0}
    t0 = time.time()
    if route == "serve":
        h = capi.serve_open(snap)
        t["serve_open_s"] = time.time() - t0
        bytes_compact = int(h.snap_info.bytes_compact)
    else:
        h = new_handle(n, k)
        t["create_s"] = time.time() - t0
        t1 = time.time()
        h.checkpoint_load(ckpt, model_only=True)
        t["checkpoint_load_s"] = time.time() - t1
        t1 = time.time()
        if pruned:
            h.synth_rows(0, 123, 0, KEEP_ROWS, NNZ, capi.SYNTH_CRITEO)          # (the keep slot FMX_PRUNE_SEEN needs)
        info, _ = take(h, fmt, pruned)
        t["compact_begin_s"] = time.time() - t1
        bytes_compact = int(info.bytes_compact)
    t1 = time.time()
    score_rows(h)
    p = h.compact_predict(1, SCORE_ROWS)
    t["rows_and_predict_s"] = time.time() - t1
    done = time.time()
    print(json.dumps({"route": route, "first_result_at": done, "phases": t, "bytes_params": int(h.info().bytes_params),
                      "bytes_compact": bytes_compact, "predict_sum_bits": int(np.asarray(p).view(np.uint64).sum(dtype=np.uint64)),
                      "predict_nan": int(np.isnan(p).sum())}), flush=True)
    h.close()


def start_run(n, k, made, ckpt, starts, out):
    for fmt, pruned, snap in made:
        runs = {"serve": [], "model": []}
        for _ in range(starts):
            for route in ("serve", "model"):                     # (the routes take turns: what drifts on a shared host drifts for both)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", route, "--features", str(n), "--factors", str(k), "--formats", fmt,
                       "--pruned", "1" if pruned else "0", "--snap", snap, "--ckpt", ckpt]
                t0 = time.time()
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
                if r.returncode != 0:
                    raise SystemExit("snapshot_rate: the %s child failed: %s" % (route, r.stderr[-2000:]))
                c = json.loads(r.stdout.strip().splitlines()[-1])
                c["to_first_result_s"] = c.pop("first_result_at") - t0
                c["library_s"] = sum(v for key, v in c["phases"].items() if key not in ("imports_s", "rows_and_predict_s"))
                c["bytes_held"] = c["bytes_params"] + c["bytes_compact"]
                runs[route].append(c)
        if len({c["predict_sum_bits"] for cs in runs.values() for c in cs}) != 1:
            raise SystemExit("snapshot_rate: the two routes' first predictions differ: no figure is reported")
        res = {}
        for route, cs in runs.items():
            cs = sorted(cs, key=lambda c: c["to_first_result_s"])
            res[route] = dict(cs[(len(cs) - 1) // 2], to_first_result_all_s=[c["to_first_result_s"] for c in cs],
                              library_all_s=sorted(c["library_s"] for c in cs))
        emit({"what": "start", "features": n, "factors": k, "format": fmt, "pruned": pruned, "starts": starts, "serve": res["serve"],
              "model": res["model"], "serve_over_model_time": res["serve"]["to_first_result_s"] / res["model"]["to_first_result_s"],
              "serve_over_model_bytes": res["serve"]["bytes_held"] / res["model"]["bytes_held"]}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir", nargs="?", default="", help="directory for the files (deleted afterwards)")
    ap.add_argument("--features", type=int, default=10_000_000)
    ap.add_argument("--factors", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--starts", type=int, default=3)
    ap.add_argument("--formats", default="int8,bf16")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--pruned", default="0")
    ap.add_argument("--snap", default="")
    ap.add_argument("--ckpt", default="")
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("snapshot_rate.py needs a HIP device: nothing here is measured on a CPU")
    if a.child:
        return child(a.child, a.features, a.factors, a.formats, a.pruned == "1", a.snap, a.ckpt)
    if not a.dir:
        raise SystemExit("snapshot_rate.py needs DIR")
    os.makedirs(a.dir, exist_ok=True)
    made, ckpt = [], os.path.join(a.dir, "rate_model.ckpt")
    try:
        made, ckpt = files_run(a.dir, a.features, a.factors, a.reps, a.formats.split(","), a.out)
        start_run(a.features, a.factors, made, ckpt, a.starts, a.out)
    finally:
        for name in os.listdir(a.dir):                            # (also what a run that failed half way left behind)
            if name.startswith("rate_") and name.split(".tmp")[0].endswith((".snap", ".ckpt")):
                os.remove(os.path.join(a.dir, name))


if __name__ == "__main__":
    main()
