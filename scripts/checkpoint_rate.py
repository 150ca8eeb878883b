"""Binary checkpoints (fmx_checkpoint_save / _load) on the MI355X: what a save and a load cost, dense and sparse, against a plain
copy of the same bytes and against the text model file.

    python scripts/checkpoint_rate.py DIR [--what main,text] [--features 10000000] [--factors 64] [--reps 2] [--out FILE]

DIR is where the files go; they are deleted afterwards.  The record names the file system DIR is on (from /proc/mounts).
main : one handle, n = --features, k = --factors, an FTRL session after one Criteo-shaped epoch (2^19 rows of 39 entries, batch
       4 096).  Save and load, dense (FMX_CKPT_DENSE_STATE) and sparse, the fastest of --reps by fmx_ckpt_info::seconds, with the
       file's bytes, GB/s of file per second and device_seconds; the sparse file's size against the dense one.  The floor in the
       same run: the bytes of the PADDED tables (V, w and the four state tables) copied device -> pinned host and back in 16 MiB
       chunks through two pinned buffers, no packing, no checksum, no file -- what is left of a save's time is the packing, the
       checksum and the file.
text : fmx_save_model / fmx_load_model against a model-only checkpoint of the same handle at n = 200 000, k = --factors (1.3e7
       numbers at k = 64: the text path stays under a minute), and the ratio.
Prints one JSON line per measurement (and appends them to --out)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libfm_amd import capi  # noqa: E402

CHUNK = 16 << 20


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
    return {"bytes": int(i.bytes), "state_rows": int(i.state_rows), "seconds": i.seconds, "device_seconds": i.device_seconds,
            "GB_s": i.bytes / i.seconds / 1e9}


def best(fn, reps):
    runs = [info_dict(fn()) for _ in range(reps)]
    return min(runs, key=lambda r: r["seconds"]), [r["seconds"] for r in runs]


def copy_floor(total_bytes, reps):
    """total_bytes device -> pinned host and back in CHUNK pieces through two pinned buffers on one stream (torch: plain hipMemcpyAsync)"""
    import torch
    dev = torch.empty(total_bytes, dtype=torch.uint8, device="cuda")
    dev.zero_()
    pin = [torch.empty(CHUNK, dtype=torch.uint8).pin_memory() for _ in range(2)]
    ev = [torch.cuda.Event() for _ in range(2)]
    res = {}
    for name in ("to_host", "to_device"):
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, off in enumerate(range(0, total_bytes, CHUNK)):
                b, nb = i & 1, min(CHUNK, total_bytes - off)
                if i >= 2:
                    ev[b].synchronize()
                if name == "to_host":
                    pin[b][:nb].copy_(dev[off:off + nb], non_blocking=True)
                else:
                    dev[off:off + nb].copy_(pin[b][:nb], non_blocking=True)
                ev[b].record()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        res[name + "_s"] = min(times)
        res[name + "_GB_s"] = total_bytes / min(times) / 1e9
    del dev
    torch.cuda.empty_cache()
    return res


def main_run(d, n, k, reps, out):
    rows, nnz, lr = 1 << 19, 39, 0.01
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, lr, -1.0, 1.0)
    h.init_params(0.0, 0.05, 19)
    h.synth_rows(0, 123, 0, rows, nnz, capi.SYNTH_CRITEO)
    h.ftrl_begin(lr, 1.0, 0.2, 0.1, 0.0, 0.001)
    h.ftrl_epoch(0, 4096, 0)
    dense, sparse = os.path.join(d, "rate_dense.ckpt"), os.path.join(d, "rate_sparse.ckpt")
    rs = capi.load().fmx_compact_row_bytes(capi.COMPACT_BF16, k) // 2 - 2          # V's row stride in floats
    padded = n * 4 * (rs + 1) * 3                                                  # V + w and the z and n tables with their strides
    try:
        rec = {"what": "main", "features": n, "factors": k, "rows": rows, "nnz": nnz, "reps": reps, "dir_mount": filesystem_of(d)[0],
               "dir_fstype": filesystem_of(d)[1], "padded_table_bytes": padded, "chunk_bytes": CHUNK}
        for name, path, kw in (("dense", dense, dict(dense=True)), ("sparse", sparse, dict())):
            h.checkpoint_save(path, **kw)                                          # warm-up (the page cache of DIR, the pinned buffers' first touch)
            rec["save_" + name], rec["save_%s_all_s" % name] = best(lambda: h.checkpoint_save(path, **kw), reps)
            h.checkpoint_load(path)
            rec["load_" + name], rec["load_%s_all_s" % name] = best(lambda: h.checkpoint_load(path), reps)
        rec["sparse_over_dense_bytes"] = rec["save_sparse"]["bytes"] / rec["save_dense"]["bytes"]
        rec["floor"] = copy_floor(padded, reps)
        rec["save_dense_over_floor"] = rec["save_dense"]["seconds"] / rec["floor"]["to_host_s"]
        rec["load_dense_over_floor"] = rec["load_dense"]["seconds"] / rec["floor"]["to_device_s"]
        emit(rec, out)
    finally:
        for p in (dense, sparse, dense + ".tmp", sparse + ".tmp"):
            if os.path.exists(p):
                os.remove(p)
        h.ftrl_end()
        h.close()


def text_run(d, k, reps, out):
    n = 200_000
    h = capi.Handle(n, k, True, True, capi.TASK_CLASSIFICATION, 0.0, 0.0, 0.001, 0.01, -1.0, 1.0)
    h.init_params(0.0, 0.05, 19)
    text, binary = os.path.join(d, "rate_model.txt"), os.path.join(d, "rate_model.ckpt")
    try:
        def timed(fn, *a):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn(*a)
                ts.append(time.perf_counter() - t0)
            return min(ts)
        rec = {"what": "text", "features": n, "factors": k, "reps": reps, "dir_fstype": filesystem_of(d)[1],
               "text_save_s": timed(h.save_model, text), "text_load_s": timed(h.load_model, text), "text_bytes": os.path.getsize(text),
               "ckpt_save_s": timed(h.checkpoint_save, binary), "ckpt_load_s": timed(h.checkpoint_load, binary),
               "ckpt_bytes": os.path.getsize(binary)}
        rec["save_ratio"] = rec["text_save_s"] / rec["ckpt_save_s"]
        rec["load_ratio"] = rec["text_load_s"] / rec["ckpt_load_s"]
        emit(rec, out)
    finally:
        for p in (text, binary, binary + ".tmp"):
            if os.path.exists(p):
                os.remove(p)
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir", help="directory for the files (deleted afterwards)")
    ap.add_argument("--what", default="main,text")
    ap.add_argument("--features", type=int, default=10_000_000)
    ap.add_argument("--factors", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.load().fmx_device_count() == 0:
        raise SystemExit("checkpoint_rate.py needs a HIP device: nothing here is measured on a CPU")
    os.makedirs(a.dir, exist_ok=True)
    what = a.what.split(",")
    if "main" in what:
        main_run(a.dir, a.features, a.factors, a.reps, a.out)
    if "text" in what:
        text_run(a.dir, a.factors, a.reps, a.out)


if __name__ == "__main__":
    main()
