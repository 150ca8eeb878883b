"""GPU: the snapshot file and the serve-only handle (fmx_compact_save / _load, fmx_serve_open: fmx_snap.hip, k_snap_rows,
k_snap_dir_check; include/fmx.h) against libfm_amd/compact.py's restatement of the file (pinned on the CPU in
tests/test_snapshot_cpu.py).

Shapes: n = 1000 features, 200 rows of 8 entries, k in {0, 8, 40, 64, 100} (no factors; a row narrower than, equal to and wider than
a wavefront's 64 lanes; k = 40 and 100 with row padding on the device: rs = 48 and 112), both formats, dense / dead / seen snapshots of
a model with planted dead rows and one row with a NaN factor.  n = 1000 is no multiple of 32, so the directory's last word is partial.

Comparisons are of bytes and bits, with one exception the issue names: a file the device never wrote is scored against
CompactModel.predict under the tolerance tests/test_gpu_compact.py and tests/test_gpu_compact_int8.py use for that comparison
(RTOL, ATOL, imported from there)."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from libfm_amd import compact
from test_gpu_compact import ATOL, RTOL, handle, make_params, write_libfm
from test_gpu_eval_ex import INT_FIELDS
from test_snapshot_cpu import bad_directories

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ROWS, NNZ = 1000, 200, 8
KS = (0, 8, 40, 64, 100)
FORMATS = ("bf16", "int8")
PRUNES = (None, "dead", "seen")
E_ARG, E_STATE = -1, -3
CHILD_TIMEOUT = 240                                              # seconds a child process may take (it imports torch and opens the device)


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


def rows(seed=5, n_ids=800):
    """ROWS rows of NNZ entries over the ids below n_ids (so that `seen` drops live features: the ids from n_ids on), targets +-1"""
    from libfm_amd import capi
    rng = np.random.default_rng(seed)
    ent = np.zeros(ROWS * NNZ, dtype=capi.ENTRY_DTYPE)
    ent["id"] = np.concatenate([rng.choice(n_ids, size=NNZ, replace=False) for _ in range(ROWS)])
    ent["id"][0] = 11                                             # (planted()'s NaN row is seen: row 0 scores NaN from every snapshot)
    ent["value"] = np.round(rng.normal(0.0, 1.0, ROWS * NNZ), 3)
    ent["value"][ent["value"] == 0] = 0.5
    rp = (np.arange(ROWS + 1) * NNZ).astype(np.uint64)
    y = np.where(rng.random(ROWS) < 0.4, 1.0, -1.0).astype(np.float32)
    return ent, rp, y


def planted(k, seed=1):
    """w0, w, v of test_gpu_compact's make_params with every seventh feature dead and, with k > 0, one NaN factor in feature 11"""
    w0, w, v = make_params(N, k, seed + k)
    w[3::7] = 0.0
    v[:, 3::7] = 0.0
    if k > 0:
        v[k // 2, 11] = np.nan
    return w0, w, v


def take(capi, h, fmt, prune):
    code = compact.FORMATS[fmt]
    if prune is None:
        return h.compact_begin(code), None
    return h.compact_begin_pruned(code, 0 if prune == "seen" else None)


def restate(path, h, ent, fmt, prune, task=1):
    """write_snapshot of the fp32 parameters the handle holds; returns (w0, w, v, keep)"""
    w0, w, v = h.get_params()
    v = np.asarray(v).reshape(h.k, N)
    seen = compact.seen_mask(N, ent["id"]) if prune == "seen" else None
    keep = compact.prune_mask(w, v, True, seen) if prune else None
    compact.write_snapshot(path, w0, w, v, True, True, task, -1.0, 1.0, fmt, keep=keep, seen=seen)
    return w0, w, v, keep


def read(path):
    with open(path, "rb") as f:
        return f.read()


def first_difference(a, b):
    if len(a) != len(b):
        return "lengths %d and %d" % (len(a), len(b))
    at = next(i for i in range(len(a)) if a[i] != b[i])
    return "first difference at byte %d: %s / %s" % (at, a[at:at + 8].hex(), b[at:at + 8].hex())


def serve_results(capi, h, cand_slot=1):
    """everything the serving calls return from the handle's snapshot, as bytes / exact values"""
    ids = np.arange(N, dtype=np.uint32)
    ev, ex = h.compact_evaluate(0), h.compact_evaluate_ex(0)
    excl_ptr = (np.arange(ROWS + 1) * 2).astype(np.uint64)       # every query excludes two candidates
    excl_idx = np.stack([np.arange(ROWS) % 50, (np.arange(ROWS) * 7 + 1) % 50], axis=1).astype(np.uint32)
    excl_idx[:, 1] = np.where(excl_idx[:, 1] == excl_idx[:, 0], (excl_idx[:, 0] + 1) % 50, excl_idx[:, 1])
    idx, score = h.compact_topk(0, cand_slot, 5, exclude=(excl_ptr, np.sort(excl_idx, axis=1).reshape(-1)))
    cw, cv = h.compact_rows(ids)
    out = {"predict": h.compact_predict(0, ROWS).tobytes(),
           "evaluate": struct.pack("<dddQ", ev.rmse, ev.mae, ev.accuracy, ev.rows),
           "evaluate_ex": struct.pack("<6Q5d", *[getattr(ex, f) for f in INT_FIELDS], ex.auc, ex.logloss, ex.rmse, ex.mae, ex.accuracy),
           "topk": idx.tobytes() + score.tobytes(), "rows": np.asarray(cw).tobytes() + np.asarray(cv).tobytes()}
    return out


def upload(h, ent, rp, y):
    h.upload_rows(0, ent, rp, y)
    h.upload_rows(1, ent[:50 * NNZ], rp[:51], y[:50])            # 50 candidate rows


CASES = [(fmt, k, prune) for fmt in FORMATS for k in KS for prune in PRUNES]
IDS = ["%s-k%d-%s" % (fmt, k, prune or "dense") for fmt, k, prune in CASES]


@pytest.mark.parametrize("fmt, k, prune", CASES, ids=IDS)
def test_file_is_the_restatements_and_serves_bit_for_bit(capi, tmp_path, fmt, k, prune):
    """byte parity: compact_save from the device == write_snapshot of the parameters get_params returns.  Bit parity of serving: a
    serve-only handle opened from the file, in the same process, returns what the original handle's snapshot returns from every
    serving call, and saves the file again byte for byte."""
    ent, rp, y = rows()
    dev, cpu, again = (str(tmp_path / x) for x in ("dev.snap", "cpu.snap", "again.snap"))
    h = handle(capi, N, k, True, 1, planted(k))
    s = None
    try:
        upload(h, ent, rp, y)
        info, pinfo = take(capi, h, fmt, prune)
        si = h.compact_save(dev)
        assert not os.path.exists(dev + ".tmp")
        _, _, _, keep = restate(cpu, h, ent, fmt, prune)
        a, b = read(dev), read(cpu)
        hd = compact.snapshot_header(dev)
        print("%s k %d %s: %d bytes, rows %d, sum_sq_err %.17g (restatement %.17g)" % (
            fmt, k, prune, len(a), hd["rows"], hd["sum_sq_err"], compact.snapshot_header(cpu)["sum_sq_err"]))
        assert a == b, first_difference(a, b)
        rows_kept = int(keep.sum()) if prune else N
        assert (si.bytes, si.rows, si.pruned, si.format, si.task, si.min_target, si.max_target) == (
            len(a), rows_kept, int(prune is not None), compact.FORMATS[fmt], 1, -1.0, 1.0)
        assert (si.nonfinite, si.max_abs_err) == (info.nonfinite, info.max_abs_err)
        assert struct.pack("<d", si.sum_sq_err) == struct.pack("<d", info.sum_sq_err)
        assert si.bytes_compact == info.bytes_compact
        if prune:
            assert (si.kept, si.dropped_dead, si.dropped_unseen) == (pinfo.kept, pinfo.dropped_dead, pinfo.dropped_unseen)
            assert pinfo.dropped_dead > 0 and (pinfo.dropped_unseen > 0) == (prune == "seen")
        if k > 0:
            assert si.nonfinite > 0                               # (feature 11, the NaN row, is live and row 0 names it: every snapshot holds it)
        want = serve_results(capi, h)
        # the second handle: the file alone
        s = capi.serve_open(dev)
        assert s.info().bytes_params == 0 and s.snap_info.bytes_compact == info.bytes_compact
        upload(s, ent, rp, y)
        got = serve_results(capi, s)
        for key in want:
            assert got[key] == want[key], key
        if prune:
            ids = np.arange(N, dtype=np.uint32)
            assert np.array_equal(s.compact_slot_of(ids), h.compact_slot_of(ids))
            assert np.array_equal(s.compact_slot_of(ids), compact.slot_of(compact.directory(keep), ids))
        s2 = s.compact_save(again)
        assert read(again) == a
        assert (s2.bytes, s2.rows, s2.nonfinite) == (si.bytes, si.rows, si.nonfinite)
        pi = s.place_info()
        assert (pi.method, pi.chunks, pi.seconds) == (0, 0, 0.0)
        s.synchronize()
    finally:
        if s is not None:
            s.close()
        h.close()


@pytest.mark.parametrize("fmt, prune", [("bf16", None), ("bf16", "dead"), ("int8", None), ("int8", "dead")])
def test_byte_parity_beyond_one_round_of_the_quantisers_grid(capi, tmp_path, fmt, prune):
    """n = 70 001, k = 64: more features than the 8 192 blocks of k_compact_quant (one feature per wavefront at this width: 32 768 a
    round) and of k_compact_quant8 (two per wavefront: 65 536 a round) hold at once, so every lane adds the squared errors of more
    than one feature and k_compact_final's lanes fold 128 blocks each -- the loop over rounds of compact.device_sum_sq is held
    against the device's sum_sq_err bit for bit, inside the byte parity of the whole file"""
    n, k = 70001, 64
    rng = np.random.default_rng(17)
    w, v = rng.normal(0.0, 0.3, n), rng.normal(0.0, 0.04, (k, n))
    w[5::11] = 0.0
    v[:, 5::11] = 0.0
    v[3, 40000] = np.inf
    dev, cpu = str(tmp_path / "dev.snap"), str(tmp_path / "cpu.snap")
    h = capi.Handle(n, k, True, True, 1, 0.0, 0.001, 0.002, 0.01, -1.0, 1.0)
    try:
        h.set_params(0.25, w, v)
        info, _ = take(capi, h, fmt, prune)
        h.compact_save(dev)
        w0, wd, vd = h.get_params()
        vd = np.asarray(vd).reshape(k, n)
        keep = compact.prune_mask(wd, vd, True) if prune else None
        compact.write_snapshot(cpu, w0, wd, vd, True, True, 1, -1.0, 1.0, fmt, keep=keep)
        a, b = read(dev), read(cpu)
        _, plain, _ = compact.quant_report(vd if keep is None else vd[:, keep], fmt)
        print("%s %s: sum_sq_err device %.17g, restated in its order %.17g, quant_report's order %.17g" % (
            fmt, prune, info.sum_sq_err, compact.snapshot_header(cpu)["sum_sq_err"], plain))
        assert a == b, first_difference(a, b)
        assert struct.pack("<d", compact.snapshot_header(cpu)["sum_sq_err"]) == struct.pack("<d", info.sum_sq_err)
    finally:
        h.close()


@pytest.mark.parametrize("fmt, k, prune", [(f, k, p) for f in FORMATS for k in KS for p in (None, "seen")],
                         ids=["%s-k%d-%s" % (f, k, p or "dense") for f in FORMATS for k in KS for p in (None, "seen")])
def test_a_file_the_device_never_wrote(capi, tmp_path, fmt, k, prune):
    """write_snapshot -> serve_open -> compact_predict against CompactModel.predict of the file read back, under the tolerance of
    tests/test_gpu_compact.py / test_gpu_compact_int8.py for that comparison; a regression file, so the task and the target range are
    the file's, not a handle's"""
    ent, rp, y = rows(seed=9)
    w0, w, v = make_params(N, k, 40 + k)                          # (no NaN row: the comparison is of numbers)
    w[3::7] = 0.0
    v[:, 3::7] = 0.0
    w32, v32 = w.astype(np.float32), v.astype(np.float32)
    seen = compact.seen_mask(N, ent["id"]) if prune else None
    keep = compact.prune_mask(w32, v32, True, seen) if prune else None
    path = str(tmp_path / "cpu.snap")
    compact.write_snapshot(path, float(np.float32(w0)), w32, v32, True, True, 0, -0.5, 0.75, fmt, keep=keep, seen=seen)
    model, hd = compact.read_snapshot(path)
    s = capi.serve_open(path)
    try:
        assert (s.snap_info.task, s.snap_info.min_target, s.snap_info.max_target) == (0, -0.5, 0.75) and s.n == N and s.k == k
        s.upload_rows(0, ent, rp, y)
        got, want = s.compact_predict(0, ROWS), model.predict(ent, rp)
        print("%s k %d %s: |serve - restatement| max %.3g" % (fmt, k, prune, np.abs(got - want).max()))
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
        ev = s.compact_evaluate(0)                               # regression: clamped to the FILE's target range
        clamped = np.minimum(0.75, np.maximum(-0.5, got))
        assert abs(ev.rmse - np.sqrt(np.mean((clamped - y) ** 2))) <= 1e-5
        cw, cv = s.compact_rows(np.arange(N, dtype=np.uint32))
        assert np.array_equal(cw, model.w) and np.array_equal(np.asarray(cv).reshape(k, N), model.v)
    finally:
        s.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_load_into_an_ordinary_handle(capi, tmp_path, fmt):
    """compact_load leaves the model bit-identical, an epoch of training does not change what the loaded snapshot scores, and a
    geometry mismatch is FMX_E_ARG naming the field with the earlier snapshot still scoring as before"""
    k = 40
    ent, rp, y = rows()
    path, other = str(tmp_path / "a.snap"), str(tmp_path / "other.snap")
    h = handle(capi, N, k, True, 1, planted(k))
    g = handle(capi, N, k, True, 1, make_params(N, k, 77))        # another model: what it loads is not what it would take itself
    try:
        upload(h, ent, rp, y)
        upload(g, ent, rp, y)
        take(capi, h, fmt, "dead")
        h.compact_save(path)
        want = serve_results(capi, h)
        before = [np.asarray(x).tobytes() for x in g.get_params()[1:]] + [struct.pack("<d", g.get_params()[0])]
        li = g.compact_load(path)
        assert li.pruned == 1 and li.bytes == os.path.getsize(path)
        assert [np.asarray(x).tobytes() for x in g.get_params()[1:]] + [struct.pack("<d", g.get_params()[0])] == before
        got = serve_results(capi, g)
        for key in want:
            assert got[key] == want[key], key
        g.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, 64, 16)
        assert np.asarray(g.get_params()[2]).tobytes() != before[1]
        assert serve_results(capi, g)["predict"] == want["predict"]
        # geometry mismatches: each field, both values in the message
        for kw, text in ((dict(n=N + 1), "num_attribute is 1001 in the file and 1000 on the handle"),
                         (dict(k=k + 1), "num_factor is 41 in the file and 40 on the handle"),
                         (dict(k1=False), "k1 is 0 in the file and 1 on the handle")):
            n2, k2, k1 = kw.get("n", N), kw.get("k", k), kw.get("k1", True)
            rng = np.random.default_rng(3)
            compact.write_snapshot(other, 0.5, rng.normal(size=n2), rng.normal(size=(k2, n2)), True, k1, 1, -1.0, 1.0, fmt)
            with pytest.raises(capi.FmxError, match=text) as e:
                g.compact_load(other)
            assert e.value.code == E_ARG
            assert serve_results(capi, g)["predict"] == want["predict"]
        # task / min / max are not compared: the handle's own hold
        w0, w, v = h.get_params()
        compact.write_snapshot(other, w0, w, np.asarray(v).reshape(k, N), True, True, 0, -9.0, 9.0, fmt)
        g.compact_load(other)
        assert g.compact_evaluate(0).rows == ROWS
    finally:
        h.close()
        g.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_corrupt_files_are_refused_not_scored(capi, tmp_path, fmt):
    """a truncated file, a flipped byte in the rows, a directory with one base off by one and one with a bit beyond n -- the last two
    behind RECOMPUTED checksums, so only the device's validation can refuse them.  Into an ordinary handle: FMX_E_ARG and the earlier
    snapshot scores as before.  Through serve_open: FMX_E_ARG and no handle."""
    k = 8
    ent, rp, y = rows()
    good, bad = str(tmp_path / "good.snap"), str(tmp_path / "bad.snap")
    h = handle(capi, N, k, True, 1, planted(k))
    try:
        upload(h, ent, rp, y)
        take(capi, h, fmt, "seen")
        h.compact_save(good)
        data, hd = read(good), compact.snapshot_header(good)
        take(capi, h, fmt, None)                                 # the handle's earlier snapshot: a dense one
        want = serve_results(capi, h)["predict"]
        rows_kind = compact.SNAP_ROWS if fmt == "int8" else compact.SNAP_V
        off, nbytes = [(s[1], s[2]) for s in hd["sections"] if s[0] == rows_kind][0]
        flipped = bytearray(data)
        flipped[off + nbytes // 2] ^= 0x04
        by_base, by_bit = bad_directories(data, hd)
        cases = [("truncated", data[:-16], "truncated"),
                 ("flipped byte", bytes(flipped), "checksum mismatch in section '%s'" % compact.SNAP_SECTION_NAMES[rows_kind]),
                 ("base off by one", bytes(by_base), "directory that is not consistent"),
                 ("bit beyond n", bytes(by_bit), "directory that is not consistent")]
        lib = capi.load()
        for name, blob, text in cases:
            with open(bad, "wb") as f:
                f.write(blob)
            with pytest.raises(capi.FmxError, match=text) as e:
                h.compact_load(bad)
            assert e.value.code == E_ARG, name
            assert h.compact_predict(0, ROWS).tobytes() == want, name
            out = capi.H()
            assert lib.fmx_serve_open(bad.encode(), -1, C.byref(out), None) == E_ARG and not out, name
            assert text.encode() in lib.fmx_last_error(None), name
            with pytest.raises(capi.FmxError, match=text):
                capi.serve_open(bad)
        h.compact_load(good)                                     # and the good file still loads
        assert h.compact_slot_of(np.arange(4, dtype=np.uint32)).shape == (4,)
    finally:
        h.close()


STRIDE_CHILD = """
import sys, numpy as np
from libfm_amd import capi
z = np.load(sys.argv[1])
h = capi.Handle(int(z["n"]), int(z["k"]), True, True, 1, 0.0, 0.001, 0.002, 0.01, -1.0, 1.0)
h.set_params(float(z["w0"]), z["w"], z["v"])
assert h.compact_begin(capi.COMPACT_BF16).bytes_compact == int(z["n"]) * (2 * int(sys.argv[3]) + 4)
h.compact_save(sys.argv[2])
h.close()
"""


def test_the_file_does_not_depend_on_the_row_stride(capi, tmp_path):
    """a bf16 file at k = 40 written by a child process run with FMX_ROW_STRIDE_KP=1 (rows of 64 on the device, not 48) equals the
    file written here byte for byte, and loads in this process"""
    k = 40
    w0, w, v = planted(k)
    npz, theirs, ours = str(tmp_path / "m.npz"), str(tmp_path / "theirs.snap"), str(tmp_path / "ours.snap")
    np.savez(npz, n=N, k=k, w0=w0, w=w, v=v)
    env = dict(os.environ, FMX_ROW_STRIDE_KP="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", STRIDE_CHILD, npz, theirs, "64"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, r.stderr[-2000:]
    h = handle(capi, N, k, True, 1, (w0, w, v))
    try:
        assert h.compact_begin(capi.COMPACT_BF16).bytes_compact == N * (2 * 48 + 4)
        h.compact_save(ours)
        a, b = read(theirs), read(ours)
        assert a == b, first_difference(a, b)
        cw, cv = h.compact_rows(np.arange(N, dtype=np.uint32))
        h.compact_end()
        h.compact_load(theirs)
        cw2, cv2 = h.compact_rows(np.arange(N, dtype=np.uint32))
        assert np.asarray(cw).tobytes() == np.asarray(cw2).tobytes() and np.asarray(cv).tobytes() == np.asarray(cv2).tobytes()
    finally:
        h.close()


def test_the_serve_only_handle_refuses_the_model(capi, tmp_path):
    """bytes_params = 0; every call of a representative set that reads or writes the model, each with valid arguments, returns
    FMX_E_STATE naming a serve-only handle, and compact_predict returns the same bits after each; compact_end then compact_load serves
    again"""
    k = 8
    ent, rp, y = rows()
    path, ckpt, mdl = str(tmp_path / "a.snap"), str(tmp_path / "a.ckpt"), str(tmp_path / "a.model")
    h = handle(capi, N, k, True, 1, planted(k))
    s = None
    try:
        upload(h, ent, rp, y)
        take(capi, h, "int8", "seen")
        h.compact_save(path)
        h.checkpoint_save(ckpt)
        h.save_model(mdl)
        w0, w, v = h.get_params()
        s = capi.serve_open(path)
        assert s.info().bytes_params == 0 and s.info().n_local == N
        upload(s, ent, rp, y)
        want = s.compact_predict(0, ROWS).tobytes()
        ids = np.arange(5, dtype=np.uint32)
        calls = [("set_params", lambda: s.set_params(w0, w, v)), ("get_params", lambda: s.get_params()),
                 ("get_param_rows", lambda: s.get_param_rows(ids)), ("init_params", lambda: s.init_params(0.0, 0.1, 1)),
                 ("load_model", lambda: s.load_model(mdl)), ("predict", lambda: s.predict(0, ROWS)), ("evaluate", lambda: s.evaluate(0)),
                 ("evaluate_ex", lambda: s.evaluate_ex(0)), ("topk", lambda: s.topk(0, 1, 5)),
                 ("sgd_epoch", lambda: s.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_SEGMENTED, 64, 16)),
                 ("adapt_begin", lambda: s.adapt_begin()), ("ftrl_begin", lambda: s.ftrl_begin()), ("als_begin", lambda: s.als_begin(0)),
                 ("sgda_begin", lambda: s.sgda_begin()), ("checkpoint_save", lambda: s.checkpoint_save(ckpt + ".2")),
                 ("checkpoint_load", lambda: s.checkpoint_load(ckpt)), ("param_sparsity", lambda: s.param_sparsity()),
                 ("compact_begin", lambda: s.compact_begin(capi.COMPACT_INT8)),
                 ("compact_begin_pruned", lambda: s.compact_begin_pruned(capi.COMPACT_INT8, 0)),
                 ("group creation", lambda: capi.Group([s]))]
        for name, call in calls:
            with pytest.raises(capi.FmxError, match="a serve-only handle holds no model") as e:
                call()
            assert e.value.code == E_STATE, name
            assert s.compact_predict(0, ROWS).tobytes() == want, name
        assert not os.path.exists(ckpt + ".2")
        s.compact_end()
        with pytest.raises(capi.FmxError) as e:
            s.compact_predict(0, ROWS)
        assert e.value.code == E_STATE
        s.compact_load(path)
        assert s.compact_predict(0, ROWS).tobytes() == want
        # the row side works: rows come back as they went up, and a slot can be freed and taken again
        ent2, rp2, y2 = s.download_rows(0)
        assert ent2.tobytes() == ent.tobytes() and np.array_equal(rp2, rp) and np.array_equal(y2, y)
        s.free_rows(0)
        s.upload_rows(0, ent, rp, y)
        assert s.compact_predict(0, ROWS).tobytes() == want
    finally:
        if s is not None:
            s.close()
        h.close()


def test_learner_view_and_load_snapshot(capi, tmp_path):
    """CompactView.save and learner.load_snapshot: the view over the file predicts, evaluates, recommends and returns rows as the view
    of the learner that took it"""
    from libfm_amd import learner as L
    from test_gpu_compact import tiny_regression, trained_learner
    tr, te = (L.Data(*tiny_regression(s)) for s in (1, 2))
    l = trained_learner(L, tr, te, 8, 3)
    path = str(tmp_path / "l.snap")
    try:
        view = l.compact("int8", prune="dead")
        si = view.save(path)
        assert si.pruned == 1 and si.bytes == os.path.getsize(path)
        served = L.load_snapshot(path)
        try:
            assert (served.format, served.prune) == ("int8", "dead")
            assert served.predict(te).tobytes() == view.predict(te).tobytes()
            assert served.evaluate(te) == view.evaluate(te)
            ids = np.arange(10, dtype=np.uint32)
            assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(served.rows(ids), view.rows(ids)))
            i1, s1 = served.recommend(te, tr, 3)
            i2, s2 = view.recommend(te, tr, 3)
            assert i1.tobytes() == i2.tobytes() and s1.tobytes() == s2.tobytes()
        finally:
            served.close()
        view.close()
    finally:
        l.close()


def test_cli_save_then_serve(capi, tmp_path):
    """one child trains and writes -serve int8 -serve_prune seen -save_snapshot F -out A; a second child runs -method serve
    -load_snapshot F -test T -out B and creates no model: A and B are the same file"""
    from test_gpu_compact import tiny_regression
    trf, tef = str(tmp_path / "train.libfm"), str(tmp_path / "test.libfm")
    write_libfm(trf, *tiny_regression(1))
    write_libfm(tef, *tiny_regression(2))
    snap, a, b = (str(tmp_path / x) for x in ("f.snap", "a.out", "b.out"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cli = [sys.executable, "-m", "libfm_amd.cli"]
    r1 = subprocess.run(cli + ["-task", "r", "-train", trf, "-test", tef, "-dim", "1,1,8", "-iter", "3", "-method", "sgd", "-learn_rate", "0.02",
                               "-seed", "42", "-serve", "int8", "-serve_prune", "seen", "-save_snapshot", snap, "-out", a],
                        cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    print(r1.stderr[-1500:])
    assert r1.returncode == 0 and "ERROR" not in r1.stderr
    assert [ln for ln in r1.stderr.splitlines() if ln.startswith("snapshot\tsave\tformat=int8\tpruned=1\t")]
    r2 = subprocess.run(cli + ["-method", "serve", "-load_snapshot", snap, "-test", tef, "-out", b],
                        cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    print(r2.stderr[-1500:])
    assert r2.returncode == 0 and "ERROR" not in r2.stderr
    assert [ln for ln in r2.stderr.splitlines() if ln.startswith("snapshot\tload\tformat=int8\tpruned=1\t")]
    assert [ln for ln in r2.stderr.splitlines() if ln.startswith("serve\tformat=int8\t")]
    assert "Loading train" not in r2.stdout
    assert os.path.getsize(a) > 0 and read(a) == read(b)
