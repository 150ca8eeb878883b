"""GPU: the pruned serving snapshot (fmx_compact_begin_pruned / fmx_compact_slot_of: k_prune_live, k_prune_mark, k_prune_keep, k_prune_dir,
the quantisers with a destination map, k_rowsums and k_fetch_rows over RowsI8P / RowsBf16P; include/fmx.h)
against libfm_amd/compact.py (pinned to a plain loop in tests/test_compact_pruned_cpu.py) and, bit for bit, against the DENSE snapshot
of the model with the dropped rows set to +0 on the same handle.

Shapes.  k in {0, 1, 8, 24, 56, 64, 100, 128, 256}: every lane map of both sources up to one row per wavefront, and the two widths
whose int8 block is smaller than its lane map (24: 32 of 64 bytes, 56: 64 of 128).  n in {1, 33, 200, 4099}: one ragged word, a word
and one id, a few words, many with a ragged tail.  k1 on and off, both tasks, both formats.  Kept patterns: none, all, only id 0,
only id n - 1, every other id, whole 32-id words dead, a random 10 % -- planted as the model's live rows (w = v = 0 elsewhere, some
of it -0), and cut further by a keep slot that names about half of the ids.  Rows are test_gpu_compact.make_rows (lengths 0, 1, 2, 33,
64, 65, 130: every tail of the round loop, a repeated id).  One case at n = 3e6 with 40 000 rows runs the grid-stride loops of every
build kernel and ids beyond 2^16 with about 10 % of the rows kept through a keep slot.

Tolerances.  Everything between the two snapshots is compared bit for bit: a dropped id yields the bits a stored row of +0 yields and
the code downstream is the same.  Against the restatement: slots, counts, bytes, nonfinite and max_abs_err exactly, sum_sq_err at rtol
1e-12 (an fp64 sum in another order), stored rows bit for bit, scores at the project's predict tolerance (RTOL, ATOL of
test_gpu_compact).

Measured on an MI355X: all 71 cases pass in 3.9 seconds; at n = 3e6 max_abs_err is equal and sum_sq_err differs by 4e-16 relative; every bit-for-bit
comparison holds, |pruned - restatement| stays below 4e-6 where 2e-5 + 1e-4 |score| is allowed (every test prints its own figure)."""
import ctypes as C

import numpy as np
import pytest

from libfm_amd import compact
from test_compact_pruned_cpu import PATTERNS, pattern, zeroed
from test_gpu_compact import (ATOL, ROWS, RTOL, compact_dtype, handle, make_params, make_rows, same_bits, tiny_regression,
                              trained_learner, write_libfm)

pytestmark = pytest.mark.gpu

FORMATS = ("int8", "bf16")
# (k, n, k1, task, pattern): every k, every n, k1 on and off, both tasks, every pattern
CASES = [(0, 200, True, 0, "alternate"), (0, 33, False, 1, "all"), (1, 4099, True, 1, "random10"), (1, 1, True, 0, "all"),
         (8, 33, True, 0, "first"), (8, 1, False, 1, "none"), (24, 200, False, 1, "dead_words"), (24, 4099, True, 0, "last"),
         (56, 200, True, 1, "alternate"), (56, 33, False, 0, "random10"), (64, 4099, True, 1, "dead_words"), (64, 200, False, 0, "all"),
         (64, 1, True, 1, "none"), (100, 200, True, 0, "random10"), (100, 4099, False, 1, "first"), (128, 200, True, 1, "last"),
         (128, 33, False, 0, "alternate"), (256, 200, False, 1, "dead_words"), (256, 33, True, 0, "none")]
IDS = ["k%d-n%d-%s-%s-%s" % (k, n, "k1" if k1 else "nok1", "cr"[1 - t], p) for k, n, k1, t, p in CASES]
SPECIAL = 3                                        # rows of the slot of planted entries (special_rows)


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


def planted_model(n, k, k1, live, seed):
    """make_params with the rows outside `live` made dead: v = 0 and (k1 on) w = 0, every third of them as -0; with k1 off half of the
    dead rows keep their w (it scores nothing).  With k = 0 and k1 off every row is dead whatever `live` says."""
    w0, w, v = make_params(n, k, seed)
    w, v = np.array(w), np.array(v)
    if k:
        v[0, live & (v[0] == 0)] = 0.125
    w[live & (w == 0)] = 0.125
    dead = np.flatnonzero(~live)
    v[:, dead] = 0.0
    v[:, dead[::3]] = -0.0
    if k1:
        w[dead] = 0.0
        w[dead[::3]] = -0.0
    else:
        w[dead[::2]] = 0.0
    return w0, w, v


def keep_rows(n, seed):
    """a slot whose entries name about half of the ids (id 0 and id n - 1 among them where n > 2), some twice, one with value 0"""
    rng = np.random.default_rng(900 + seed)
    ids = np.flatnonzero(rng.random(n) < 0.5)
    if n > 2:
        ids = np.union1d(ids, [0, n - 1])
    if n == 1:
        ids = np.array([0] if seed % 2 else [], dtype=np.int64)
    ids = rng.permutation(np.concatenate([ids, ids[:5]]))
    sizes = []
    while sum(sizes) < len(ids):
        sizes.append(min(int(rng.integers(0, 10)), len(ids) - sum(sizes)))
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ent = np.zeros(len(ids), dtype=compact_dtype())
    ent["id"], ent["value"] = ids, 1.0
    if len(ent):
        ent["value"][0] = 0.0                                                   # seen whatever the value
    return ent, rp


def special_rows(keep):
    """SPECIAL rows: a dropped id with value inf beside a kept one, a dropped id alone, nothing"""
    gone, kept = np.flatnonzero(~keep), np.flatnonzero(keep)
    a = ([(gone[0], np.inf)] if len(gone) else []) + ([(kept[0], 1.5)] if len(kept) else [])
    b = [(gone[-1], -2.0)] if len(gone) else []
    rows = [a, b, []]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    ent = np.zeros(int(rp[-1]), dtype=compact_dtype())
    flat = [e for r in rows for e in r]
    ent["id"], ent["value"] = [e[0] for e in flat], [e[1] for e in flat]
    return ent, rp


def fields(st, skip=("device_seconds", "rank_seconds")):
    return {f: getattr(st, f) for f, _ in st._fields_ if f not in skip}


def same_fields(a, b):
    fa, fb = fields(a), fields(b)
    return all(np.float64(fa[f]).tobytes() == np.float64(fb[f]).tobytes() for f in fa)


def outputs(h, capi, task, with_special):
    """everything a snapshot returns for the slots 0 (scored rows; queries and candidates of the top-K) and 3 (special rows)"""
    out = {"predict": h.compact_predict(0, ROWS), "evaluate": h.compact_evaluate(0), "topk": h.compact_topk(0, 0, 5)}
    out["ex"] = [h.compact_evaluate_ex(0, link) for link in ((capi.LINK_LOGISTIC, capi.LINK_PROBIT) if task == 1 else (capi.LINK_LOGISTIC,))]
    if with_special:
        out["special"] = h.compact_predict(3, SPECIAL)
    return out


def assert_same_outputs(a, b, what):
    assert same_bits(a["predict"], b["predict"]), what
    assert same_fields(a["evaluate"], b["evaluate"]), what
    for x, y in zip(a["ex"], b["ex"]):
        assert same_fields(x, y), what
    assert np.array_equal(a["topk"][0], b["topk"][0]) and same_bits(a["topk"][1], b["topk"][1]), what
    if "special" in a and "special" in b:
        assert same_bits(a["special"], b["special"]), what


def check_against_restatement(h, n, k, info, pinfo, pm):
    """check 1: slots, counts, bytes, the report and the stored rows"""
    ids = np.arange(n, dtype=np.uint32)
    assert np.array_equal(h.compact_slot_of(ids), pm.slot_of(ids))
    assert {f: int(getattr(pinfo, f)) for f, _ in pinfo._fields_} == pm.prune_info
    assert info.features == n and info.bytes_compact == pm.info["bytes_compact"] == pinfo.bytes_directory + pinfo.bytes_rows
    assert info.nonfinite == pm.info["nonfinite"] and info.max_abs_err == pm.info["max_abs_err"]
    assert abs(info.sum_sq_err - pm.info["sum_sq_err"]) <= 1e-12 * pm.info["sum_sq_err"]
    cw, cv = h.compact_rows(ids)
    nan = np.isnan(pm.v)
    assert same_bits(cw, pm.w) and np.array_equal(np.isnan(cv), nan) and same_bits(cv[~nan], pm.v[~nan])
    gone = ~pm.keep
    assert not cw[gone].any() and not np.signbit(cw[gone]).any() and not cv[:, gone].any() and not np.signbit(cv[:, gone]).any()


# ---- checks 1 - 5 on one handle per case ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("format", FORMATS)
@pytest.mark.parametrize("k, n, k1, task, pat", CASES, ids=IDS)
def test_pruned_snapshot_equals_the_dense_snapshot_of_the_zeroed_model(capi, format, k, n, k1, task, pat):
    fmt = compact.FORMATS[format]
    live = pattern(pat, n, seed=k)
    ent, rp, y = make_rows(n, 60 + k, task)
    kent, krp = keep_rows(n, k + n)
    h = handle(capi, n, k, k1, task, planted_model(n, k, k1, live, k + 7))
    try:
        h.upload_rows(0, ent, rp, y)
        h.upload_rows(1, kent, krp, None)
        w0, w, v = h.get_params()
        seen = compact.seen_mask(n, kent["id"])
        keep_d, keep_s = compact.prune_mask(w, v, k1), compact.prune_mask(w, v, k1, seen)
        if k or k1:
            assert np.array_equal(keep_d, live)                                 # (the planted pattern is what the rule finds)
        sent, srp = special_rows(keep_s)
        h.upload_rows(3, sent, srp, None)
        # FMX_PRUNE_DEAD alone
        info, pinfo = h.compact_begin_pruned(fmt)
        pm = compact.CompactModel(w0, w, v, True, k1, format, keep=keep_d)
        check_against_restatement(h, n, k, info, pinfo, pm)
        assert pinfo.dropped_dead == h.param_sparsity().dead_features == n - int(keep_d.sum()) and pinfo.dropped_unseen == 0    # check 2
        out_d = outputs(h, capi, task, False)
        want = pm.predict(ent, rp)
        print("%s k %d n %d %s: kept %d of %d, bytes %d (directory %d); |pruned - restatement| max %.3g" % (
            format, k, n, pat, pinfo.kept, n, info.bytes_compact, pinfo.bytes_directory, np.abs(out_d["predict"] - want).max()))
        np.testing.assert_allclose(out_d["predict"], want, rtol=RTOL, atol=ATOL)                                        # check 5
        dense_info = h.compact_begin(fmt)                                       # check 4: the unmodified model, rows of -0 included
        assert_same_outputs(out_d, outputs(h, capi, task, False), "dead alone against the dense snapshot of the model as it is")
        assert dense_info.bytes_compact == n * compact.row_bytes(format, k)
        with pytest.raises(capi.FmxError) as ei:                                # (a dense snapshot has no slots)
            h.compact_slot_of(np.zeros(1, dtype=np.uint32))
        assert ei.value.code == -3
        # FMX_PRUNE_DEAD | FMX_PRUNE_SEEN
        info, pinfo = h.compact_begin_pruned(fmt, seen_slot=1)
        pm = compact.CompactModel(w0, w, v, True, k1, format, keep=keep_s, seen=seen)
        check_against_restatement(h, n, k, info, pinfo, pm)
        assert pinfo.kept + pinfo.dropped_dead + pinfo.dropped_unseen == n
        out_s = outputs(h, capi, task, True)
        with np.errstate(invalid="ignore"):
            np.testing.assert_allclose(out_s["predict"], pm.predict(ent, rp), rtol=RTOL, atol=ATOL)
            # (row 0 holds an inf: the device multiplies the padding of a row by it too, the restatement has no padding -- at k = 0 with
            # k1 off they differ there, so that row is compared with the zeroed dense snapshot alone)
            np.testing.assert_allclose(out_s["special"][1:], pm.predict(sent, srp)[1:], rtol=RTOL, atol=ATOL)
        if (~keep_s).any():
            assert np.isnan(out_s["special"][0])                                # check 6: inf on a dropped id is 0 * inf
        assert out_s["special"][2] == float(np.float32(w0))
        # check 3: the dense snapshots of the model with the dropped rows set to +0
        for keep, out, what in ((keep_d, out_d, "dead"), (keep_s, out_s, "dead | seen")):
            h.set_params(w0, *zeroed(w, v, keep))
            h.compact_begin(fmt)
            assert_same_outputs(out, outputs(h, capi, task, True), what + " against the dense snapshot of the zeroed model")
    finally:
        h.close()


@pytest.mark.parametrize("n", (1, 33, 200, 4099))
@pytest.mark.parametrize("pat", PATTERNS)
def test_every_pattern_at_every_size(capi, n, pat):
    """the directory build alone decides these: slots and counts against the restatement, scores against the zeroed dense snapshot"""
    k, k1, task = 8, True, 0
    format = FORMATS[(n + len(pat)) % 2]
    fmt = compact.FORMATS[format]
    live = pattern(pat, n)
    ent, rp, y = make_rows(n, 5, task)
    h = handle(capi, n, k, k1, task, planted_model(n, k, k1, live, 3))
    try:
        h.upload_rows(0, ent, rp, y)
        w0, w, v = h.get_params()
        info, pinfo = h.compact_begin_pruned(fmt)
        pm = compact.CompactModel(w0, w, v, True, k1, format, keep=live)
        check_against_restatement(h, n, k, info, pinfo, pm)
        got = h.compact_predict(0, ROWS)
        if pat == "none":
            assert pinfo.kept == 0 and np.all(got == float(np.float32(w0)))     # kept = 0 scores w0 plus nothing
        h.set_params(w0, *zeroed(w, v, live))
        h.compact_begin(fmt)
        assert same_bits(got, h.compact_predict(0, ROWS))
    finally:
        h.close()


# ---- the large case ------------------------------------------------------------------------------------------------------------
def test_grid_stride_loops_and_ids_beyond_2_16(capi):
    n, k, rows, nnz = 3_000_000, 8, 40_000, 8
    rng = np.random.default_rng(321)
    seen_ids = np.flatnonzero(rng.random(n) < 0.1)
    seen_ids = np.union1d(seen_ids, np.arange(n - nnz, n))
    kent = np.zeros(len(seen_ids) // nnz * nnz + nnz, dtype=compact_dtype())
    kent["id"] = np.resize(rng.permutation(seen_ids), len(kent))
    kent["id"][:nnz] = np.arange(n - nnz, n)
    kent["value"] = 1.0
    krp = (np.arange(len(kent) // nnz + 1) * nnz).astype(np.uint64)
    ent = np.zeros(rows * nnz, dtype=compact_dtype())
    ent["id"] = np.where(rng.random(rows * nnz) < 0.5, rng.choice(seen_ids, rows * nnz), rng.integers(0, n, rows * nnz))
    ent["id"][:nnz] = np.arange(n - nnz, n)                                     # the last features of the table
    ent["value"] = np.round(rng.normal(0.0, 1.0, rows * nnz), 3)
    rp = (np.arange(rows + 1) * nnz).astype(np.uint64)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    h = capi.Handle(n, k, True, True, 1, 0.0, 0.001, 0.002, 0.01, -1.0, 1.0)
    try:
        h.init_params(0.0, 0.05, 7)
        h.upload_rows(0, ent, rp, y)
        h.upload_rows(1, kent, krp, None)
        w0, w, v = h.get_params()
        w[::7] = 0.0078125                                                         # ... the others score, every 7th through w too
        v[:, ::5] = 0.0                                                         # every 5th row is dead (init_params leaves w = 0) ...
        w[::35] = 0.0
        h.set_params(w0, w, v)
        seen = compact.seen_mask(n, kent["id"])
        keep = compact.prune_mask(w, v, True, seen)
        dead = compact.dead_mask(w, v, True)
        info, pinfo = h.compact_begin_pruned(capi.COMPACT_INT8, seen_slot=1)
        assert (pinfo.features, pinfo.kept, pinfo.dropped_dead, pinfo.dropped_unseen) == (n, int(keep.sum()), int(dead.sum()), int((~dead & ~seen).sum()))
        assert 0.05 * n < pinfo.kept < 0.15 * n and pinfo.dropped_dead == h.param_sparsity().dead_features
        assert pinfo.bytes_directory == 8 * ((n + 31) // 32) and pinfo.bytes_rows == pinfo.kept * 16
        assert info.bytes_compact == pinfo.bytes_directory + pinfo.bytes_rows
        mx, ss, nf = compact.quant_report(np.asarray(v[:, keep], dtype=np.float32), "int8")      # the report over the kept rows, as check 1
        print("n %d: max_abs_err %.9g (want %.9g) sum_sq_err %.17g (want %.17g)" % (n, info.max_abs_err, mx, info.sum_sq_err, ss))
        assert info.nonfinite == nf == 0 and info.max_abs_err == mx > 0 and abs(info.sum_sq_err - ss) <= 1e-12 * ss
        d = compact.directory(keep)
        assert np.array_equal(h.compact_slot_of(np.arange(n, dtype=np.uint32)), compact.slot_of(d, np.arange(n)))
        got = h.compact_predict(0, rows)
        ev, ex, tk = h.compact_evaluate(0), h.compact_evaluate_ex(0), h.compact_topk(0, 0, 3, 0, 64)
        ids, inv = np.unique(ent["id"], return_inverse=True)
        assert ids.max() == n - 1 and ids.max() > 2 ** 16 and not keep[ids].all() and keep[ids].any()
        local = ent.copy()
        local["id"] = inv
        pm = compact.CompactModel(w0, w[ids], v[:, ids], True, True, "int8", keep=keep[ids])
        cw, cv = h.compact_rows(ids.astype(np.uint32))
        assert same_bits(cw, pm.w) and same_bits(cv, pm.v)
        want = pm.predict(local, rp)
        print("n %d: kept %d (%.1f %%), bytes %d against %d dense; |pruned - restatement| max %.3g" % (
            n, pinfo.kept, 100.0 * pinfo.kept / n, info.bytes_compact, n * 16, np.abs(got - want).max()))
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
        h.set_params(w0, *zeroed(w, v, keep))
        assert h.compact_begin(capi.COMPACT_INT8).bytes_compact == n * 16
        assert same_bits(got, h.compact_predict(0, rows))
        assert same_fields(ev, h.compact_evaluate(0)) and same_fields(ex, h.compact_evaluate_ex(0))
        tk2 = h.compact_topk(0, 0, 3, 0, 64)
        assert np.array_equal(tk[0], tk2[0]) and same_bits(tk[1], tk2[1])
    finally:
        h.close()


# ---- check 6: lifetime ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("format, k", [("int8", 64), ("bf16", 8)])
def test_frozen_and_replaced(capi, format, k):
    n, k1, task = 200, True, 0
    fmt = compact.FORMATS[format]
    live = pattern("random10", n) | pattern("dead_words", n)
    ent, rp, y = make_rows(n, 70 + k, task)
    h = handle(capi, n, k, k1, task, planted_model(n, k, k1, live, k), lr=0.05)
    try:
        h.upload_rows(0, ent, rp, y)
        w0, w, v = h.get_params()
        p0 = h.predict(0, ROWS)
        info, pinfo = h.compact_begin_pruned(fmt, seen_slot=0)
        seen = compact.seen_mask(n, ent["id"])
        assert pinfo.kept == int((live & seen).sum())
        c0 = h.compact_predict(0, ROWS)
        slots0 = h.compact_slot_of(np.arange(n, dtype=np.uint32))
        assert same_bits(h.predict(0, ROWS), p0)                                # taking the snapshot wrote nothing
        h.sgd_epoch(0, capi.SGD_MINIBATCH, batch=16)                            # training an epoch changes nothing it returns
        assert not same_bits(h.predict(0, ROWS), p0)
        assert same_bits(h.compact_predict(0, ROWS), c0)
        assert np.array_equal(h.compact_slot_of(np.arange(n, dtype=np.uint32)), slots0)
        # dense -> pruned -> dense -> pruned, each of the model as it stands then
        for turn in range(2):
            w0t, wt, vt = h.get_params()
            h.compact_begin(fmt)
            dense = h.compact_predict(0, ROWS)
            np.testing.assert_allclose(dense, compact.CompactModel(w0t, wt, vt, True, k1, format).predict(ent, rp), rtol=RTOL, atol=ATOL)
            info, pinfo = h.compact_begin_pruned(fmt)
            keep = compact.prune_mask(wt, vt, k1)
            assert pinfo.kept == int(keep.sum())
            assert same_bits(h.compact_predict(0, ROWS), dense)                 # (dead rows only: the dense scores themselves)
            assert np.array_equal(h.compact_slot_of(np.arange(n, dtype=np.uint32)), compact.slot_of(compact.directory(keep), np.arange(n)))
            h.set_params(w0t + 0.5, wt * 0.5, vt)
        h.compact_end()
        with pytest.raises(capi.FmxError) as ei:
            h.compact_slot_of(np.zeros(1, dtype=np.uint32))
        assert ei.value.code == -3
        # kept = 0: w0 plus nothing
        h.set_params(0.25, np.zeros(n), np.zeros((k, n)))
        info, pinfo = h.compact_begin_pruned(fmt)
        assert (pinfo.kept, pinfo.dropped_dead, pinfo.bytes_rows) == (0, n, 0) and info.bytes_compact == pinfo.bytes_directory
        assert np.all(h.compact_predict(0, ROWS) == 0.25)
        assert np.all(h.compact_slot_of(np.arange(n, dtype=np.uint32)) == capi.SLOT_NONE)
        cw, cv = h.compact_rows(np.arange(n, dtype=np.uint32))
        assert not cw.any() and not cv.any()
    finally:
        h.close()


# ---- check 7: refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(capi):
    lib = capi.load()
    k, n = 8, 200
    ent, rp, y = make_rows(n, 50, 1)
    h = handle(capi, n, k, True, 1, make_params(n, k, 5))
    info, pinfo = capi.CompactInfo(), capi.CompactPruneInfo()
    ids, out = np.arange(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    O = capi.CompactPruneOpts
    D, S = capi.PRUNE_DEAD, capi.PRUNE_SEEN

    def begin(o):
        return lib.fmx_compact_begin_pruned(h.h, None if o is None else C.byref(o), C.byref(info), C.byref(pinfo))

    def refused(rc, code, name="fmx_compact_begin_pruned"):
        assert rc == code, (name, rc)
        assert name.encode() in lib.fmx_last_error(h.h), lib.fmx_last_error(h.h)

    def usable():
        assert begin(O(capi.COMPACT_INT8, D | S, 0, 0)) == 0 and pinfo.features == n and pinfo.kept > 0
        assert np.all(np.isfinite(h.compact_predict(0, ROWS)))

    try:
        h.upload_rows(0, ent, rp, y)
        refused(lib.fmx_compact_slot_of(h.h, ids.ctypes.data, 4, out.ctypes.data), -3, "fmx_compact_slot_of")     # no snapshot at all
        refused(begin(None), -1)
        refused(begin(O(2, D, -1, 0)), -1)
        refused(begin(O(0, D, -1, 0)), -1)
        refused(begin(O(capi.COMPACT_BF16, 0, -1, 0)), -1)                       # flags without FMX_PRUNE_DEAD
        refused(begin(O(capi.COMPACT_BF16, S, 0, 0)), -1)
        refused(begin(O(capi.COMPACT_BF16, D | 4, -1, 0)), -1)                   # unknown bits
        refused(begin(O(capi.COMPACT_BF16, D, -1, 1)), -1)                       # reserved
        refused(begin(O(capi.COMPACT_BF16, D, 0, 0)), -1)                        # keep_slot without FMX_PRUNE_SEEN
        refused(begin(O(capi.COMPACT_BF16, D | S, 99, 0)), -1)
        refused(begin(O(capi.COMPACT_BF16, D | S, -1, 0)), -1)
        refused(begin(O(capi.COMPACT_BF16, D | S, 5, 0)), -3)                    # a slot that was never uploaded
        with pytest.raises(capi.FmxError):                                       # (nothing above left a snapshot behind)
            h.compact_predict(0, ROWS)
        usable()
        assert lib.fmx_compact_begin_pruned(h.h, C.byref(O(capi.COMPACT_BF16, D, -1, 0)), None, None) == 0     # either may be NULL
        bad = np.array([0, n], dtype=np.uint32)
        refused(lib.fmx_compact_slot_of(h.h, bad.ctypes.data, 2, out.ctypes.data), -1, "fmx_compact_slot_of")
        refused(lib.fmx_compact_slot_of(h.h, None, 2, out.ctypes.data), -1, "fmx_compact_slot_of")
        refused(lib.fmx_compact_slot_of(h.h, ids.ctypes.data, 2, None), -1, "fmx_compact_slot_of")
        wv = np.zeros(2 * (k + 1))
        refused(lib.fmx_compact_get_rows(h.h, bad.ctypes.data, 2, wv.ctypes.data, wv.ctypes.data), -1, "fmx_compact_get_rows")
        assert lib.fmx_compact_slot_of(h.h, ids.ctypes.data, 0, out.ctypes.data) == 0
        usable()
        # a keep_slot with kept `-relation` blocks
        main = np.zeros(6, dtype=capi.ENTRY_DTYPE)
        main["id"], main["value"] = np.arange(6), 1.0
        bent = np.zeros(3, dtype=capi.ENTRY_DTYPE)
        bent["id"], bent["value"] = np.arange(3), 0.5
        rel = [(bent, np.arange(4, dtype=np.uint64), np.array([0, 1, 2, 0, 1, 2], dtype=np.uint32), 10)]
        h.upload_block_rows(3, main, np.arange(7, dtype=np.uint64), np.ones(6, np.float32), rel, keep=True)
        refused(begin(O(capi.COMPACT_INT8, D | S, 3, 0)), -4)
        usable()
        assert h.compact_slot_of(ids).shape == (4,)
        assert lib.fmx_compact_end(h.h) == 0
        assert np.all(np.isfinite(h.predict(0, ROWS)))
    finally:
        h.close()
    hs = handle(capi, n, k, True, 1, None, shard_rank=0, shard_world=2)          # a feature shard
    try:
        assert lib.fmx_compact_begin_pruned(hs.h, C.byref(O(capi.COMPACT_INT8, D, -1, 0)), C.byref(info), C.byref(pinfo)) == -4
        assert b"fmx_compact_begin_pruned" in lib.fmx_last_error(hs.h)
        assert lib.fmx_compact_slot_of(hs.h, ids.ctypes.data, 4, out.ctypes.data) == -4
        hs.upload_rows(0, ent, rp, y)                                            # (still usable)
    finally:
        hs.close()


# ---- check 8: learner and CLI --------------------------------------------------------------------------------------------------
def test_learner_view_and_cli_serve_prune(capi, tmp_path, capsys):
    from libfm_amd import cli
    from libfm_amd import data as D
    from libfm_amd import learner as L
    k, iters = 8, 3
    tr_raw, te_raw = tiny_regression(1, n=40), tiny_regression(2, n=60)          # the test rows name features training never saw
    trf, tef, outs = (str(tmp_path / f) for f in ("tr.libfm", "te.libfm", "serve.txt"))
    write_libfm(trf, *tr_raw)
    write_libfm(tef, *te_raw)
    tr, te = L.Data(*D.load(trf)), L.Data(*D.load(tef))
    l = trained_learner(L, tr, te, k, iters)
    try:
        n = l.fm.num_attribute
        seen = compact.seen_mask(n, tr.entries["id"])
        dense = l.compact("int8")
        assert dense.prune_info is None
        view = l.compact(format="int8", prune="seen")
        pi = view.prune_info
        assert (pi.features, pi.kept, pi.dropped_unseen) == (n, int(seen.sum()) - pi.dropped_dead, n - int(seen.sum())) and pi.dropped_unseen > 0
        assert view.info.bytes_compact == pi.bytes_directory + pi.bytes_rows == 8 * ((n + 31) // 32) + pi.kept * 16
        w0, w, v = l._h.get_params()
        pm = compact.CompactModel(w0, w, v, True, True, "int8", keep=compact.prune_mask(w, v, True, seen), seen=seen)
        assert {f: int(getattr(pi, f)) for f, _ in pi._fields_} == pm.prune_info
        np.testing.assert_allclose(view.predict_raw(te), pm.predict(te.entries, te.row_ptr), rtol=RTOL, atol=ATOL)
        want_out, metric = view.predict(te), view.evaluate(te)
        counts = {f: int(getattr(pi, f)) for f, _ in pi._fields_}
        dead_view = l.compact("int8", prune="dead")
        assert dead_view.prune_info.dropped_unseen == 0 and same_bits(dead_view.predict_raw(te), l.compact("int8").predict_raw(te))
        with pytest.raises(ValueError, match="unknown prune rule"):
            l.compact("int8", prune="small")
        view.close()
    finally:
        l.close()
    capsys.readouterr()
    argv = ["-task", "r", "-train", trf, "-test", tef, "-dim", "1,1,%d" % k, "-iter", str(iters), "-method", "sgd", "-learn_rate", "0.02",
            "-init_stdev", "0.1", "-seed", "42"]
    assert cli.main(argv + ["-out", outs, "-serve", "int8", "-serve_prune", "seen"]) == 0
    line = [ln for ln in capsys.readouterr().err.splitlines() if ln.startswith("compact\t")]
    assert len(line) == 1
    got = dict(f.split("=") for f in line[0].split("\t")[1:])
    assert got["format"] == "int8" and got["prune"] == "seen"
    assert {f: int(got[f]) for f in ("kept", "dropped_dead", "dropped_unseen", "bytes_directory", "bytes_rows")} == {
        f: counts[f] for f in ("kept", "dropped_dead", "dropped_unseen", "bytes_directory", "bytes_rows")}
    assert int(got["bytes"]) == counts["bytes_directory"] + counts["bytes_rows"]
    assert float(got["Test(int8)"]) == pytest.approx(metric, rel=1e-5)
    p_serve = np.array([float(x) for x in open(outs).read().split()])
    np.testing.assert_allclose(p_serve, want_out, rtol=1e-5, atol=1e-9)           # (%g keeps 6 digits)
    assert cli.main(argv + ["-serve_prune", "seen"]) == 0
    assert "ERROR: -serve_prune needs -serve" in capsys.readouterr().err
