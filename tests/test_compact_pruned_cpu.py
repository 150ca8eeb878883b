"""CPU: the pruned serving snapshot's restatement (libfm_amd/compact.py: prune_mask, directory, slot_of, CompactModel(keep=...);
include/fmx.h "fmx_compact_begin_pruned") and what of the two new entry points can be checked without a device.

The directory and the lookup are checked against a plain Python loop -- a second statement of the format -- at sizes around the
32-id word (n = 1, 31, 32, 33, 64), at a few words (200) and at many with a ragged tail (4099), under the kept patterns none, all,
only id 0, only id n - 1, every other id, whole words dead and a random 10 %.  The pruned CompactModel must score, bit for bit, what
the dense CompactModel of the model with the dropped rows zeroed scores: both run the same fp64 formula on the same values."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_compact_cpu import planted

SIZES = (1, 31, 32, 33, 64, 200, 4099)
PATTERNS = ("none", "all", "first", "last", "alternate", "dead_words", "random10")


def pattern(name, n, seed=0):
    m = np.zeros(n, dtype=bool)
    if name == "all":
        m[:] = True
    elif name == "first":
        m[0] = True
    elif name == "last":
        m[n - 1] = True
    elif name == "alternate":
        m[::2] = True
    elif name == "dead_words":                     # words 0, 2, 4, ... are dead as a whole, the others kept as a whole
        m[:] = (np.arange(n) // 32) % 2 == 1
    elif name == "random10":
        m[:] = np.random.default_rng(100 + n + seed).random(n) < 0.1
    elif name != "none":
        raise ValueError(name)
    return m


def loop_directory(mask):
    """[(bits, base)] per 32 ids and the slot of every id, one id at a time"""
    pairs, slots, kept = [], [], 0
    for j in range(0, len(mask), 32):
        bits, base = 0, kept
        for b, on in enumerate(mask[j:j + 32]):
            if on:
                bits |= 1 << b
                slots.append(kept)
                kept += 1
            else:
                slots.append(0xFFFFFFFF)
        pairs.append((bits, base))
    return pairs, slots


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", PATTERNS)
def test_directory_and_slot_of_against_a_loop(n, name):
    from libfm_amd import compact
    m = pattern(name, n)
    d = compact.directory(m)
    pairs, slots = loop_directory(m)
    assert d.dtype == np.uint32 and d.shape == ((n + 31) // 32, 2)
    assert [(int(a), int(b)) for a, b in d] == pairs
    got = compact.slot_of(d, np.arange(n))
    assert got.dtype == np.uint32 and got.tolist() == slots
    order = np.random.default_rng(n).permutation(n)                    # any order, repeats allowed
    ids = np.concatenate([order, order[:3]])
    assert compact.slot_of(d, ids).tolist() == [slots[i] for i in ids]
    assert compact.SLOT_NONE == 0xFFFFFFFF
    # slots are the kept ids in ascending id order
    assert np.array_equal(np.flatnonzero(m), np.flatnonzero(got != compact.SLOT_NONE))
    assert np.array_equal(got[m], np.arange(int(m.sum()), dtype=np.uint32))


def loop_dead(w, v, k1):
    """fmx_param_sparsity's dead_features rule, one feature at a time, on the fp32 values"""
    w32, v32 = np.asarray(w, dtype=np.float32), np.asarray(v, dtype=np.float32)
    out = []
    for j in range(len(w32)):
        vz = all(float(v32[f, j]) == 0.0 for f in range(v32.shape[0]))
        out.append(vz and (float(w32[j]) == 0.0 or not k1))
    return np.array(out, dtype=bool)


def model(n, k, seed, k1=True):
    """a seeded model with planted rows: dead ones (w = 0, v = 0), rows of -0, rows with only w or only one factor alive, the special
    values of test_compact_cpu.planted in live rows and -- where n allows -- a NaN row (returned: its id or None)"""
    rng = np.random.default_rng(seed)
    w = rng.normal(0.0, 0.3, n)
    v = rng.normal(0.0, 0.3 / np.sqrt(max(k, 1)), (k, n))
    dead = rng.random(n) < 0.3
    w[dead], v[:, dead] = 0.0, 0.0
    neg = rng.random(n) < 0.1                                          # -0 everywhere: dead too
    w[neg], v[:, neg] = -0.0, -0.0
    only_w = rng.random(n) < 0.1
    v[:, only_w] = 0.0                                                 # dead exactly when k1 is off (or w is 0 already)
    if k:
        only_v = rng.random(n) < 0.1
        w[only_v], v[:, only_v] = 0.0, 0.0
        v[k - 1, only_v] = 0.25
    px, _ = planted()
    fin = px[np.isfinite(px)]
    if k and n >= 64:
        v[0, 40:40 + len(fin)] = fin                                   # ties, subnormals, the overflow to inf
    nan_id = None
    if k and n >= 33:
        nan_id = 32
        w[nan_id], v[:, nan_id] = 0.0, 0.0
        v[0, nan_id] = np.nan                                          # NaN != 0: not dead
    return 0.3, w, v, nan_id


def rows_over(n, seed, skip=None, force=None, rows=30):
    """seeded rows over the ids 0 .. n - 1 (never `skip`, `force` at least once), real values, an empty row and repeated ids among them"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 12, rows)
    sizes[0] = 0
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ent = np.zeros(int(rp[-1]), dtype=np.dtype([("id", np.uint32), ("value", np.float32)]))
    pool = np.array([i for i in range(n) if i != skip] or [0])
    ent["id"] = rng.choice(pool, size=len(ent))
    ent["value"] = np.round(rng.normal(0.0, 1.0, len(ent)), 3)
    if force is not None:
        ent["id"][len(ent) // 2] = force
    return ent, rp


def zeroed(w, v, keep):
    w2, v2 = np.array(w, dtype=np.float64), np.array(v, dtype=np.float64)
    w2[~keep] = 0.0
    v2[:, ~keep] = 0.0
    return w2, v2


@pytest.mark.parametrize("format", ["bf16", "int8"])
@pytest.mark.parametrize("n, k, k1", [(1, 4, True), (33, 1, True), (200, 8, True), (200, 8, False), (4099, 5, True), (200, 0, True)])
def test_pruned_model_scores_as_the_dense_model_with_dropped_rows_zeroed(format, n, k, k1):
    from libfm_amd import compact
    w0, w, v, nan_id = model(n, k, 7 * n + k, k1)
    train = rows_over(n, 1 + n, skip=nan_id)                           # the NaN row is unseen
    test = rows_over(n, 2 + n, force=nan_id)                           # ... and the scored rows name it
    seen = compact.seen_mask(n, train[0]["id"])
    dead = loop_dead(w, v, k1)
    assert np.array_equal(compact.dead_mask(w, v, k1), dead)
    for s in (None, seen):
        keep = compact.prune_mask(w, v, k1, s)
        assert np.array_equal(keep, ~dead & (seen if s is not None else True))
        pm = compact.CompactModel(w0, w, v, True, k1, format, keep=keep, seen=s)
        dm = compact.CompactModel(w0, *zeroed(w, v, keep), True, k1, format)
        with np.errstate(invalid="ignore"):                            # (inf - inf in the rows that meet the planted overflow)
            for ent, rp in (train, test):
                a, b = pm.predict(ent, rp), dm.predict(ent, rp)
                assert a.tobytes() == b.tobytes()
            if s is None and nan_id is not None:
                assert keep[nan_id] and np.isnan(pm.predict(*test)).any()  # kept: its NaN reaches the scores
        if s is not None and nan_id is not None:
            assert not keep[nan_id]
        # rows in slot order, the directory, the counts and the report over the kept rows
        ids = np.flatnonzero(keep)
        dense = compact.CompactModel(w0, w, v, True, k1, format)
        assert np.array_equal(pm.rows_w, np.asarray(w, dtype=np.float64)[ids])
        assert pm.rows_v.shape == (k, len(ids)) and pm.rows_v.tobytes() == np.ascontiguousarray(dense.v[:, ids] if k else pm.rows_v).tobytes()
        assert np.array_equal(pm.slot_of(np.arange(n)), compact.slot_of(compact.directory(keep), np.arange(n)))
        pi = pm.prune_info
        assert pi["features"] == n and pi["kept"] == len(ids) and pi["dropped_dead"] == int(dead.sum())
        assert pi["dropped_unseen"] == (int((~dead & ~seen).sum()) if s is not None else 0)
        assert pi["kept"] + pi["dropped_dead"] + pi["dropped_unseen"] == n
        assert pi["bytes_directory"] == 8 * ((n + 31) // 32) and pi["bytes_rows"] == len(ids) * compact.row_bytes(format, k)
        assert pm.info["bytes_compact"] == pi["bytes_directory"] + pi["bytes_rows"]
        v32 = np.asarray(v, dtype=np.float32)
        assert (pm.info["max_abs_err"], pm.info["sum_sq_err"], pm.info["nonfinite"]) == compact.quant_report(v32[:, ids], format)


def test_dropped_dead_is_the_dead_count_of_param_sparsity():
    """under FMX_PRUNE_DEAD alone: dropped_dead = dead_features, nothing is unseen, and -0 counts as zero while NaN does not"""
    from libfm_amd import compact
    for n, k, k1 in [(200, 8, True), (200, 8, False), (33, 1, True), (64, 0, True), (64, 0, False)]:
        w0, w, v, _ = model(n, k, n + k, k1)
        dead = loop_dead(w, v, k1)
        pm = compact.CompactModel(w0, w, v, True, k1, "int8", keep=compact.prune_mask(w, v, k1))
        assert pm.prune_info["dropped_dead"] == int(dead.sum()) > 0 and pm.prune_info["dropped_unseen"] == 0
        assert pm.prune_info["kept"] == n - int(dead.sum())
    w, v = np.array([-0.0, 0.0, 0.0, 1.0]), np.array([[-0.0, np.nan, 0.0, 0.0]])
    assert compact.dead_mask(w, v, True).tolist() == [True, False, True, False]
    assert compact.dead_mask(w, v, False).tolist() == [True, False, True, True]
    assert compact.dead_mask(w, np.zeros((0, 4)), True).tolist() == [True, True, True, False]      # num_factor = 0


def test_an_infinite_value_on_a_dropped_id_gives_nan_as_from_the_zero_row():
    from libfm_amd import compact
    w0, w, v, _ = model(64, 4, 5)
    keep = compact.prune_mask(w, v, True)
    gone = int(np.flatnonzero(~keep)[0])
    ent = np.zeros(2, dtype=np.dtype([("id", np.uint32), ("value", np.float32)]))
    ent["id"], ent["value"] = (gone, int(np.flatnonzero(keep)[0])), (np.inf, 1.0)
    rp = np.array([0, 2], dtype=np.uint64)
    with np.errstate(invalid="ignore"):
        a = compact.CompactModel(w0, w, v, keep=keep).predict(ent, rp)
        b = compact.CompactModel(w0, *zeroed(w, v, keep)).predict(ent, rp)
    assert np.isnan(a[0]) and a.tobytes() == b.tobytes()


# ---- the declarations, the binding and the refusals that need no device --------------------------------------------------------
FUNCTIONS = {
    "fmx_compact_begin_pruned": "fmx_handle h, const fmx_compact_prune_opts *o, fmx_compact_info *info, fmx_compact_prune_info *pinfo",
    "fmx_compact_slot_of": "fmx_handle h, const uint32_t *ids, uint32_t count, uint32_t *slot_out",
}


def test_header_declares_and_capi_binds_the_two_functions():
    from libfm_amd import capi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    bound = {name: (res, args) for name, res, args in capi.SYMBOLS}
    structs = {"fmx_compact_prune_opts": capi.CompactPruneOpts, "fmx_compact_info": capi.CompactInfo,
               "fmx_compact_prune_info": capi.CompactPruneInfo}
    for name, params in FUNCTIONS.items():
        mt = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert mt, name
        got = [" ".join(p.split()) for p in mt.group(1).split(",")]
        assert got == [" ".join(p.split()) for p in params.split(",")], name
        res, args = bound[name]
        assert res is C.c_int and len(args) == len(got)
        for p, a in zip(got, args):
            base = p.replace("const ", "").split()[0]
            if base in structs:
                assert a is C.POINTER(structs[base]), (name, p)
    assert re.search(r"#define\s+FMX_PRUNE_DEAD\s+1u", txt) and re.search(r"#define\s+FMX_PRUNE_SEEN\s+2u", txt)
    assert (capi.PRUNE_DEAD, capi.PRUNE_SEEN, capi.SLOT_NONE) == (1, 2, 0xFFFFFFFF)
    assert C.sizeof(capi.CompactPruneOpts) == 16 and [f for f, _ in capi.CompactPruneOpts._fields_] == ["format", "flags", "keep_slot", "reserved"]
    assert C.sizeof(capi.CompactPruneInfo) == 48 and [f for f, _ in capi.CompactPruneInfo._fields_] == [
        "features", "kept", "dropped_dead", "dropped_unseen", "bytes_directory", "bytes_rows"]
    assert callable(capi.Handle.compact_begin_pruned) and callable(capi.Handle.compact_slot_of)


def test_symbols_without_an_abi_version_change_and_null_handles():
    from libfm_amd import build, capi
    build.build()
    lib = capi.load()
    assert lib.fmx_abi_version() == 11
    opts, info, pinfo = capi.CompactPruneOpts(capi.COMPACT_INT8, capi.PRUNE_DEAD, -1, 0), capi.CompactInfo(), capi.CompactPruneInfo()
    ids, out = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    assert lib.fmx_compact_begin_pruned(None, C.byref(opts), C.byref(info), C.byref(pinfo)) == -1
    assert lib.fmx_compact_begin_pruned(None, None, None, None) == -1
    assert lib.fmx_compact_slot_of(None, ids.ctypes.data, 1, out.ctypes.data) == -1


@pytest.mark.parametrize("argv, text", [
    (["-method", "sgd", "-serve_prune", "dead"], "ERROR: -serve_prune needs -serve"),
    (["-method", "sgd", "-serve", "int8", "-serve_prune", "small"], "ERROR: -serve_prune knows dead and seen, not 'small'"),
    (["-method", "mcmc", "-serve", "int8", "-serve_prune", "seen"], "ERROR: -serve is not supported with -method mcmc"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    assert cli.main(["-task", "r", "-train", "no_such_train", "-test", "no_such_test", "-learn_rate", "0.01"] + argv) == 0
    assert text in capsys.readouterr().err


def test_learners():
    from libfm_amd import learner as L
    with pytest.raises(ValueError, match="unknown prune rule"):
        L.CompactView(L.FMLearnSGD(), "int8", "magnitude")
    with pytest.raises(NotImplementedError, match="average over the draws"):
        L.FMLearnMCMC().compact("int8", prune="dead")
    assert L.CompactView.PRUNE == (None, "dead", "seen")
