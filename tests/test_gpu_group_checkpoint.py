"""GPU: group checkpoints (fmx_group_checkpoint_save / _load; csrc/fmx_ckpt.hip, k_ckpt_rows_shard / k_ckpt_merge / k_ckpt_global_ids
in fmx_ckpt_kernels.h): a group of feature shards writes the file ONE unsharded handle with the same state
writes, in global feature order, and a group of any shard count -- or a handle -- loads it.

Every comparison is of bit patterns or bytes; no tolerance appears.  The reference for the file's bytes is the existing single-handle
fmx_checkpoint_save and the numpy restatement libfm_amd/checkpoint.py, never the group's own save.  Groups are loopback shards on
device 0, built by make_group of tests/test_gpu_group_stateful.py; the data cases and helpers are tests/test_gpu_checkpoint.py's."""
import io
import os
import struct

import numpy as np
import pytest

import test_gpu_checkpoint as TC
from group_checkpoint_cases import EDGE_CASES, MULTI_CHUNK, edge_ids, edge_properties
from oracle import oracle as O
from test_checkpoint_cpu import bits, sparse_case
from test_ftrl_cpu import PARITY, parity_case
from test_gpu_group_stateful import close, make_group

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_UNSUPPORTED = -1, -3, -4
N, LR = TC.N, TC.LR
WORLDS = [(2, 0), (3, 1), (8, 1)]                               # (world, shard_hash)
SESSION = {"adagrad": 1, "ftrl": 2, None: 0}


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


def group(capi, m, world, shard_hash, d=None):
    hs, grp = make_group(capi, world, [0] * world, m, 1, LR, -1.0, 1.0, shard_hash)
    if d is not None:
        grp.upload_rows(0, d.entries, d.row_ptr, d.target)
    return hs, grp


def snap(drv, rule, n):
    """(w0, w, v, state tables ...) of a group or a handle, every state row by global id"""
    w0, w, v = drv.get_params()
    ids = np.arange(n, dtype=np.uint32)
    st = {"ftrl": drv.ftrl_state_rows, "adagrad": drv.adapt_state_rows, None: lambda _: ()}[rule](ids)
    return (np.array([w0]), w, v) + tuple(st)


def data(path):
    with open(path, "rb") as f:
        return f.read()


def info_fields(i):
    return (i.version, i.session, i.num_attribute, i.num_factor, i.k0, i.k1, i.flags, i.state_rows, i.bytes)


def no_session_on_any_member(capi, grp):
    """neither kind of session is open on any member: a begin of either kind is refused while a member holds the other kind"""
    assert TC.open_rule(capi, grp) is None
    grp.adapt_begin("adagrad", **TC.ADAGRAD)
    grp.adapt_end()
    grp.ftrl_begin(**PARITY)
    grp.ftrl_end()


# ---- 1. the group writes the unsharded handle's file ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle_files(capi, tmp_path_factory):
    """rule -> (model, the handle's bits, its sparse file, its dense file) after two epochs on the sparse data case"""
    out = {}
    d, m = sparse_case(8)
    base = tmp_path_factory.mktemp("handle_files")
    for rule in ("ftrl", "adagrad"):
        a = TC.new_handle(capi, m, d)
        try:
            TC.begin(a, rule)
            TC.epoch(a, rule)
            TC.epoch(a, rule)
            sparse, dense = str(base / (rule + "_sparse.ckpt")), str(base / (rule + "_dense.ckpt"))
            a.checkpoint_save(sparse)
            a.checkpoint_save(dense, dense=True)
            out[rule] = (m, TC.snapshot(a, rule), sparse, dense)
        finally:
            a.close()
    return out


@pytest.mark.parametrize("world, shard_hash", WORLDS)
@pytest.mark.parametrize("rule", ["ftrl", "adagrad"])
def test_the_group_writes_the_handles_file(capi, tmp_path, handle_files, rule, world, shard_hash):
    from libfm_amd import checkpoint as ck
    m, want, a_sparse, a_dense = handle_files[rule]
    for src in (a_sparse, a_dense):
        hs, grp = group(capi, TC.other_model(m), world, shard_hash)
        try:
            assert TC.open_rule(capi, grp) is None
            got = grp.checkpoint_load(src)
            assert info_fields(got) == info_fields(capi.checkpoint_info(src))
            assert TC.open_rule(capi, grp) == rule
            assert TC.same(want, snap(grp, rule, N)), src
            b_sparse, b_dense = str(tmp_path / "b_sparse.ckpt"), str(tmp_path / "b_dense.ckpt")
            si = grp.checkpoint_save(b_sparse)
            di = grp.checkpoint_save(b_dense, dense=True)
            assert TC.same(want, snap(grp, rule, N))             # (a save changes nothing)
        finally:
            close(hs, grp)
        assert data(b_sparse) == data(a_sparse) and data(b_dense) == data(a_dense), src
        assert not os.path.exists(b_sparse + ".tmp") and not os.path.exists(b_dense + ".tmp")
        assert info_fields(si) == info_fields(capi.checkpoint_info(a_sparse)) and info_fields(di) == info_fields(capi.checkpoint_info(a_dense))
        assert info_fields(capi.checkpoint_info(b_sparse)) == info_fields(capi.checkpoint_info(a_sparse))
        assert 0 < si.state_rows < N and di.state_rows == N
    # libfm_amd/checkpoint.py reads and writes the group's file as it is
    for b in (b_sparse, b_dense):
        py = str(tmp_path / "py.ckpt")
        ck.write(py, ck.read(b))
        assert data(py) == data(b)


# ---- 2. resume is exact on shards ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k0k1", [(True, True), (False, False)], ids=["k0k1", "nok0k1"])
@pytest.mark.parametrize("k", [0, 3, 20, 64])
@pytest.mark.parametrize("rule", ["ftrl", "adagrad"])
def test_resume_is_exact_on_shards(capi, tmp_path, rule, k, k0k1):
    """A trains two epochs; B trains one, saves and is destroyed; C -- other parameters, no session -- loads and trains one more: A and
    C hold the same bits, and their files are byte-identical"""
    d, m = parity_case(k, *k0k1)
    mid, fa, fc = (str(tmp_path / x) for x in ("mid.ckpt", "a.ckpt", "c.ckpt"))
    hs, a = group(capi, m, 3, 1, d)
    try:
        TC.begin(a, rule)
        TC.epoch(a, rule)
        TC.epoch(a, rule)
        want = snap(a, rule, N)
        a.checkpoint_save(fa)
    finally:
        close(hs, a)
    hs, b = group(capi, m, 3, 1, d)
    try:
        TC.begin(b, rule)
        TC.epoch(b, rule)
        info = b.checkpoint_save(mid)
    finally:
        close(hs, b)
    assert info.session == SESSION[rule] and info.bytes == os.path.getsize(mid) and info.state_rows < N
    hs, c = group(capi, TC.other_model(m), 3, 1, d)
    try:
        c.checkpoint_load(mid)
        assert TC.open_rule(capi, c) == rule
        TC.epoch(c, rule)
        have = snap(c, rule, N)
        c.checkpoint_save(fc)
    finally:
        close(hs, c)
    assert want[0][0] == have[0][0] and TC.same(want, have)
    empty = k == 0 and not k0k1[1]                               # (neither factors nor linear weights: nothing is trained)
    assert data(fa) == data(fc) and (data(fa) != data(mid)) != empty


# ---- 3. resharding -------------------------------------------------------------------------------------------------------------
def test_resharding_and_the_serving_route(capi, tmp_path):
    """a file of W = 3 hashed loads into W = 2 unhashed and into one unsharded handle: the same bits everywhere, byte-identical files
    from all three, and the handle goes on to an int8 serving snapshot"""
    d, m = parity_case(8)
    f3, f2, f1 = (str(tmp_path / x) for x in ("w3.ckpt", "w2.ckpt", "w1.ckpt"))
    hs, g3 = group(capi, m, 3, 1, d)
    try:
        TC.begin(g3, "ftrl")
        TC.epoch(g3, "ftrl")
        want = snap(g3, "ftrl", N)
        g3.checkpoint_save(f3)
    finally:
        close(hs, g3)
    hs, g2 = group(capi, TC.other_model(m), 2, 0, d)
    try:
        g2.checkpoint_load(f3)
        assert TC.same(want, snap(g2, "ftrl", N))
        g2.checkpoint_save(f2)
    finally:
        close(hs, g2)
    h = TC.new_handle(capi, TC.other_model(m), d)
    try:
        h.checkpoint_load(f3)
        assert TC.same(want, TC.snapshot(h, "ftrl"))
        h.checkpoint_save(f1)
        h.compact_begin(format=capi.COMPACT_INT8)
        served, live = h.compact_predict(0, d.n_rows), h.predict(0, d.n_rows)
        assert served.shape == live.shape and np.isfinite(served).all() and not np.array_equal(served, np.zeros_like(served))
        h.compact_end()
    finally:
        h.close()
    assert data(f3) == data(f2) == data(f1)


# ---- 4. kernel edges -----------------------------------------------------------------------------------------------------------
def edge_record(rule, n, k, ids, seed):
    """a record with random parameters and random state rows (every row, or the rows `ids`) and the session's expected constants"""
    rng = np.random.default_rng(seed)
    rows = n if ids is None else len(ids)
    tabs = {"n": (rng.random((rows, 1 + k)) + 0.5).astype(np.float32)}
    if rule == "ftrl":
        tabs["z"] = rng.standard_normal((rows, 1 + k)).astype(np.float32)
    return dict(num_attribute=n, num_factor=k, k0=1, k1=1, session=SESSION[rule], flags=1 if ids is None else 0,
                consts=TC.expected_consts(rule), w0=float(rng.standard_normal()), w=rng.standard_normal(n).astype(np.float32),
                v=rng.standard_normal((n, k)).astype(np.float32), state_ids=ids, state=tabs)


def edge_model(n, k):
    m = O.Model(n, k, True, True, 0.01, 0.002, 0.001)
    m.v[:] = O.init_values(1, n, max(k, 1), 0.05)[:k]
    m.w[:] = O.init_values(2, n, 1, 0.02)[0]
    m.w0 = 0.03
    return m


@pytest.mark.parametrize("rule", ["ftrl", "adagrad"])
@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_kernel_edges(capi, tmp_path, name, rule):
    """files written by the numpy restatement with random rows: the group loads them to the record's bits and writes them back byte
    for byte, dense and sparse.  (A random state row differs from the start state, an unlisted one is the start state: the sparse
    criterion picks the listed ids again.)  The property that makes each case an edge is asserted first."""
    from libfm_amd import checkpoint as ck
    n, k, world, shard_hash = EDGE_CASES[name]
    owner, _ = capi.shard_place(n, world, shard_hash, np.arange(n, dtype=np.uint32))
    props = edge_properties(name, n, k, world, owner)
    assert all(props.values()), props
    ids = edge_ids(name, n, world, owner)
    for chosen in (None, ids):
        rec = edge_record(rule, n, k, chosen, 5 + n + k)
        py, out = str(tmp_path / "py.ckpt"), str(tmp_path / "out.ckpt")
        ck.write(py, rec)
        hs, grp = group(capi, edge_model(n, k), world, shard_hash)
        try:
            info = grp.checkpoint_load(py)
            assert info.state_rows == (n if chosen is None else len(chosen))
            got = snap(grp, rule, n)
            assert got[0][0] == rec["w0"]
            assert np.array_equal(bits(got[1].astype(np.float32)), bits(rec["w"]))
            assert np.array_equal(bits(got[2].T.astype(np.float32)), bits(rec["v"]))
            sel = np.arange(n) if chosen is None else chosen
            for i, tab in enumerate(("z", "n") if rule == "ftrl" else ("n",)):
                lin, fac = got[3 + 2 * i], got[4 + 2 * i]
                assert np.array_equal(bits(lin[sel].astype(np.float32)), bits(rec["state"][tab][:, 0])), tab
                assert np.array_equal(bits(fac.T[sel].astype(np.float32)), bits(rec["state"][tab][:, 1:])), tab
            grp.checkpoint_save(out, dense=chosen is None)
        finally:
            close(hs, grp)
        assert data(out) == data(py), (name, chosen is None)


def test_no_member_owns_nothing(capi):
    """n = 5 at W = 8 -- members that own nothing -- cannot be built: fmx_create refuses more shards than features, so the smallest
    share a member can hold is the one row of the n = 9, W = 8 cases above"""
    c, t = TC.code(capi, capi.Handle, 5, 2, shard_rank=0, shard_world=8, shard_hash=1)
    assert c == E_ARG and "more feature shards than features" in t


@pytest.mark.parametrize("rule", ["ftrl", "adagrad"])
def test_a_sparse_file_without_rows(capi, tmp_path, rule):
    """begin, then save without an epoch: state_rows is 0, the file is the unsharded handle's, and it loads"""
    n, k, world, shard_hash = EDGE_CASES["n9_w8"]
    m = edge_model(n, k)
    fg, fh = str(tmp_path / "g.ckpt"), str(tmp_path / "h.ckpt")
    h = capi.Handle(n, k, True, True, 1, m.reg0, m.regw, m.regv, LR, -1.0, 1.0)
    try:
        h.set_params(m.w0, m.w, m.v)
        TC.begin(h, rule)
        want = snap(h, rule, n)
        assert h.checkpoint_save(fh).state_rows == 0
    finally:
        h.close()
    hs, grp = group(capi, m, world, shard_hash)
    try:
        TC.begin(grp, rule)
        info = grp.checkpoint_save(fg)
        assert (info.session, info.state_rows) == (SESSION[rule], 0)
    finally:
        close(hs, grp)
    assert data(fg) == data(fh)
    hs, grp = group(capi, m, 3, 1)
    try:
        grp.set_params(0.5, m.w * 2.0, m.v * 2.0)
        grp.checkpoint_load(fg)
        assert TC.same(want, snap(grp, rule, n))
    finally:
        close(hs, grp)


def test_multi_chunk_sections(capi, tmp_path):
    """n = 70 001, k = 64, FTRL, dense, W = 3 hashed: V is 17.9 MB and z / n are 18.2 MB each -- two 16 MiB chunks, the second with an
    odd row count.  The group's file loads into a fresh group to the same bits and into a handle whose own save is the same bytes."""
    n, k, world, shard_hash = MULTI_CHUNK
    assert n * k * 4 > (16 << 20) and n * (k + 1) * 4 > (16 << 20)
    per_v, per_s = ((16 << 20) // (k * 4)) & ~1, ((16 << 20) // ((k + 1) * 4)) & ~1
    assert per_v < n < 2 * per_v and per_s < n < 2 * per_s and (n - per_v) % 2 == 1 and (n - per_s) % 2 == 1
    d = O.synth_rows(7, 0, 256, 32, n)
    m = O.Model(n, k, True, True, 0.01, 0.002, 0.001)
    m.v[:] = O.init_values(1, n, k, 0.05)
    m.w[:] = O.init_values(2, n, 1, 0.02)[0]
    m.w0 = 0.03
    fg, fh = str(tmp_path / "g.ckpt"), str(tmp_path / "h.ckpt")
    hs, grp = group(capi, m, world, shard_hash, d)
    try:
        TC.begin(grp, "ftrl")
        TC.epoch(grp, "ftrl")
        want = snap(grp, "ftrl", n)
        info = grp.checkpoint_save(fg, dense=True)
        assert info.state_rows == n and info.bytes == os.path.getsize(fg)
    finally:
        close(hs, grp)
    m2 = m.copy()
    m2.v[:] *= -1.0
    m2.w[:] += 1.0
    hs, grp = group(capi, m2, world, shard_hash)
    try:
        grp.checkpoint_load(fg)
        assert TC.same(want, snap(grp, "ftrl", n))
    finally:
        close(hs, grp)
    h = capi.Handle(n, k, True, True, 1, m.reg0, m.regw, m.regv, LR, -1.0, 1.0)
    try:
        h.set_params(m2.w0, m2.w, m2.v)
        h.checkpoint_load(fg)
        h.checkpoint_save(fh, dense=True)
    finally:
        h.close()
    assert data(fg) == data(fh)


# ---- 5. flags ------------------------------------------------------------------------------------------------------------------
def test_flags_and_session_kinds(capi, tmp_path):
    from libfm_amd import checkpoint as ck
    d, m = parity_case(8)
    ftrl_file, model_file = str(tmp_path / "ftrl.ckpt"), str(tmp_path / "model.ckpt")
    hs, a = group(capi, m, 3, 1, d)
    try:
        TC.begin(a, "ftrl")
        TC.epoch(a, "ftrl")
        want = snap(a, "ftrl", N)
        a.checkpoint_save(ftrl_file)
        info = a.checkpoint_save(model_file, model_only=True)    # MODEL_ONLY on save: no session in the file with one open
        assert (info.session, info.state_rows, info.flags) == (0, 0, 2)
        rec = ck.read(model_file)
        assert rec["session"] == 0 and rec["state"] == {} and not rec["consts"].any()
    finally:
        close(hs, a)
    hs, g = group(capi, TC.other_model(m), 2, 1, d)
    try:
        # an FTRL file onto an open AdaGrad session: FTRL on every member (an AdaGrad begin is refused while a member holds FTRL ...)
        g.adapt_begin("adagrad", **TC.ADAGRAD)
        g.checkpoint_load(ftrl_file)
        assert TC.open_rule(capi, g) == "ftrl" and TC.same(want, snap(g, "ftrl", N))
        c, t = TC.code(capi, g.adapt_begin, "adagrad", **TC.ADAGRAD)
        assert c == E_STATE and "fmx_ftrl session is open" in t
        # a file without a session leaves the sessions alone
        TC.epoch(g, "ftrl")
        st = snap(g, "ftrl", N)[3:]
        g.checkpoint_load(model_file)
        assert TC.open_rule(capi, g) == "ftrl" and TC.same(st, snap(g, "ftrl", N)[3:]) and TC.same(want[:3], snap(g, None, N))
        # MODEL_ONLY on load: the file's parameters, every member's session state bit for bit
        g.set_params(m.w0, m.w, m.v)
        g.checkpoint_load(ftrl_file, model_only=True)
        assert TC.same(st, snap(g, "ftrl", N)[3:]) and TC.same(want[:3], snap(g, None, N))
    finally:
        close(hs, g)


# ---- 6. refusals change nothing ------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(capi, tmp_path):
    d, m = parity_case(8)
    good, cut, bad = str(tmp_path / "good.ckpt"), str(tmp_path / "cut.ckpt"), str(tmp_path / "bad.ckpt")
    lib = capi.load()
    assert lib.fmx_group_checkpoint_save(None, os.fsencode(good), None, None) == E_ARG
    assert lib.fmx_group_checkpoint_load(None, os.fsencode(good), None, None) == E_ARG
    hs, g = group(capi, m, 3, 1, d)
    try:
        TC.begin(g, "ftrl")
        TC.epoch(g, "ftrl")
        g.checkpoint_save(good)
        TC.epoch(g, "ftrl")                                      # (the group has moved on: a load that went through would show)
        before = snap(g, "ftrl", N)
        # arguments
        for fn in (g.checkpoint_load, g.checkpoint_save):
            c, t = TC.code(capi, fn, None)
            assert c == E_ARG and "path is NULL" in t
        opts = capi.CkptOpts(4, 0)
        assert lib.fmx_group_checkpoint_load(g.g, os.fsencode(good), opts, None) == E_ARG and "unknown flags" in lib.fmx_group_last_error(g.g).decode()
        assert lib.fmx_group_checkpoint_save(g.g, os.fsencode(bad), opts, None) == E_ARG and not os.path.exists(bad)
        assert "unknown flags" in lib.fmx_group_last_error(g.g).decode()
        assert TC.code(capi, g.checkpoint_load, str(tmp_path / "no_such_file"))[0] == E_ARG
        c, t = TC.code(capi, g.checkpoint_save, str(tmp_path / "no_such_dir" / "x.ckpt"))
        assert c == E_ARG and "cannot create" in t
        # the header-level corruptions: truncated, not a checkpoint, bad magic, a version from the future, a header checksum
        blob = data(good)
        future = bytearray(blob)
        struct.pack_into("<I", future, 8, 2)
        flipped = bytearray(blob)
        flipped[100] ^= 0x04
        for cand, text in ((blob[:-1], "truncated"), (blob[:200], "shorter than a checkpoint header"), (b"x" + blob[1:], "bad magic"),
                           (bytes(future), "version"), (bytes(flipped), "checksum")):
            with open(cut, "wb") as f:
                f.write(cand)
            c, t = TC.code(capi, g.checkpoint_load, cut)
            assert c == E_ARG and text in t, (text, t)
            assert TC.code(capi, capi.checkpoint_info, cut) == (c, t.split(": ", 2)[2])      # (the per-handle load's message shape)
        assert TC.same(before, snap(g, "ftrl", N)) and TC.open_rule(capi, g) == "ftrl"
        TC.epoch(g, "ftrl")                                      # (the group still trains)
    finally:
        close(hs, g)
    assert sorted(os.listdir(tmp_path)) == ["cut.ckpt", "good.ckpt"]
    # a geometry mismatch in each field, against the group's GLOBAL geometry
    for field, kw, text in (("num_attribute", dict(n=N + 1), "num_attribute is 6400 in the file and 6401 on the group"),
                            ("num_factor", dict(k=7), "num_factor is 8 in the file and 7 on the group"),
                            ("k0", dict(k0=False), "k0 is 1 in the file and 0 on the group"),
                            ("k1", dict(k1=False), "k1 is 1 in the file and 0 on the group")):
        mm = O.Model(kw.get("n", N), kw.get("k", 8), kw.get("k0", True), kw.get("k1", True), 0.01, 0.002, 0.001)
        mm.v[:] = O.init_values(1, mm.n, mm.k, 0.05)
        hs, g = group(capi, mm, 2, 1)
        try:
            TC.begin(g, "ftrl")
            was = snap(g, "ftrl", mm.n)
            c, t = TC.code(capi, g.checkpoint_load, good)
            assert c == E_ARG and text in t, (field, t)
            assert TC.same(was, snap(g, "ftrl", mm.n))
        finally:
            close(hs, g)
    # an open ALS session on the group
    hs, g = group(capi, TC.other_model(m), 2, 1, d)
    try:
        g.als_begin(0)
        was = snap(g, None, N)
        c, t = TC.code(capi, g.checkpoint_load, good)
        assert c == E_STATE and "ALS" in t and "shard 0" in t
        assert TC.same(was, snap(g, None, N))
        g.als_end()
        g.checkpoint_load(good)
        TC.epoch(g, "ftrl")
    finally:
        close(hs, g)


# ---- 7. streaming failures -----------------------------------------------------------------------------------------------------
def patch_ids(src, dst, change, ck):
    """a copy of a sparse file whose id list is change(ids), with the section's and the header's checksums made right again"""
    blob = bytearray(data(src))
    head = ck.read_header(bytes(blob))
    at, (kind, off, nbytes, _) = [(i, s) for i, s in enumerate(head["sections"]) if s[0] == ck.SEC_IDS][0]
    ids = change(np.frombuffer(bytes(blob[off:off + nbytes]), dtype="<u4").copy())
    blob[off:off + nbytes] = ids.astype("<u4").tobytes()
    struct.pack_into("<Q", blob, 88 + 32 * at + 24, ck.checksum(blob[off:off + nbytes]))
    struct.pack_into("<Q", blob, 280, ck.checksum(blob[:280]))
    with open(dst, "wb") as f:
        f.write(bytes(blob))


def descending_pair(ids):
    mid = len(ids) // 2
    ids[mid], ids[mid + 1] = ids[mid + 1], ids[mid]
    return ids


def id_beyond_n(ids):
    ids[-1] = N
    return ids


def test_streaming_failures_close_every_session(capi, tmp_path):
    """a flipped body byte, and id lists with right checksums that are not ascending or name an id >= n: FMX_E_ARG naming the section,
    no session left on any member, the group usable.  These are error returns: the bad id never becomes an address."""
    from libfm_amd import checkpoint as ck
    d, m = parity_case(8)
    good, bad = str(tmp_path / "good.ckpt"), str(tmp_path / "bad.ckpt")
    hs, g = group(capi, m, 3, 1, d)
    try:
        TC.begin(g, "ftrl")
        TC.epoch(g, "ftrl")
        g.checkpoint_save(good)
        want = snap(g, "ftrl", N)
    finally:
        close(hs, g)
    assert len(ck.read(good)["state_ids"]) > 4
    cases = [(lambda: TC.corrupt(good, bad, ck.SEC_V, ck), "'V'", "checksum mismatch"),
             (lambda: TC.corrupt(good, bad, ck.SEC_N, ck), "'state n'", "checksum mismatch"),
             (lambda: TC.corrupt(good, bad, ck.SEC_IDS, ck), "'state ids'", ""),
             (lambda: patch_ids(good, bad, descending_pair, ck), "'state ids'", "not strictly ascending"),
             (lambda: patch_ids(good, bad, id_beyond_n, ck), "'state ids'", "not below num_attribute")]
    for make, name, text in cases:
        make()
        if text and "checksum" not in text:
            ck.read_header(data(bad))                            # (the header is a good one: only the list is wrong)
        hs, g = group(capi, TC.other_model(m), 3, 1, d)
        try:
            g.adapt_begin("adagrad", **TC.ADAGRAD)
            c, t = TC.code(capi, g.checkpoint_load, bad)
            assert c == E_ARG and name in t and text in t and "unspecified" in t and "closed" in t, t
            no_session_on_any_member(capi, g)
            g.set_params(m.w0, m.w, m.v)                         # (the group stays usable)
            TC.begin(g, "ftrl")
            TC.epoch(g, "ftrl")
            g.checkpoint_load(good)
            assert TC.same(want, snap(g, "ftrl", N))
        finally:
            close(hs, g)


# ---- 8. a one-member group -----------------------------------------------------------------------------------------------------
def test_one_member_group_and_the_per_handle_refusal(capi, tmp_path):
    d, m = sparse_case(8)
    fh, fg = str(tmp_path / "h.ckpt"), str(tmp_path / "g.ckpt")
    h = TC.new_handle(capi, m, d)
    try:
        TC.begin(h, "ftrl")
        TC.epoch(h, "ftrl")
        want = TC.snapshot(h, "ftrl")
        h.checkpoint_save(fh)
    finally:
        h.close()
    h = TC.new_handle(capi, TC.other_model(m), d)
    g = capi.Group([h])
    try:
        g.checkpoint_load(fh)
        assert TC.same(want, snap(g, "ftrl", N))                 # (a member's state is read through its group)
        g.checkpoint_save(fg)
        c, t = TC.code(capi, g.checkpoint_load, str(tmp_path / "no_such_file"))
        assert c == E_ARG and "fmx_group_checkpoint_load" in t
    finally:
        close([h], g)
    assert data(fh) == data(fg)
    hs, g = group(capi, m, 2, 0)
    try:
        for fn in (hs[1].checkpoint_save, hs[1].checkpoint_load):
            c, t = TC.code(capi, fn, fh)
            assert c == E_UNSUPPORTED and "feature shards" in t
    finally:
        close(hs, g)


# ---- 9. the learner ------------------------------------------------------------------------------------------------------------
def test_unsharded_learner_continues_from_a_groups_file(capi, tmp_path):
    """FMLearnSGD(optimizer="ftrl").load_checkpoint of a file a capi.Group wrote: its first epoch is, bit for bit, the epoch of an
    unsharded handle loaded from the same file"""
    from libfm_amd import learner as L
    d, m = parity_case(8)
    path = str(tmp_path / "g.ckpt")
    hs, g = group(capi, m, 3, 1, d)
    try:
        g.ftrl_begin(alpha=0.05, l1_w=0.01, l1_v=0.002, init_acc=0.25)
        g.ftrl_epoch(0, TC.BATCH, 0)
        g.checkpoint_save(path)
    finally:
        close(hs, g)
    l = L.FMLearnSGD()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor, l.fm.regv = m.n, m.k, 0.01
    l.fm.w0, l.fm.w, l.fm.v = 0.0, np.zeros(m.n), np.zeros((m.k, m.n))
    l.task, l.learn_rate, l.batch, l.num_iter, l.min_target, l.max_target = 1, 0.05, TC.BATCH, 1, -1.0, 1.0
    l.out = io.StringIO()
    l.optimizer = "ftrl"
    l.init()
    assert l.load_checkpoint(path).session == 2
    ld = L.Data(d.entries, d.row_ptr, np.where(d.target > 0, 1.0, -1.0))
    l.learn(ld, ld)
    have = TC.snapshot(l._h, "ftrl")
    fm = l.fm
    l.close()
    h = capi.Handle(m.n, m.k, fm.k0, fm.k1, 1, fm.reg0, fm.regw, fm.regv, 0.05, -1.0, 1.0)
    try:
        h.upload_rows(0, d.entries, d.row_ptr, np.where(d.target > 0, 1.0, -1.0).astype(np.float32))
        h.checkpoint_load(path)
        h.ftrl_epoch(0, TC.BATCH, 0)
        want = TC.snapshot(h, "ftrl")
    finally:
        h.close()
    assert TC.same(want, have)


# ---- 10. two distinct devices ----------------------------------------------------------------------------------------------------
def test_two_devices(capi, tmp_path):
    """one shard per device (the staging buffers cross between devices; no kernel reads another device's table): the handle's file
    loads to the handle's bits and is written back byte for byte"""
    if capi.load().fmx_device_count() < 2:
        pytest.skip("needs two devices")
    d, m = sparse_case(8)
    fh, fg = str(tmp_path / "h.ckpt"), str(tmp_path / "g.ckpt")
    h = TC.new_handle(capi, m, d)
    try:
        TC.begin(h, "ftrl")
        TC.epoch(h, "ftrl")
        want = TC.snapshot(h, "ftrl")
        h.checkpoint_save(fh)
    finally:
        h.close()
    hs, g = make_group(capi, 2, [0, 1], TC.other_model(m), 1, LR, -1.0, 1.0, 1)
    try:
        g.checkpoint_load(fh)
        assert TC.same(want, snap(g, "ftrl", N))
        g.checkpoint_save(fg)
    finally:
        close(hs, g)
    assert data(fh) == data(fg)
