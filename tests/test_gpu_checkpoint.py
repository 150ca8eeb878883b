"""GPU: exact binary checkpoints of the model and of an open AdaGrad / FTRL session (fmx_checkpoint_save / _load / _info,
csrc/fmx_ckpt.hip and fmx_ckpt_kernels.h) -- resume is exact, sparse and dense state load to the same bits,
the file is what libfm_amd/checkpoint.py writes, the device reads what Python wrote, refusals change nothing, session kinds and
flags, and the command line.  The shapes are tests/test_gpu_ftrl.py's parity size (n = 6400, 512 rows of 32 entries, batch 64,
micro-chunk 16); the sparse files come from test_checkpoint_cpu.sparse_case.  No tolerance appears anywhere: every comparison is of
bits (the float64 arrays the library hands out hold fp32 values; they are compared as 64-bit patterns, so -0 is not +0) or bytes."""
import contextlib
import io
import os

import numpy as np
import pytest

from test_checkpoint_cpu import bits, sparse_case
from test_ftrl_cpu import PARITY, parity_case

pytestmark = pytest.mark.gpu

N = 6400
LR, BATCH, CHUNK = 0.01, 64, 16
ADAGRAD = dict(init_acc=0.5, learn_rate=0.05)
WIDTHS = (0, 3, 8, 20, 64)                   # every row-stride rule (1, 4, 8, 32, 64 floats) and the table without factors


def new_handle(capi, m, d=None, **kw):
    h = capi.Handle(m.n, m.k, m.k0, m.k1, 1, m.reg0, m.regw, m.regv, LR, -1.0, 1.0, **kw)
    h.set_params(m.w0, m.w, m.v)
    if d is not None:
        h.upload_rows(0, d.entries, d.row_ptr, d.target)
    return h


def other_model(m):
    """a model of the same geometry with different parameters (w only with k1: without it the file holds no w)"""
    from oracle import oracle as O
    c = m.copy()
    c.v[:] = O.init_values(11, m.n, m.k, 0.08)
    if m.k1:
        c.w[:] = O.init_values(12, m.n, 1, 0.03)[0]
    c.w0 = -0.2
    return c


def begin(h, rule):
    if rule == "ftrl":
        h.ftrl_begin(**PARITY)
    elif rule == "adagrad":
        h.adapt_begin("adagrad", **ADAGRAD)


def epoch(h, rule):
    return {"ftrl": h.ftrl_epoch, "adagrad": h.adapt_epoch}[rule](0, BATCH, CHUNK)


def state(h, rule):
    ids = np.arange(h.n, dtype=np.uint32)
    return {"ftrl": h.ftrl_state_rows, "adagrad": h.adapt_state_rows, None: lambda _: ()}[rule](ids)


def snapshot(h, rule):
    w0, w, v = h.get_params()
    return (np.array([w0]), w, v) + tuple(state(h, rule))


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def open_rule(capi, h):
    """which session the handle has open, asked of the library"""
    out = []
    for rule, fn in (("adagrad", h.adapt_state_rows), ("ftrl", h.ftrl_state_rows)):
        try:
            fn(np.zeros(1, dtype=np.uint32))
            out.append(rule)
        except capi.FmxError as e:
            assert e.code == -3
    assert len(out) <= 1
    return out[0] if out else None


def code(capi, fn, *a, **kw):
    with pytest.raises(capi.FmxError) as ei:
        fn(*a, **kw)
    return ei.value.code, ei.value.text


# ---- 1. resume is exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k0k1", [(True, True), (False, False)], ids=["k0k1", "nok0k1"])
@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("rule", ["ftrl", "adagrad"])
def test_resume_is_exact(tmp_path, rule, k, k0k1):
    """A trains two epochs; B trains one, saves and is destroyed; C starts from other parameters without a session, loads and trains
    one: A and C hold the same bits in w0, w, V and every state row"""
    from libfm_amd import capi
    d, m = parity_case(k, *k0k1)
    path = str(tmp_path / "b.ckpt")
    a = new_handle(capi, m, d)
    try:
        begin(a, rule)
        epoch(a, rule)
        epoch(a, rule)
        want = snapshot(a, rule)
    finally:
        a.close()
    b = new_handle(capi, m, d)
    try:
        begin(b, rule)
        epoch(b, rule)
        info = b.checkpoint_save(path)
    finally:
        b.close()
    empty = k == 0 and not k0k1[1]                               # (neither factors nor linear weights: nothing is trained but the bias)
    assert info.session == {"adagrad": 1, "ftrl": 2}[rule] and info.bytes == os.path.getsize(path)
    assert info.state_rows < N and (info.state_rows > 0) != empty
    c = new_handle(capi, other_model(m), d)
    try:
        assert open_rule(capi, c) is None
        got = c.checkpoint_load(path)
        assert (got.session, got.state_rows, got.bytes) == (info.session, info.state_rows, info.bytes)
        assert open_rule(capi, c) == rule
        epoch(c, rule)
        have = snapshot(c, rule)
    finally:
        c.close()
    assert want[0][0] == have[0][0]                              # w0
    assert same(want, have)
    assert same(want[1:3], snapshot_of_model(m)[1:3]) == empty   # (the epochs moved the parameters)


def snapshot_of_model(m):
    return (np.array([m.w0]), m.w.astype(np.float32).astype(np.float64), m.v.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("rule", ["ftrl", "adagrad"])
def test_resume_is_exact_through_a_pair_epoch(tmp_path, rule):
    """one pointwise and one stored-pair epoch (fmx_ftrl_pair_epoch / fmx_adapt_pair_epoch) on each side of the file"""
    from libfm_amd import capi
    d, m = parity_case(8)
    rng = np.random.default_rng(5)
    pa = rng.integers(0, d.n_rows, 700).astype(np.uint32)
    pb = ((pa + 1 + rng.integers(0, d.n_rows - 1, 700)) % d.n_rows).astype(np.uint32)
    path = str(tmp_path / "b.ckpt")

    def both(h):
        epoch(h, rule)
        {"ftrl": h.ftrl_pair_epoch, "adagrad": h.adapt_pair_epoch}[rule](0, BATCH)
    a = new_handle(capi, m, d)
    try:
        a.upload_pairs(0, pa, pb)
        begin(a, rule)
        both(a)
        both(a)
        want = snapshot(a, rule)
    finally:
        a.close()
    b = new_handle(capi, m, d)
    try:
        b.upload_pairs(0, pa, pb)
        begin(b, rule)
        both(b)
        b.checkpoint_save(path)
    finally:
        b.close()
    c = new_handle(capi, other_model(m), d)
    try:
        c.upload_pairs(0, pa, pb)
        c.checkpoint_load(path)
        both(c)
        have = snapshot(c, rule)
    finally:
        c.close()
    assert want[0][0] == have[0][0] and same(want, have)


@pytest.mark.parametrize("k", WIDTHS)
def test_model_only_load_reproduces_the_parameters(tmp_path, k):
    """a handle without a session: load reproduces w0, w and V bit for bit (plain fmx_sgd_epoch makes no promise to continue alike)"""
    from libfm_amd import capi
    d, m = parity_case(k)
    path = str(tmp_path / "m.ckpt")
    a = new_handle(capi, m, d)
    try:
        a.sgd_epoch(0, capi.SGD_MINIBATCH, batch=BATCH)
        want = snapshot(a, None)
        info = a.checkpoint_save(path)
    finally:
        a.close()
    assert (info.session, info.state_rows) == (0, 0)
    c = new_handle(capi, other_model(m))
    try:
        c.checkpoint_load(path)
        assert same(want, snapshot(c, None)) and open_rule(capi, c) is None
    finally:
        c.close()


# ---- 2. sparse against dense, 3. the file against the restatement ---------------------------------------------------------------
def expected_consts(rule):
    """the session's fp32 constants as fmx_*_begin forms them from the doubles"""
    c = np.zeros(8, dtype=np.float32)
    if rule == "ftrl":
        c[:7] = [np.float32(1.0) / np.float32(PARITY["alpha"]), PARITY["beta"], PARITY["l1_w"], PARITY["l1_v"], PARITY["l2_w"], PARITY["l2_v"], 0.0]
    else:
        c[:2] = [ADAGRAD["learn_rate"], ADAGRAD["init_acc"]]
    return c


def record_of(h, m, rule, snap, ids):
    """the checkpoint record of a handle's snapshot: every state row (ids None: dense) or the rows `ids`"""
    rec = dict(num_attribute=m.n, num_factor=m.k, k0=int(m.k0), k1=int(m.k1), session={"ftrl": 2, "adagrad": 1}[rule],
               flags=1 if ids is None else 0, consts=expected_consts(rule), w0=float(snap[0][0]),
               w=snap[1].astype(np.float32) if m.k1 else None, v=snap[2].T.astype(np.float32), state_ids=ids, state={})
    rows = slice(None) if ids is None else ids
    tabs = dict(zip(("z", "n") if rule == "ftrl" else ("n",), zip(snap[3::2], snap[4::2])))
    for name, (lin, fac) in tabs.items():
        rec["state"][name] = np.concatenate([lin[rows, None], fac.T[rows]], axis=1).astype(np.float32)
    return rec


@pytest.mark.parametrize("rule", ["ftrl", "adagrad"])
def test_sparse_against_dense_and_the_restatement(tmp_path, rule):
    from libfm_amd import capi, checkpoint as ck
    d, m = sparse_case(8)
    in_data = np.unique(d.entries["id"])
    sparse, dense, again, py = (str(tmp_path / x) for x in ("sparse.ckpt", "dense.ckpt", "again.ckpt", "py.ckpt"))
    a = new_handle(capi, m, d)
    try:
        begin(a, rule)
        epoch(a, rule)
        epoch(a, rule)
        want = snapshot(a, rule)
        si = a.checkpoint_save(sparse)
        di = a.checkpoint_save(dense, dense=True)
        a.checkpoint_save(again)
        assert same(want, snapshot(a, rule))                     # (a save changes nothing)
    finally:
        a.close()
    print("%s: sparse %d rows, %d bytes; dense %d rows, %d bytes; %d features in the data" % (
        rule, si.state_rows, si.bytes, di.state_rows, di.bytes, len(in_data)))
    # 2. the sparse file holds rows, no more than the data touches, and only ids of the data; the dense one every row
    assert 0 < si.state_rows <= len(in_data) and di.state_rows == N and si.bytes < di.bytes
    srec, drec = ck.read(sparse), ck.read(dense)
    assert len(srec["state_ids"]) == si.state_rows and np.isin(srec["state_ids"], in_data).all()
    assert drec["state_ids"] is None and (srec["flags"], drec["flags"]) == (0, 1)
    info = capi.checkpoint_info(sparse)
    assert (info.version, info.session, info.num_attribute, info.num_factor, info.k0, info.k1, info.flags, info.state_rows, info.bytes) == (
        1, si.session, N, 8, 1, 1, 0, si.state_rows, os.path.getsize(sparse))
    for path in (sparse, dense):                                 # two fresh handles, one file each: the saving handle's bits
        c = new_handle(capi, other_model(m))
        try:
            c.checkpoint_load(path)
            assert same(want, snapshot(c, rule)), path
        finally:
            c.close()
    # 3. the file is the restatement's: read() gives the handle's arrays, write() of them gives the file's bytes; saves repeat
    with open(sparse, "rb") as f1, open(again, "rb") as f2:
        sparse_bytes = f1.read()
        assert sparse_bytes == f2.read()
    for path, rec, ids in ((sparse, srec, srec["state_ids"]), (dense, drec, None)):
        mine = record_of(None, m, rule, want, ids)
        assert np.array_equal(bits(rec["consts"]), bits(mine["consts"]))
        assert np.array_equal(bits(rec["w"]), bits(mine["w"])) and np.array_equal(bits(rec["v"]), bits(mine["v"]))
        assert np.float64(rec["w0"]).tobytes() == np.float64(mine["w0"]).tobytes()
        for name in mine["state"]:
            assert np.array_equal(bits(rec["state"][name]), bits(mine["state"][name])), (path, name)
        ck.write(py, mine)
        with open(path, "rb") as f1, open(py, "rb") as f2:
            assert f1.read() == f2.read(), path


# ---- 4. the device reads what Python wrote --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 3, 20])
@pytest.mark.parametrize("rule", ["ftrl", "adagrad"])
def test_the_device_reads_what_python_wrote(tmp_path, rule, k):
    from libfm_amd import capi, checkpoint as ck
    d, m = parity_case(k)
    rng = np.random.default_rng(3 + k)
    file_model = other_model(m)
    base = snapshot_of_model(file_model)
    ids = np.array([0, 1, 5, 63, 64, 65, 1000, 4097, N - 2, N - 1, 77], dtype=np.uint32)
    ids.sort()
    ref = new_handle(capi, file_model)                           # what set_params + begin give with the same constants
    try:
        begin(ref, rule)
        start = snapshot(ref, rule)
    finally:
        ref.close()
    for chosen in (None, ids):
        rows = N if chosen is None else len(chosen)
        tabs = {"n": (rng.random((rows, 1 + k)) + 0.5).astype(np.float32)}
        if rule == "ftrl":
            tabs["z"] = rng.standard_normal((rows, 1 + k)).astype(np.float32)
        rec = dict(num_attribute=N, num_factor=k, k0=1, k1=1, session={"ftrl": 2, "adagrad": 1}[rule], flags=1 if chosen is None else 0,
                   consts=expected_consts(rule), w0=file_model.w0, w=base[1].astype(np.float32), v=base[2].T.astype(np.float32),
                   state_ids=chosen, state=tabs)
        path = str(tmp_path / "py.ckpt")
        ck.write(path, rec)
        h = new_handle(capi, m)
        try:
            info = h.checkpoint_load(path)
            assert info.state_rows == rows and open_rule(capi, h) == rule
            got = snapshot(h, rule)
        finally:
            h.close()
        assert same(base, got[:3])
        sel = np.arange(N) if chosen is None else chosen
        rest = np.setdiff1d(np.arange(N), sel)
        for i, name in enumerate(("z", "n") if rule == "ftrl" else ("n",)):
            lin, fac = got[3 + 2 * i], got[4 + 2 * i]
            assert np.array_equal(bits(lin[sel].astype(np.float32)), bits(tabs[name][:, 0])), name
            assert np.array_equal(bits(fac.T[sel].astype(np.float32)), bits(tabs[name][:, 1:])), name
            # the rows that are not listed are the start state of the file's parameters
            assert np.array_equal(bits(lin[rest]), bits(start[3 + 2 * i][rest])) and np.array_equal(bits(fac[:, rest]), bits(start[4 + 2 * i][:, rest]))
        assert len(rest) == (0 if chosen is None else N - len(ids))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def corrupt(src, dst, kind, ck):
    """a copy of the file with one byte flipped in the middle of a section"""
    with open(src, "rb") as f:
        data = bytearray(f.read())
    off, nbytes = [(s[1], s[2]) for s in ck.read_header(bytes(data))["sections"] if s[0] == kind][0]
    data[off + nbytes // 2] ^= 0x04
    with open(dst, "wb") as f:
        f.write(bytes(data))


def test_refusals_change_nothing(tmp_path):
    from libfm_amd import capi, checkpoint as ck
    d, m = parity_case(8)
    good, cut, bad = str(tmp_path / "good.ckpt"), str(tmp_path / "cut.ckpt"), str(tmp_path / "bad.ckpt")
    a = new_handle(capi, m, d)
    try:
        begin(a, "ftrl")
        epoch(a, "ftrl")
        a.checkpoint_save(good)
        epoch(a, "ftrl")                                         # (the handle has moved on: a load that went through would show)
        before = snapshot(a, "ftrl")
        # arguments
        assert a.lib.fmx_checkpoint_load(a.h, None, None, None) == -1 and a.lib.fmx_checkpoint_save(a.h, None, None, None) == -1
        opts = capi.CkptOpts(4, 0)
        assert a.lib.fmx_checkpoint_load(a.h, os.fsencode(good), opts, None) == -1 and "unknown flags" in a.lib.fmx_last_error(a.h).decode()
        assert a.lib.fmx_checkpoint_save(a.h, os.fsencode(bad), opts, None) == -1 and not os.path.exists(bad)
        assert code(capi, a.checkpoint_load, str(tmp_path / "no_such_file"))[0] == -1
        # a truncated file, a file that is no checkpoint, a version from the future
        with open(good, "rb") as f:
            data = f.read()
        for blob, text in ((data[:-1], "truncated"), (data[:200], "shorter than a checkpoint header"), (b"x" + data[1:], "bad magic")):
            with open(cut, "wb") as f:
                f.write(blob)
            c, t = code(capi, a.checkpoint_load, cut)
            assert c == -1 and text in t
            assert code(capi, capi.checkpoint_info, cut) == (c, t.split(": ", 2)[2])
        assert same(before, snapshot(a, "ftrl")) and open_rule(capi, a) == "ftrl"
    finally:
        a.close()
    # a geometry mismatch in each field: the message names the field and both values
    for field, kw, text in (("num_attribute", dict(n=N + 1), "num_attribute is 6400 in the file and 6401 on the handle"),
                            ("num_factor", dict(k=7), "num_factor is 8 in the file and 7 on the handle"),
                            ("k0", dict(k0=False), "k0 is 1 in the file and 0 on the handle"),
                            ("k1", dict(k1=False), "k1 is 1 in the file and 0 on the handle")):
        h = capi.Handle(kw.get("n", N), kw.get("k", 8), kw.get("k0", True), kw.get("k1", True), 1, learn_rate=LR)
        try:
            h.init_params(0.0, 0.1, 3)
            h.ftrl_begin(**PARITY)
            was = snapshot(h, "ftrl")
            c, t = code(capi, h.checkpoint_load, good)
            assert c == -1 and text in t, field
            assert same(was, snapshot(h, "ftrl"))
        finally:
            h.close()
    # a flipped byte in V and in a state section: FMX_E_ARG naming the section, the session closed, a good load works afterwards
    want = None
    for kind, name in ((ck.SEC_V, "'V'"), (ck.SEC_N, "'state n'"), (ck.SEC_IDS, "'state ids'")):
        corrupt(good, bad, kind, ck)
        h = new_handle(capi, other_model(m), d)
        try:
            h.adapt_begin("adagrad", **ADAGRAD)
            c, t = code(capi, h.checkpoint_load, bad)
            assert c == -1 and name in t and "unspecified" in t and "closed" in t, t
            assert open_rule(capi, h) is None
            h.set_params(m.w0, m.w, m.v)                         # (the handle stays usable)
            h.checkpoint_load(good)
            assert open_rule(capi, h) == "ftrl"
            got = snapshot(h, "ftrl")
            want = want or got
            assert same(want, got)
        finally:
            h.close()


def test_refusals_by_handle_kind_and_session(tmp_path):
    from libfm_amd import capi
    d, m = parity_case(3)
    good = str(tmp_path / "good.ckpt")
    a = new_handle(capi, m, d)
    try:
        a.checkpoint_save(good)
        # an SGDA session, an ALS session: FMX_E_STATE, nothing changes
        a.sgda_begin()
        was = snapshot(a, None)
        assert code(capi, a.checkpoint_load, good)[0] == -3
        assert same(was, snapshot(a, None))
        a.sgda_end()
        a.als_begin(0)
        was = snapshot(a, None)
        c, t = code(capi, a.checkpoint_load, good)
        assert c == -3 and "ALS" in t
        assert same(was, snapshot(a, None))
        a.als_end()
        a.checkpoint_load(good)
        # a directory that cannot be written to: FMX_E_ARG and no .tmp file left behind
        plain_file = tmp_path / "plain_file"
        plain_file.write_bytes(b"x")
        for target in (tmp_path / "no_such_dir" / "x.ckpt", plain_file / "x.ckpt"):
            c, t = code(capi, a.checkpoint_save, str(target))
            assert c == -1 and "cannot create" in t
        assert sorted(os.listdir(tmp_path)) == ["good.ckpt", "plain_file"]
    finally:
        a.close()
    hs = capi.Handle(100, 3, shard_rank=0, shard_world=2, learn_rate=LR)
    try:
        for fn in (hs.checkpoint_save, hs.checkpoint_load):
            c, t = code(capi, fn, good)
            assert c == -4 and "feature shards" in t
    finally:
        hs.close()


# ---- 6. session kinds and flags -----------------------------------------------------------------------------------------------
def test_session_kinds_and_flags(tmp_path):
    from libfm_amd import capi, checkpoint as ck
    d, m = parity_case(8)
    ftrl_file, model_file = str(tmp_path / "ftrl.ckpt"), str(tmp_path / "model.ckpt")
    a = new_handle(capi, m, d)
    try:
        begin(a, "ftrl")
        epoch(a, "ftrl")
        want = snapshot(a, "ftrl")
        a.checkpoint_save(ftrl_file)
        info = a.checkpoint_save(model_file, model_only=True)    # FMX_CKPT_MODEL_ONLY on save: a file without a session
        assert (info.session, info.state_rows, info.flags) == (0, 0, 2)
        rec = ck.read(model_file)
        assert rec["session"] == 0 and rec["state"] == {} and not rec["consts"].any()
    finally:
        a.close()
    h = new_handle(capi, other_model(m), d)
    try:
        # an FTRL file onto an open AdaGrad session: FTRL open, AdaGrad closed
        h.adapt_begin("adagrad", **ADAGRAD)
        h.checkpoint_load(ftrl_file)
        assert open_rule(capi, h) == "ftrl" and same(want, snapshot(h, "ftrl"))
        # a file without a session leaves the open session alone
        epoch(h, "ftrl")
        st = state(h, "ftrl")
        h.checkpoint_load(model_file)
        assert open_rule(capi, h) == "ftrl" and same(st, state(h, "ftrl")) and same(want[:3], snapshot(h, None))
        # FMX_CKPT_MODEL_ONLY on load: the parameters are the file's, the handle's session state stays bit for bit
        h.set_params(m.w0, m.w, m.v)
        h.checkpoint_load(ftrl_file, model_only=True)
        assert same(st, state(h, "ftrl")) and same(want[:3], snapshot(h, None))
        # a serving snapshot taken before a load is a frozen copy
        h.set_params(0.5, m.w * 2.0, m.v * 2.0)
        h.compact_begin()
        frozen, live = h.compact_predict(0, d.n_rows), h.predict(0, d.n_rows)
        h.checkpoint_load(ftrl_file)
        assert np.array_equal(bits(frozen), bits(h.compact_predict(0, d.n_rows))) and not np.array_equal(live, h.predict(0, d.n_rows))
        h.compact_end()
    finally:
        h.close()


# ---- the learners -----------------------------------------------------------------------------------------------------------
def test_learner_resumes_bit_for_bit(tmp_path):
    """FMLearnSGD.save_checkpoint / load_checkpoint: a learner that only names the file (optimizer left at its default) takes the
    file's optimizer and constants, init() and learn() do not begin the session again, and one more iteration ends on the bits of
    the uninterrupted run; load_checkpoint after init() does the same"""
    from libfm_amd import learner as L
    d, m = parity_case(8)
    data = L.Data(d.entries, d.row_ptr, np.where(d.target > 0, 1.0, -1.0))
    path = str(tmp_path / "l.ckpt")

    def learner(model, iters, configure=True):
        l = L.FMLearnSGD()
        l.fm = L.FMModel()
        l.fm.num_attribute, l.fm.num_factor, l.fm.regv = model.n, model.k, 0.01
        l.fm.w0, l.fm.w, l.fm.v = model.w0, model.w.copy(), model.v.copy()
        l.task, l.learn_rate, l.batch, l.num_iter, l.min_target, l.max_target = 1, 0.05, BATCH, iters, -1.0, 1.0
        l.out = io.StringIO()
        if configure:
            l.optimizer, l.l1_w, l.l1_v, l.init_acc = "ftrl", 0.01, 0.002, 0.25
        return l
    a = learner(m, 2)
    a.init()
    a.learn(data, data)
    want = snapshot(a._h, "ftrl")
    a.close()
    b = learner(m, 1)
    b.init()
    b.learn(data, data)
    info = b.save_checkpoint(path)
    b.close()
    assert info.session == 2 and info.state_rows > 0
    for after_init in (False, True):
        c = learner(other_model(m), 1, configure=False)
        if after_init:
            c.init()
            assert open_rule(L.capi, c._h) is None
            assert c.load_checkpoint(path).session == 2
        else:
            assert c.load_checkpoint(path) is None
            c.init()
        assert c.optimizer == "ftrl" and (c.l1_w, c.l1_v, c.init_acc) == (float(np.float32(0.01)), float(np.float32(0.002)), 0.25)
        assert open_rule(L.capi, c._h) == "ftrl"
        c.learn(data, data)
        have = snapshot(c._h, "ftrl")
        assert np.array_equal(c.fm.v, have[2])                   # (the host model follows the device)
        c.close()
        assert same(want, have), after_init


# ---- 7. the command line --------------------------------------------------------------------------------------------------------
def test_cli_resumes_byte_for_byte(tmp_path, oracle, capsys):
    from libfm_amd import cli
    d, _ = parity_case(8)
    trf = str(tmp_path / "train.libfm")
    oracle.Data(d.entries, d.row_ptr, np.where(d.target > 0, 1.0, 0.0).astype(np.float32)).write_libsvm(trf)
    a, b, c = (str(tmp_path / x) for x in "abc")
    common = ["-task", "c", "-train", trf, "-test", trf, "-dim", "1,1,8", "-method", "sgd", "-optimizer", "ftrl", "-learn_rate", "0.05",
              "-l1", "0.01,0.002", "-regular", "0,0.01,0.01", "-init_stdev", "0.05", "-seed", "7", "-batch", "64"]

    def run(extra):
        with contextlib.redirect_stdout(io.StringIO()):
            assert cli.main(common + extra) == 0
        err = capsys.readouterr().err
        assert "ERROR" not in err, err
        return err
    err = run(["-iter", "2", "-save_checkpoint", a])
    assert "checkpoint\tsave\tsession=ftrl\tstate_rows=" in err
    run(["-iter", "1", "-save_checkpoint", b])
    err = run(["-iter", "1", "-load_checkpoint", b, "-save_checkpoint", c])
    assert "checkpoint\tload\tsession=ftrl" in err and "checkpoint\tsave\tsession=ftrl" in err
    with open(a, "rb") as fa, open(b, "rb") as fb, open(c, "rb") as fc:
        da, db, dc = fa.read(), fb.read(), fc.read()
    assert da == dc and da != db
    assert cli.main(common + ["-iter", "1", "-load_checkpoint", b, "-load_model", a]) == 0
    assert "ERROR: -load_checkpoint replaces -load_model" in capsys.readouterr().err
    assert cli.main(common[:8] + ["-method", "als", "-save_checkpoint", a]) == 0
    assert "ERROR: -save_checkpoint / -load_checkpoint belong to -method sgd and -method bpr" in capsys.readouterr().err
