"""CPU: the numpy restatement of the binary checkpoint format (libfm_amd/checkpoint.py; the layout is csrc/fmx_ckpt_format.h and
DESIGN.md section 24) -- round trips, the checksum against a literal worked out here, everything the reader refuses -- the three
symbols in the header and the binding, and the property of the data case tests/test_gpu_checkpoint.py takes its sparse files from.
Every comparison is of bits or bytes."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from test_ftrl_cpu import parity_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTRL_CONSTS = [20.0, 1.0, 0.5, 0.3, 0.01, 0.02, 0.25, 0.0]
ADAGRAD_CONSTS = [0.05, 1.0, 0, 0, 0, 0, 0, 0]


def sparse_case(k, k0=True, k1=True):
    """the data and start model of the sparse-against-dense tests on the device: the parity case of tests/test_gpu_ftrl.py with 128
    rows, which leave a good part of the 6400 features untouched (test_sparse_case_property)"""
    return parity_case(k, k0, k1, rows=128)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def record(n, k, session, dense, k1=True, state_rows=None, seed=0):
    """a record with random contents; sparse: state_rows ids drawn from [0, n)"""
    from libfm_amd import checkpoint as ck
    rng = np.random.default_rng(seed + 1000 * k + n)
    rec = dict(num_attribute=n, num_factor=k, k0=1, k1=int(k1), session=session, flags=ck.DENSE_STATE if dense else 0,
               consts=np.array({0: [0] * 8, 1: ADAGRAD_CONSTS, 2: FTRL_CONSTS}[session], dtype=np.float32),
               w0=float(rng.standard_normal()), w=rng.standard_normal(n).astype(np.float32) if k1 else None,
               v=rng.standard_normal((n, k)).astype(np.float32), state_ids=None, state={})
    if session:
        rows = n if dense else state_rows
        if not dense:
            rec["state_ids"] = np.sort(rng.choice(n, size=rows, replace=False)).astype(np.uint32)
        rec["state"] = {"n": rng.random((rows, 1 + k)).astype(np.float32)}
        if session == 2:
            rec["state"]["z"] = rng.standard_normal((rows, 1 + k)).astype(np.float32)
    return rec


def assert_records_equal(a, b):
    for key in ("num_attribute", "num_factor", "k0", "k1", "session", "flags"):
        assert int(a[key]) == int(b[key]), key
    assert np.array_equal(bits(np.asarray(a["consts"], dtype=np.float32)), bits(np.asarray(b["consts"], dtype=np.float32)))
    assert struct.pack("<d", a["w0"]) == struct.pack("<d", b["w0"])
    for key in ("w", "v", "state_ids"):
        assert (a[key] is None) == (b[key] is None), key
        if a[key] is not None:
            assert a[key].shape == b[key].shape and np.array_equal(bits(a[key]), bits(b[key])), key
    assert sorted(a["state"]) == sorted(b["state"])
    for key in a["state"]:
        assert a["state"][key].shape == b["state"][key].shape and np.array_equal(bits(a["state"][key]), bits(b["state"][key])), key


CASES = [(n, k, session, dense, k1) for k in (0, 3, 20) for session in (0, 1, 2) for dense in (False, True)
         for n, k1 in ((101, True), (64, False)) if session or not dense]


@pytest.mark.parametrize("n, k, session, dense, k1", CASES)
def test_round_trip(tmp_path, n, k, session, dense, k1):
    """write then read gives equal arrays, and write(read(f)) is byte-identical.  n = 101 and 37 state rows are odd, so the u32 and
    f32 sections (w with n odd, V and the tables with k = 0 / 20: 1 / 21 floats a row) need their padding"""
    from libfm_amd import checkpoint as ck
    rec = record(n, k, session, dense, k1, state_rows=37)
    a, b = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    size = ck.write(a, rec)
    assert size == os.path.getsize(a) and size % 8 == 0
    back = ck.read(a)
    assert_records_equal(rec, back)
    ck.write(b, back)
    with open(a, "rb") as fa, open(b, "rb") as fb:
        data = fa.read()
        assert data == fb.read()
    head = ck.read_header(data)
    assert head["state_rows"] == (0 if not session else n if dense else 37)
    kinds = [s[0] for s in head["sections"]]
    assert kinds == [x for x in (1, 2 if k1 else None, 3, 4 if session and not dense else None, 5 if session == 2 else None,
                                 6 if session else None) if x]
    if n % 2 and k1:                                             # (the padding is there, and it is zero)
        off, nbytes = [(s[1], s[2]) for s in head["sections"] if s[0] == ck.SEC_W][0]
        assert nbytes % 8 == 4 and data[off + nbytes:off + nbytes + 4] == b"\0\0\0\0"


def test_checksum_literal():
    """three words, the last one padded, against mix64 written out in plain Python integers"""
    from libfm_amd import checkpoint as ck
    M = (1 << 64) - 1

    def mix64(x):
        x ^= x >> 30
        x = (x * 0xBF58476D1CE4E5B9) & M
        x ^= x >> 27
        x = (x * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)
    data = bytes(range(1, 21))                                   # 20 bytes: two words and four bytes
    words = [int.from_bytes(data[0:8], "little"), int.from_bytes(data[8:16], "little"), int.from_bytes(data[16:20] + b"\0\0\0\0", "little")]
    assert words[0] == 0x0807060504030201 and words[2] == 0x14131211
    want = sum(mix64(u ^ ((i * 0x9E3779B97F4A7C15) & M)) for i, u in enumerate(words)) & M
    assert ck.checksum(data) == want
    assert ck.checksum(data + b"\0\0\0\0") == want               # (the padding is part of the definition)
    assert ck.checksum(b"") == 0
    assert ck.checksum(data) != ck.checksum(data[8:16] + data[0:8] + data[16:])      # (the word index is mixed in: order matters)
    assert mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF       # (the finaliser itself: splitmix64's well-known first output from seed 0)


def _good_file(tmp_path, session=2, dense=False):
    from libfm_amd import checkpoint as ck
    path = str(tmp_path / "good.ckpt")
    ck.write(path, record(101, 3, session, dense, True, state_rows=37))
    with open(path, "rb") as f:
        return ck, path, bytearray(f.read())


def _refused(ck, tmp_path, data, match):
    bad = str(tmp_path / "bad.ckpt")
    with open(bad, "wb") as f:
        f.write(bytes(data))
    with pytest.raises(ck.CheckpointError, match=match):
        ck.read(bad)


def _reseal(ck, data):
    """recompute the header checksum after a deliberate change of a header field"""
    struct.pack_into("<Q", data, 280, ck.checksum(bytes(data[:280])))


def test_reader_refusals(tmp_path):
    ck, path, good = _good_file(tmp_path)
    ck.read(path)
    d = bytearray(good); d[0] ^= 0x20
    _refused(ck, tmp_path, d, "bad magic")
    d = bytearray(good); struct.pack_into("<I", d, 8, 2); _reseal(ck, d)
    _refused(ck, tmp_path, d, "version 2")
    _refused(ck, tmp_path, good[:-1], "truncated")
    _refused(ck, tmp_path, good[:100], "shorter than a checkpoint header")
    d = bytearray(good); d[20] ^= 1                              # (a header byte, not resealed)
    _refused(ck, tmp_path, d, "header's checksum")
    head = ck.read_header(bytes(good))
    assert [s[0] for s in head["sections"]] == [1, 2, 3, 4, 5, 6]
    for kind, off, nbytes, _ in head["sections"]:                # one flipped byte in each section in turn
        d = bytearray(good); d[off + nbytes // 2] ^= 0x10
        _refused(ck, tmp_path, d, "section '%s'" % ck.SECTION_NAMES[kind])
    off, nbytes = [(s[1], s[2]) for s in head["sections"] if s[0] == ck.SEC_W][0]
    d = bytearray(good); d[off + nbytes + 1] = 1                 # (a non-zero padding byte)
    _refused(ck, tmp_path, d, "section 'w'")
    # state_rows > num_attribute, behind a valid header checksum
    d = bytearray(good); struct.pack_into("<Q", d, 72, 102); _reseal(ck, d)
    _refused(ck, tmp_path, d, "state_rows 102 > num_attribute 101")


def _with_ids(ck, good, ids):
    """the good file with another id list, its section checksum and the header resealed: only the list itself is wrong"""
    head = ck.read_header(bytes(good))
    i, (kind, off, nbytes, _) = [(i, s) for i, s in enumerate(head["sections"]) if s[0] == ck.SEC_IDS][0]
    raw = np.asarray(ids, dtype="<u4").tobytes()
    assert len(raw) == nbytes
    d = bytearray(good)
    d[off:off + nbytes] = raw
    struct.pack_into("<Q", d, 88 + 32 * i + 24, ck.checksum(raw))
    _reseal(ck, d)
    return d


def test_reader_refuses_bad_id_lists(tmp_path):
    ck, path, good = _good_file(tmp_path)
    ids = ck.read(path)["state_ids"].copy()
    assert len(ids) == 37
    ck.read(path)
    swapped = ids.copy(); swapped[[4, 5]] = swapped[[5, 4]]
    _refused(ck, tmp_path, _with_ids(ck, good, swapped), "state ids")
    twice = ids.copy(); twice[7] = twice[6]
    _refused(ck, tmp_path, _with_ids(ck, good, twice), "state ids")
    beyond = ids.copy(); beyond[-1] = 101
    _refused(ck, tmp_path, _with_ids(ck, good, beyond), "state ids")
    rec = record(101, 3, 2, False, True, state_rows=37)
    rec["state_ids"] = swapped
    with pytest.raises(ck.CheckpointError, match="state ids"):   # (the writer refuses them too)
        ck.write(str(tmp_path / "w.ckpt"), rec)


def test_header_and_binding():
    """the three symbols stand in include/fmx.h and in capi's table; fmx_ckpt_info and fmx_ckpt_opts have the header's layout"""
    from libfm_amd import capi
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        header = f.read()
    names = [n for n, _, _ in capi.SYMBOLS]
    for fn in ("fmx_checkpoint_save", "fmx_checkpoint_load", "fmx_checkpoint_info"):
        assert names.count(fn) == 1
        assert ("int %s(" % fn) in header
    for text in ("#define FMX_CKPT_DENSE_STATE 1u", "#define FMX_CKPT_MODEL_ONLY  2u", "typedef struct fmx_ckpt_opts { uint32_t flags; uint32_t reserved; } fmx_ckpt_opts;"):
        assert text in header
    assert (capi.CKPT_DENSE_STATE, capi.CKPT_MODEL_ONLY) == (1, 2)
    assert C.sizeof(capi.CkptOpts) == 8
    assert C.sizeof(capi.CkptInfo) == 64
    assert [(f, getattr(capi.CkptInfo, f).offset) for f, _ in capi.CkptInfo._fields_] == [
        ("version", 0), ("session", 4), ("num_attribute", 8), ("num_factor", 16), ("k0", 20), ("k1", 24), ("flags", 28),
        ("state_rows", 32), ("bytes", 40), ("seconds", 48), ("device_seconds", 56)]
    assert "#define FMX_ABI_VERSION 11" in header               # (added without an ABI version change)


def test_sparse_case_property():
    """at least a quarter of the features occur in no row of the sparse case and at least a quarter occur in some row: a sparse file
    of a session trained on it must leave rows out AND hold rows (tests/test_gpu_checkpoint.py cannot pass vacuously)"""
    d, m = sparse_case(8)
    touched = np.zeros(m.n, dtype=bool)
    touched[d.entries["id"]] = True
    print("touched %d of %d features" % (touched.sum(), m.n))
    assert m.n == 6400 and d.n_rows == 128
    assert touched.mean() >= 0.25 and (~touched).mean() >= 0.25


@pytest.mark.parametrize("argv, text", [
    (["-method", "als", "-save_checkpoint", "x"], "ERROR: -save_checkpoint / -load_checkpoint belong to -method sgd and -method bpr: -method als has no checkpoint"),
    (["-method", "mcmc", "-load_checkpoint", "x"], "-method mcmc has no checkpoint"),
    (["-method", "sgda", "-save_checkpoint", "x"], "-method sgda has no checkpoint"),
    (["-method", "sgd", "-load_checkpoint", "x", "-load_model", "y"], "ERROR: -load_checkpoint replaces -load_model: give one of them"),
    (["-method", "sgd", "-checkpoint_dense", "1"], "ERROR: -checkpoint_dense needs -save_checkpoint"),
    (["-method", "sgd", "-save_checkpoint", "x", "-checkpoint_dense", "2"], "ERROR: -checkpoint_dense takes 0 or 1"),
    (["-method", "sgd", "-save_checkpoint", ""], "ERROR: -save_checkpoint needs a filename"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    assert cli.main(["-task", "r", "-train", "no_such_train", "-test", "no_such_test", "-learn_rate", "0.01"] + argv) == 0
    assert text in capsys.readouterr().err


def test_learner_refuses_a_mismatch(tmp_path):
    """an optimizer set by the caller that is not the file's session raises a ValueError naming both -- from the header, no device"""
    from libfm_amd import checkpoint as ck, learner as L
    path = str(tmp_path / "f.ckpt")
    ck.write(path, record(101, 3, 2, False, True, state_rows=37))
    l = L.FMLearnSGD()
    l.optimizer = "adagrad"
    with pytest.raises(ValueError, match="optimizer is adagrad but the file's session is ftrl"):
        l.load_checkpoint(path)
    l = L.FMLearnSGD()
    assert l.load_checkpoint(path) is None and l.optimizer == "ftrl"      # (before init(): looked at, loaded by init())
    l = L.FMLearnSGDA()
    with pytest.raises(ValueError, match="session is ftrl but FMLearnSGDA knows sgd"):
        l.load_checkpoint(path)
