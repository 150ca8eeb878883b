"""CPU restatement of the binary checkpoint format (include/fmx.h "fmx_checkpoint_*", csrc/fmx_ckpt_format.h).
numpy only: no library, no device.  The device writes and reads the same bytes; tests/test_gpu_checkpoint.py holds the two together.

Little-endian.  A 288-byte header:
     0  char[8]  magic b"FMXCKPT\\0"
     8  u32 version (1)          12  u32 session: 0 none, 1 AdaGrad, 2 FTRL
    16  u64 num_attribute        24  u32 num_factor    28  u32 k0    32  u32 k1
    36  u32 flags the file was saved with (1 dense state, 2 model only)
    40  f32[8] the session's constants: AdaGrad eta, init_acc; FTRL 1 / alpha, beta, l1_w, l1_v, l2_w, l2_v, init_acc; zeros behind
    72  u64 state_rows           80  u32 number of sections    84  u32 0
    88  6 x {u32 kind, u32 0, u64 offset, u64 bytes, u64 checksum}, unused entries all zero
   280  u64 checksum of bytes 0 .. 279
then the sections in the order of their kinds, the first at byte 288, each padded with zero bytes to a multiple of 8:
    1 w0  one f64                                2 w   num_attribute f32, only with k1
    3 V   [num_attribute][num_factor] f32         4 ids state_rows u32, strictly ascending; absent when dense or without a session
    5 z   (FTRL only), 6 n: [state_rows][1 + num_factor] f32, the linear coordinate's value first
A section's checksum is the sum mod 2^64, over its padded 8-byte words u_i, of mix64(u_i ^ (i * 0x9E3779B97F4A7C15)).

A record (read's result, write's argument) is a dict:
    num_attribute, num_factor, k0, k1, flags     ints (flags: DENSE_STATE | MODEL_ONLY as the file was saved)
    session                                      0, 1 or 2
    consts                                       float32[8]
    w0                                           float (fp64)
    w                                            float32[num_attribute], or None without k1
    v                                            float32[num_attribute][num_factor]
    state_ids                                    uint32[state_rows], or None (dense, or no session)
    state                                        {"n": float32[state_rows][1 + num_factor]} and for FTRL also "z"; {} without a session
"""
import struct

import numpy as np

MAGIC = b"FMXCKPT\0"
VERSION = 1
HEADER_BYTES = 288
MAX_SECTIONS = 6
DENSE_STATE, MODEL_ONLY = 1, 2
SESSION_NONE, SESSION_ADAGRAD, SESSION_FTRL = 0, 1, 2
SEC_W0, SEC_W, SEC_V, SEC_IDS, SEC_Z, SEC_N = 1, 2, 3, 4, 5, 6
SECTION_NAMES = {SEC_W0: "w0", SEC_W: "w", SEC_V: "V", SEC_IDS: "state ids", SEC_Z: "state z", SEC_N: "state n"}
SESSION_NAMES = {SESSION_NONE: "none", SESSION_ADAGRAD: "adagrad", SESSION_FTRL: "ftrl"}
ADAGRAD_CONSTS = ("eta", "init_acc")
FTRL_CONSTS = ("inv_alpha", "beta", "l1_w", "l1_v", "l2_w", "l2_v", "init_acc")
GOLDEN = 0x9E3779B97F4A7C15


class CheckpointError(ValueError):
    pass


def _mix64(x):
    """fmx_kernels.h mix64 on a uint64 array (the arithmetic wraps mod 2^64)"""
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def checksum(data):
    """the checksum of a section: `data` is its bytes without the padding"""
    data = bytes(data)
    data += b"\0" * (-len(data) % 8)
    u = np.frombuffer(data, dtype="<u8")
    if u.size == 0:
        return 0
    with np.errstate(over="ignore"):
        return int(_mix64(u ^ (np.arange(u.size, dtype=np.uint64) * np.uint64(GOLDEN))).sum(dtype=np.uint64))


def _plan(session, num_attribute, num_factor, k1, flags, state_rows):
    """[(kind, offset, bytes)] of the sections and the file's length"""
    row = (1 + num_factor) * 4
    secs, off = [], HEADER_BYTES

    def add(kind, nbytes):
        nonlocal off
        secs.append((kind, off, nbytes))
        off += nbytes + (-nbytes % 8)
    add(SEC_W0, 8)
    if k1:
        add(SEC_W, num_attribute * 4)
    add(SEC_V, num_attribute * num_factor * 4)
    if session != SESSION_NONE:
        if not flags & DENSE_STATE:
            add(SEC_IDS, state_rows * 4)
        if session == SESSION_FTRL:
            add(SEC_Z, state_rows * row)
        add(SEC_N, state_rows * row)
    return secs, off


def _header(rec, state_rows, table):
    head = bytearray(HEADER_BYTES)
    head[0:8] = MAGIC
    struct.pack_into("<IIQIIII", head, 8, VERSION, rec["session"], rec["num_attribute"], rec["num_factor"], int(bool(rec["k0"])),
                     int(bool(rec["k1"])), rec["flags"])
    head[40:72] = np.asarray(rec["consts"], dtype="<f4").tobytes()
    struct.pack_into("<QII", head, 72, state_rows, len(table), 0)
    for i, (kind, off, nbytes, cs) in enumerate(table):
        struct.pack_into("<IIQQQ", head, 88 + 32 * i, kind, 0, off, nbytes, cs)
    struct.pack_into("<Q", head, 280, checksum(head[:280]))
    return bytes(head)


def write(path, rec):
    """write a record as a checkpoint file; returns the number of bytes.  Shapes and the id list are checked (CheckpointError)."""
    n, k, session, flags = int(rec["num_attribute"]), int(rec["num_factor"]), int(rec["session"]), int(rec["flags"])
    if session not in SESSION_NAMES or flags & ~(DENSE_STATE | MODEL_ONLY):
        raise CheckpointError("unknown session %r or flags %r" % (session, flags))
    consts = np.zeros(8, dtype=np.float32)
    given = np.asarray(rec.get("consts", ()), dtype=np.float32).reshape(-1)
    consts[:given.size] = given
    v = np.ascontiguousarray(rec["v"], dtype="<f4").reshape(n, k)
    w = None
    if rec["k1"]:
        w = np.ascontiguousarray(rec["w"], dtype="<f4")
        if w.shape != (n,):
            raise CheckpointError("w has shape %r, not (%d,)" % (w.shape, n))
    body = {SEC_W0: struct.pack("<d", float(rec["w0"])), SEC_W: None if w is None else w.tobytes(), SEC_V: v.tobytes()}
    state_rows = 0
    if session != SESSION_NONE:
        ids = rec.get("state_ids")
        if flags & DENSE_STATE:
            if ids is not None:
                raise CheckpointError("a dense file has no state ids")
            state_rows = n
        else:
            ids = np.ascontiguousarray(ids, dtype="<u4").reshape(-1)
            state_rows = ids.size
            _check_ids(ids, n)
            body[SEC_IDS] = ids.tobytes()
        for kind, name in ((SEC_Z, "z"), (SEC_N, "n")):
            if kind == SEC_Z and session != SESSION_FTRL:
                continue
            t = np.ascontiguousarray(rec["state"][name], dtype="<f4")
            if t.shape != (state_rows, 1 + k):
                raise CheckpointError("state %s has shape %r, not (%d, %d)" % (name, t.shape, state_rows, 1 + k))
            body[kind] = t.tobytes()
    secs, total = _plan(session, n, k, bool(rec["k1"]), flags, state_rows)
    table = [(kind, off, nbytes, checksum(body[kind])) for kind, off, nbytes in secs]
    rec = dict(rec, consts=consts)
    with open(path, "wb") as f:
        f.write(_header(rec, state_rows, table))
        for kind, off, nbytes in secs:
            assert f.tell() == off and len(body[kind]) == nbytes
            f.write(body[kind] + b"\0" * (-nbytes % 8))
        assert f.tell() == total
    return total


def _check_ids(ids, n):
    if ids.size and (int(ids.max()) >= n or np.any(ids[1:] <= ids[:-1])):
        raise CheckpointError("section 'state ids': the ids are not strictly ascending or not below num_attribute")


def read_header(data):
    """the header of a file's bytes (at least the first 288; the whole length is checked against len(data) by read): a dict with
    the record's scalar fields, state_rows and sections = [(kind, offset, bytes, checksum)]"""
    if len(data) < HEADER_BYTES:
        raise CheckpointError("the file is shorter than a checkpoint header")
    if data[0:8] != MAGIC:
        raise CheckpointError("bad magic: not a checkpoint file")
    version, session, n, k, k0, k1, flags = struct.unpack_from("<IIQIIII", data, 8)
    if version != VERSION:
        raise CheckpointError("checkpoint version %d, this module reads version %d" % (version, VERSION))
    if struct.unpack_from("<Q", data, 280)[0] != checksum(data[:280]):
        raise CheckpointError("the header's checksum does not match")
    state_rows, n_sections, zero = struct.unpack_from("<QII", data, 72)
    if session not in SESSION_NAMES or flags & ~(DENSE_STATE | MODEL_ONLY) or k0 > 1 or k1 > 1 or not 0 < n < 2 ** 32 or k > 1024 or zero:
        raise CheckpointError("a header field is out of range")
    if state_rows > n:
        raise CheckpointError("state_rows %d > num_attribute %d" % (state_rows, n))
    if (session == SESSION_NONE and state_rows) or (session != SESSION_NONE and flags & DENSE_STATE and state_rows != n):
        raise CheckpointError("state_rows %d does not fit the session and flags" % state_rows)
    secs, total = _plan(session, n, k, bool(k1), flags, state_rows)
    table = [struct.unpack_from("<IIQQQ", data, 88 + 32 * i) for i in range(MAX_SECTIONS)]
    want = [(kind, 0, off, nbytes) for kind, off, nbytes in secs] + [(0, 0, 0, 0)] * (MAX_SECTIONS - len(secs))
    if n_sections != len(secs) or [t[:4] for t in table] != want or any(t[4] for t in table[len(secs):]):
        raise CheckpointError("the section table does not match the header's fields")
    return dict(version=version, session=session, num_attribute=n, num_factor=k, k0=k0, k1=k1, flags=flags,
                consts=np.frombuffer(data[40:72], dtype="<f4").copy(), state_rows=state_rows, total=total,
                sections=[(t[0], t[2], t[3], t[4]) for t in table[:len(secs)]])


def read(path):
    """read and verify a checkpoint file (CheckpointError names what is wrong); returns a record"""
    with open(path, "rb") as f:
        data = f.read()
    h = read_header(data)
    if h["total"] != len(data):
        raise CheckpointError("the sections end at byte %d but the file has %d bytes (truncated?)" % (h["total"], len(data)))
    n, k, rows = h["num_attribute"], h["num_factor"], h["state_rows"]
    raw = {}
    for kind, off, nbytes, cs in h["sections"]:
        raw[kind] = data[off:off + nbytes]
        if checksum(raw[kind]) != cs or any(data[off + nbytes:off + nbytes + (-nbytes % 8)]):
            raise CheckpointError("section '%s': checksum mismatch" % SECTION_NAMES[kind])
    rec = {key: h[key] for key in ("num_attribute", "num_factor", "k0", "k1", "flags", "session", "consts")}
    rec["w0"] = struct.unpack("<d", raw[SEC_W0])[0]
    rec["w"] = np.frombuffer(raw[SEC_W], dtype="<f4").copy() if SEC_W in raw else None
    rec["v"] = np.frombuffer(raw[SEC_V], dtype="<f4").reshape(n, k).copy()
    rec["state_ids"] = None
    if SEC_IDS in raw:
        rec["state_ids"] = np.frombuffer(raw[SEC_IDS], dtype="<u4").copy()
        _check_ids(rec["state_ids"], n)
    rec["state"] = {name: np.frombuffer(raw[kind], dtype="<f4").reshape(rows, 1 + k).copy()
                    for kind, name in ((SEC_Z, "z"), (SEC_N, "n")) if kind in raw}
    return rec


def consts_dict(rec):
    """the session's constants by name ({} without a session)"""
    names = {SESSION_ADAGRAD: ADAGRAD_CONSTS, SESSION_FTRL: FTRL_CONSTS}.get(rec["session"], ())
    return {name: float(rec["consts"][i]) for i, name in enumerate(names)}
