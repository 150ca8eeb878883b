"""CPU: the snapshot file (include/fmx.h "fmx_compact_save"; csrc/fmx_snap_format.h) without a device.

  * the numpy restatement (libfm_amd/compact.py write_snapshot / read_snapshot / snapshot_header): round trips bit for bit, both
    formats, dense and pruned, determinism, the header against the arguments;
  * the C++ parser: scripts/snap_header_check.cpp is built with the host compiler and -fsanitize=address,undefined and run as a
    child; it must accept a restatement-written file and refuse every mutation of the list under "The file" of the format, each
    written here with the header checksum recomputed where the mutation is not the checksum itself; its messages name the field;
  * the four symbols in the header, the binding and the library; the ABI version; NULL handles;
  * the guard lint: every entry point of include/fmx.h that takes a handle either refuses a serve-only handle first thing
    (serve_refuse) or is on the allow-list, which has to be the one DESIGN.md section 27 spells out.

Every comparison is of bits or bytes."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libfm_amd", "csrc")
E_ARG = -1                                                       # FMX_E_ARG

# the calls that work on a serve-only handle (DESIGN.md section 27 spells out the same list: test_guard_allow_list_is_the_documented_one)
ALLOW = ["fmx_destroy", "fmx_last_error", "fmx_get_info", "fmx_get_place_info", "fmx_synchronize",
         "fmx_upload_rows", "fmx_upload_block_rows", "fmx_upload_block_rows_ex", "fmx_synth_rows", "fmx_synth_rows_ex", "fmx_free_rows",
         "fmx_rows_info", "fmx_download_rows",
         "fmx_compact_predict", "fmx_compact_evaluate", "fmx_compact_evaluate_ex", "fmx_compact_topk", "fmx_compact_get_rows",
         "fmx_compact_slot_of", "fmx_compact_end", "fmx_compact_save", "fmx_compact_load"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def model(n, k, seed=0, dead_every=0, nan_row=None, k1=True):
    """a random fp32 model (w0, w[n], v[k][n]); dead_every: every such feature is all zero (a pruned snapshot drops it); nan_row: one
    factor of that feature is NaN (with k > 0)"""
    rng = np.random.default_rng(1000 * k + n + seed)
    w = rng.standard_normal(n).astype(np.float32)
    v = (0.1 * rng.standard_normal((k, n))).astype(np.float32)
    if dead_every:
        w[::dead_every] = 0
        v[:, ::dead_every] = 0
    if nan_row is not None and k > 0:
        v[k // 2, nan_row] = np.nan
    return float(rng.standard_normal()), w, v


def same_model(a, b):
    assert (a.format, a.k0, a.k1, a.k, a.n) == (b.format, b.k0, b.k1, b.k, b.n)
    assert struct.pack("<d", a.w0) == struct.pack("<d", b.w0)
    assert a.w.shape == b.w.shape and np.array_equal(bits(a.w), bits(b.w))
    assert a.v.shape == b.v.shape and np.array_equal(bits(a.v), bits(b.v))
    assert (a.keep is None) == (b.keep is None)
    if a.keep is not None:
        assert np.array_equal(a.keep, b.keep) and np.array_equal(a.dir, b.dir)
        assert np.array_equal(bits(a.rows_w), bits(b.rows_w)) and a.rows_v.shape == b.rows_v.shape and np.array_equal(bits(a.rows_v), bits(b.rows_v))
        assert a.prune_info == b.prune_info


ROUND_TRIP = [(fmt, pruned, k, n) for fmt in ("bf16", "int8") for pruned in (False, True) for k in (0, 5, 40, 64, 100)
              for n in (1, 31, 32, 33, 1000)]


@pytest.mark.parametrize("fmt, pruned, k, n", ROUND_TRIP)
def test_round_trip(tmp_path, fmt, pruned, k, n):
    """write_snapshot -> read_snapshot gives the tables of CompactModel(the same parameters) bit for bit; writing twice gives the same
    bytes; snapshot_header agrees with the arguments.  n = 1000 carries a row with a NaN factor; the pruned cases drop every third
    feature as dead and, at n = 33, keep only what a seen mask of every second id leaves."""
    from libfm_amd import compact
    w0, w, v = model(n, k, dead_every=3 if pruned else 0, nan_row=7 if n == 1000 else None)
    seen = (np.arange(n) % 2 == 0) if pruned and n == 33 else None
    keep = compact.prune_mask(w, v, True, seen) if pruned else None
    a, b = str(tmp_path / "a.snap"), str(tmp_path / "b.snap")
    size = compact.write_snapshot(a, w0, w, v, True, True, 1, -1.0, 1.0, fmt, keep=keep, seen=seen)
    assert size == os.path.getsize(a) and size % 8 == 0
    assert compact.write_snapshot(b, w0, w, v, True, True, 1, -1.0, 1.0, compact.FORMATS[fmt], keep=keep, seen=seen) == size
    with open(a, "rb") as fa, open(b, "rb") as fb:
        assert fa.read() == fb.read()
    got, hd = compact.read_snapshot(a)
    same_model(got, compact.CompactModel(w0, w, v, True, True, fmt, keep=keep, seen=seen))
    head = compact.snapshot_header(a)
    assert head == hd
    rows = int(keep.sum()) if pruned else n
    assert (head["format_name"], head["num_attribute"], head["num_factor"], head["k0"], head["k1"], head["task"], head["min_target"],
            head["max_target"], head["pruned"], head["kept"], head["rows"], head["total"]) == (
        fmt, n, k, 1, 1, 1, -1.0, 1.0, int(pruned), rows if pruned else 0, rows, size)
    assert head["P"] == (compact.row_bytes("int8", k) if fmt == "int8" else 0)
    assert [s[0] for s in head["sections"]] == [x for x in (1, 2 if pruned else None, 3 if fmt == "int8" else None,
                                                            4 if fmt == "bf16" else None, 5 if fmt == "bf16" else None) if x]
    mx, ss, nf = compact.quant_report(v if keep is None else v[:, keep], fmt)
    assert (head["max_abs_err"], head["nonfinite"]) == (mx, nf)
    assert abs(head["sum_sq_err"] - ss) <= 1e-12 * ss              # (the same terms in the device's order: fmx_compact_info's bits)
    if n == 1000 and k > 0:
        assert nf > 0 and np.isnan(got.v[:, 7]).any()


@pytest.mark.parametrize("fmt", ["bf16", "int8"])
def test_keep_nothing(tmp_path, fmt):
    """a pruned snapshot whose keep is all false: no rows, a directory of zeros, and every id reads +0"""
    from libfm_amd import compact
    n, k = 70, 5
    w0, w, v = model(n, k)
    seen = np.zeros(n, dtype=bool)
    keep = compact.prune_mask(w, v, True, seen)
    assert not keep.any()
    path = str(tmp_path / "none.snap")
    compact.write_snapshot(path, w0, w, v, True, True, 0, 0.0, 5.0, fmt, keep=keep, seen=seen)
    got, hd = compact.read_snapshot(path)
    assert hd["kept"] == 0 and hd["rows"] == 0 and hd["dropped_unseen"] + hd["dropped_dead"] == n and not got.dir.any()
    assert not got.w.any() and not got.v.any() and got.rows_v.shape == (k, 0)
    same_model(got, compact.CompactModel(w0, w, v, True, True, fmt, keep=keep, seen=seen))
    with pytest.raises(compact.SnapshotError, match="keep is not prune_mask"):
        compact.write_snapshot(path, w0, w, v, True, True, 0, 0.0, 5.0, fmt, keep=~keep, seen=seen)


def test_device_order_sum_is_the_sum():
    """device_sum_sq adds exactly quant_report's terms -- one per coordinate of a kept, finite row -- in another order: equal to a few
    ulps for every lane mapping (k below, at and above a wavefront's 64 lanes; more rows than one round of the grid holds is not
    reachable at test sizes, the loop over rounds is the same code)"""
    from libfm_amd import compact
    for fmt in ("bf16", "int8"):
        for k in (1, 5, 40, 64, 100, 300):
            _, w, v = model(257, k, nan_row=11)
            keep = np.arange(257) % 5 != 0
            for kp in (None, keep):
                got = compact.device_sum_sq(v, fmt, kp)
                _, want, _ = compact.quant_report(v if kp is None else v[:, kp], fmt)
                assert want > 0 and abs(got - want) <= 1e-13 * want, (fmt, k, got, want)


# ---- the C++ parser ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) to build scripts/snap_header_check.cpp with")
    exe = str(tmp_path_factory.mktemp("snapcheck") / "snap_header_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "scripts", "snap_header_check.cpp"), "-o", exe]
    # the sanitizers' runtimes inside the program where the compiler can put them there (gcc's flags): the program then runs the
    # same whatever else the process loads
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300).returncode != 0:
        subprocess.run(cmd, check=True, timeout=300)
    return exe


def run_checker(exe, *args):
    p = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    return p.returncode, p.stdout.decode()


def test_parser_self_test(checker):
    """planned and encoded headers parse back; every prefix, every flipped bit and a length off by one are refused; random mutations
    behind a valid checksum are refused or re-plan to themselves -- all from heap buffers of exactly the length the parser is told"""
    rc, out = run_checker(checker)
    print(out)
    assert rc == 0 and " 0 failures" in out


def reseal(data):
    from libfm_amd import checkpoint as ck
    struct.pack_into("<Q", data, 248, ck.checksum(bytes(data[:248])))


MUTATIONS = [
    # name, (offset, struct format, value) or a callable on the bytearray, reseal, what the message names
    ("magic", lambda d: d.__setitem__(0, d[0] ^ 0x20), False, "bad magic"),
    ("version", (8, "<I", 2), True, "version 2"),
    ("header checksum", lambda d: d.__setitem__(20, d[20] ^ 1), False, "header's checksum"),
    ("format", (12, "<I", 2), True, "unknown format 2"),
    ("num_attribute 0", (16, "<Q", 0), True, "num_attribute 0"),
    ("num_attribute 2^32", (16, "<Q", 1 << 32), True, "num_attribute 4294967296"),
    ("num_factor", (24, "<I", 1025), True, "num_factor 1025"),
    ("k0", (28, "<I", 2), True, "k0 / k1"),
    ("task", (36, "<I", 7), True, "task 7"),
    ("kept > num_attribute", (64, "<Q", 1001), True, "kept 1001 > num_attribute 1000"),
    ("P", (60, "<I", 32), True, "P (bytes of an int8 block) is 32"),
    ("section table", (120 + 32 + 16, "<Q", 12345), True, "section table entry 1"),
    ("section count", (112, "<I", 2), True, "section table has 2 entries"),
    ("truncated", lambda d: d.__delitem__(slice(len(d) - 8, len(d))), False, "truncated"),
    ("one byte long", lambda d: d.append(0), False, "truncated"),
]


@pytest.mark.parametrize("fmt", ["bf16", "int8"])
def test_parser_accepts_and_refuses(tmp_path, checker, fmt):
    from libfm_amd import compact
    n, k = 1000, 40
    w0, w, v = model(n, k, dead_every=3)
    keep = compact.prune_mask(w, v, True)
    good = str(tmp_path / "good.snap")
    compact.write_snapshot(good, w0, w, v, True, True, 1, -1.0, 1.0, fmt, keep=keep)
    rc, out = run_checker(checker, good)
    print(out)
    assert rc == 0 and ("ok format %d num_attribute 1000 num_factor 40" % compact.FORMATS[fmt]) in out and ("kept %d" % keep.sum()) in out
    dense = str(tmp_path / "dense.snap")
    compact.write_snapshot(dense, w0, w, v, True, True, 1, -1.0, 1.0, fmt)
    assert run_checker(checker, dense)[0] == 0
    with open(good, "rb") as f:
        data = f.read()
    with open(dense, "rb") as f:
        dense_data = f.read()
    cases = [(name, data, how, seal, text) for name, how, seal, text in MUTATIONS]
    # kept without pruned: the dense file with kept set; P of the other format's rule
    cases.append(("kept without pruned", dense_data, (64, "<Q", 5), True, "kept 5 without pruned"))
    cases.append(("pruned 2", data, (56, "<I", 2), True, "pruned is 2"))
    cases.append(("counts", data, (96, "<Q", 1), True, "kept + dropped_dead + dropped_unseen"))
    for name, src, how, seal, text in cases:
        d = bytearray(src)
        if callable(how):
            how(d)
        else:
            struct.pack_into(how[1], d, how[0], how[2])
        if seal:
            reseal(d)
        bad = str(tmp_path / "bad.snap")
        with open(bad, "wb") as f:
            f.write(bytes(d))
        rc, out = run_checker(checker, bad)
        print("%-22s -> %d %s" % (name, rc, out.strip()))
        assert rc == 2 and out.startswith("refused: ") and text in out, name
        with pytest.raises(compact.SnapshotError):                 # (the restatement's reader refuses the same files)
            compact.read_snapshot(bad)


def test_reader_refuses_what_only_the_body_shows(tmp_path):
    """one flipped byte in each section; a directory with a base off by one, or a bit beyond n, behind RECOMPUTED checksums"""
    from libfm_amd import checkpoint as ck, compact
    n, k = 1000, 8
    w0, w, v = model(n, k, dead_every=3)
    keep = compact.prune_mask(w, v, True)
    good = str(tmp_path / "good.snap")
    compact.write_snapshot(good, w0, w, v, True, True, 1, -1.0, 1.0, "int8", keep=keep)
    with open(good, "rb") as f:
        data = f.read()
    hd = compact.snapshot_header(good)

    def refused(d, match):
        bad = str(tmp_path / "bad.snap")
        with open(bad, "wb") as f:
            f.write(bytes(d))
        with pytest.raises(compact.SnapshotError, match=match):
            compact.read_snapshot(bad)
    for kind, off, nbytes, _ in hd["sections"]:
        d = bytearray(data); d[off + nbytes // 2] ^= 0x10
        refused(d, "section '%s'" % compact.SNAP_SECTION_NAMES[kind])
    for d in bad_directories(data, hd):
        refused(d, "section 'dir'")


def bad_directories(data, hd):
    """the file with (a) one base off by one, (b) a bit set beyond num_attribute in the last word -- the section's checksum and the
    header's recomputed, so that only a check of the directory itself can refuse them (tests/test_gpu_snapshot.py loads them too)"""
    from libfm_amd import checkpoint as ck
    i, (kind, off, nbytes, _) = [(i, s) for i, s in enumerate(hd["sections"]) if s[0] == 2][0]
    n = hd["num_attribute"]
    out = []
    for which in ("base", "bit"):
        dirw = np.frombuffer(data[off:off + nbytes], dtype="<u4").reshape(-1, 2).copy()
        if which == "base":
            dirw[len(dirw) // 2, 1] += 1
        else:
            assert n % 32
            dirw[-1, 0] |= np.uint32(1 << 31)
        d = bytearray(data)
        d[off:off + nbytes] = dirw.tobytes()
        struct.pack_into("<Q", d, 120 + 32 * i + 24, ck.checksum(dirw.tobytes()))
        reseal(d)
        out.append(d)
    return out


# ---- header, binding, library ---------------------------------------------------------------------------------------------------
NEW = ("fmx_compact_save", "fmx_compact_load", "fmx_snapshot_info", "fmx_serve_open")


def test_symbols_header_binding_library(tmp_path):
    from libfm_amd import capi, compact
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        header = f.read()
    names = [n for n, _, _ in capi.SYMBOLS]
    lib = capi.load()
    for fn in NEW:
        assert names.count(fn) == 1 and ("int %s(" % fn) in header
        assert getattr(lib, fn) is not None                        # (exported: -fvisibility=hidden hides everything fmx.h does not declare)
    assert "#define FMX_ABI_VERSION 11" in header and lib.fmx_abi_version() == 11
    assert C.sizeof(capi.SnapInfo) == 144
    assert [(f, getattr(capi.SnapInfo, f).offset) for f, _ in capi.SnapInfo._fields_] == [
        ("version", 0), ("format", 4), ("num_attribute", 8), ("num_factor", 16), ("k0", 20), ("k1", 24), ("task", 28), ("min_target", 32),
        ("max_target", 40), ("pruned", 48), ("row_bytes", 52), ("kept", 56), ("rows", 64), ("nonfinite", 72), ("max_abs_err", 80),
        ("sum_sq_err", 88), ("dropped_dead", 96), ("dropped_unseen", 104), ("bytes", 112), ("bytes_compact", 120), ("seconds", 128),
        ("device_seconds", 136)]
    # NULL handles, NULL paths: FMX_E_ARG, no device touched
    info = capi.SnapInfo()
    assert lib.fmx_compact_save(None, b"x", C.byref(info)) == E_ARG
    assert lib.fmx_compact_load(None, b"x", C.byref(info)) == E_ARG
    err = C.create_string_buffer(256)
    assert lib.fmx_snapshot_info(None, C.byref(info), err, len(err)) == E_ARG and b"NULL" in err.value
    h = capi.H()
    assert lib.fmx_serve_open(None, 0, C.byref(h), None) == E_ARG and not h
    assert lib.fmx_serve_open(b"x", 0, None, None) == E_ARG
    missing = str(tmp_path / "no_such.snap").encode()
    assert lib.fmx_serve_open(missing, 0, C.byref(h), None) == E_ARG and not h
    assert b"cannot open" in lib.fmx_last_error(None)
    # fmx_snapshot_info is the C++ parser behind the ABI: a restatement-written file, field for field, and a refusal with its reason
    w0, w, v = model(100, 5, dead_every=4)
    keep = compact.prune_mask(w, v, True)
    path = str(tmp_path / "f.snap")
    size = compact.write_snapshot(path, w0, w, v, True, False, 0, -2.5, 7.0, "int8", keep=keep)
    si, hd = capi.snapshot_info(path), compact.snapshot_header(path)
    assert (si.version, si.format, si.num_attribute, si.num_factor, si.k0, si.k1, si.task, si.min_target, si.max_target, si.pruned,
            si.row_bytes, si.kept, si.rows, si.nonfinite, si.dropped_dead, si.dropped_unseen, si.bytes, si.bytes_compact) == (
        1, 3, 100, 5, 1, 0, 0, -2.5, 7.0, 1, 16, int(keep.sum()), int(keep.sum()), 0, hd["dropped_dead"], 0, size, 0)
    assert struct.pack("<dd", si.max_abs_err, si.sum_sq_err) == struct.pack("<dd", hd["max_abs_err"], hd["sum_sq_err"])
    with open(path, "r+b") as f:
        f.truncate(size - 8)
    with pytest.raises(capi.FmxError, match="truncated"):
        capi.snapshot_info(path)
    # a refused file gives no handle, before any device is looked for
    assert lib.fmx_serve_open(path.encode(), 0, C.byref(h), None) == E_ARG and not h
    assert b"truncated" in lib.fmx_last_error(None)


def test_int8_block_size_is_the_devices(tmp_path):
    """fmx_snap_format.h restates compact8_row_bytes: for every k the library's rule and compact.row_bytes agree, and the C++ parser
    (through fmx_snapshot_info) accepts an int8 header of that k with exactly that P and refuses P + 8 and, where there is one, P - 8"""
    from libfm_amd import capi, compact
    lib = capi.load()
    path = str(tmp_path / "k.snap")
    for k in range(0, 1025):
        p = compact.row_bytes("int8", k)
        assert lib.fmx_compact_row_bytes(capi.COMPACT_INT8, k) == p
        compact.write_snapshot(path, 0.0, np.zeros(1, dtype=np.float32), np.zeros((k, 1), dtype=np.float32), True, True, 0, 0.0, 1.0, "int8")
        si = capi.snapshot_info(path)
        assert (si.num_factor, si.row_bytes, si.bytes) == (k, p, 256 + 8 + p)
        with open(path, "rb") as f:
            good = f.read()
        for wrong in (p + 8, p - 8):
            if wrong < 8:
                continue
            d = bytearray(good)
            struct.pack_into("<I", d, 60, wrong)
            reseal(d)
            with open(path, "wb") as f:
                f.write(bytes(d))
            with pytest.raises(capi.FmxError, match="P \\(bytes of an int8 block\\) is %d" % wrong):
                capi.snapshot_info(path)


# ---- the guard lint ---------------------------------------------------------------------------------------------------------------
def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def handle_entry_points():
    """every prototype of include/fmx.h whose first parameter is an fmx_handle"""
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        header = strip_comments(f.read())
    return re.findall(r"\b(fmx_\w+)\s*\(\s*fmx_handle\s+\w+", header)


def sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(".hip"):
            with open(os.path.join(CSRC, name)) as f:
                out[name] = strip_comments(f.read())
    return out


def body_of(fn, src):
    """(file, the text between the braces of fn's definition)"""
    for name, text in src.items():
        m = re.search(r"^[\w \*]*\b%s\s*\(\s*fmx_handle\s+(\w+)[^;{]*\{" % fn, text, flags=re.M)
        if not m:
            continue
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            i += 1
        return name, m.group(1), text[m.end():i - 1]
    raise AssertionError("%s is declared in include/fmx.h and defined nowhere under libfm_amd/csrc" % fn)


def guarded_first(param, body):
    """serve_refuse(<handle>, ...) stands in front of every other use of the handle but the NULL check"""
    at = body.find("serve_refuse(")
    if at < 0:
        return False
    if not re.match(r"serve_refuse\(\s*%s\s*," % param, body[at:]):
        return False
    before = body[:at]
    before = re.sub(r"if\s*\(\s*!%s\b[^;]*;" % param, " ", before, count=1)      # the NULL check (it may test other pointers too)
    return re.search(r"\b%s\b" % param, before) is None


def test_guard_lint():
    fns = handle_entry_points()
    assert len(fns) >= 88 and len(set(fns)) == len(fns)
    for fn in ALLOW + ["fmx_compact_begin", "fmx_compact_begin_pruned", "fmx_comm_init_rank", "fmx_predict", "fmx_sgd_epoch", "fmx_checkpoint_load"]:
        assert fn in fns, fn
    src = sources()
    missed = []
    for fn in fns:
        name, param, body = body_of(fn, src)
        if fn in ALLOW:
            assert "serve_refuse(" not in body, "%s is on the allow-list and refuses a serve-only handle" % fn
        elif not guarded_first(param, body):
            missed.append("%s (%s)" % (fn, name))
    assert not missed, "entry points that reach their work with a serve-only handle: " + ", ".join(missed)
    # a group refuses a serve-only member before it keeps any handle
    _, text = [(n, t) for n, t in src.items() if "int fmx_group_create(" in t][0]
    body = text[text.index("int fmx_group_create("):]
    assert "serve_refuse(" in body[:body.index("new fmx_group_s")]
    # one helper, one message
    with open(os.path.join(CSRC, "fmx_internal.h")) as f:
        internal = f.read()
    assert internal.count("a serve-only handle holds no model") == 1 and "FMX_E_STATE" in internal[internal.index("inline int serve_refuse"):][:300]
    assert not any("a serve-only handle holds no model" in t for t in src.values())


def test_guard_allow_list_is_the_documented_one():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    sec = design[design.index("\n## 27."):]
    para = sec[sec.index("Allow-list"):]
    para = para[:para.index("\n\n")]
    assert sorted(set(re.findall(r"fmx_\w+", para))) == sorted(ALLOW)


# ---- the command line's refusals, before any device -----------------------------------------------------------------------------
@pytest.mark.parametrize("argv, text", [
    (["-method", "sgd", "-train", "x", "-test", "y", "-task", "r", "-save_snapshot", "f"], "ERROR: -save_snapshot needs -serve (bf16 | int8)"),
    (["-method", "sgd", "-train", "x", "-test", "y", "-task", "r", "-serve", "int8", "-save_snapshot", ""], "ERROR: -save_snapshot needs a filename"),
    (["-method", "sgd", "-train", "x", "-test", "y", "-task", "r", "-load_snapshot", "f"], "ERROR: -load_snapshot belongs to -method serve"),
    (["-method", "sgd", "-optimizer", "ftrl", "-devices", "0,0", "-train", "x", "-test", "y", "-task", "c", "-save_snapshot", "f"],
     "ERROR: -save_snapshot is not supported with -devices"),
    (["-method", "serve", "-test", "y"], "ERROR: -method serve needs -load_snapshot"),
    (["-method", "serve", "-load_snapshot", "f"], "ERROR: -test is mandatory"),
    (["-method", "serve", "-load_snapshot", "f", "-test", "y", "-train", "x"], "ERROR: -train is not supported with -method serve"),
    (["-method", "serve", "-load_snapshot", "f", "-test", "y", "-dim", "1,1,8"], "ERROR: -dim is not supported with -method serve"),
    (["-method", "serve", "-load_snapshot", "f", "-test", "y", "-learn_rate", "0.1"], "ERROR: -learn_rate is not supported with -method serve"),
    (["-method", "serve", "-load_snapshot", "f", "-test", "y", "-iter", "3"], "ERROR: -iter is not supported with -method serve"),
    (["-method", "serve", "-load_snapshot", "f", "-test", "y", "-save_model", "m"], "ERROR: -save_model is not supported with -method serve"),
    (["-method", "serve", "-load_snapshot", "f", "-test", "y", "-topk", "3"], "ERROR: top-K retrieval needs -topk and -candidates"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    assert cli.main(argv) == 0
    assert text in capsys.readouterr().err


def test_cli_serve_reads_the_header_first(tmp_path, capsys):
    """-method serve refuses a file that is no snapshot, and a -task that is not the file's, from the header alone"""
    from libfm_amd import cli, compact
    junk, snap = str(tmp_path / "junk"), str(tmp_path / "f.snap")
    with open(junk, "wb") as f:
        f.write(b"x" * 400)
    assert cli.main(["-method", "serve", "-load_snapshot", junk, "-test", "no_such_test"]) == 0
    assert "ERROR: bad magic" in capsys.readouterr().err
    w0, w, v = model(50, 3)
    compact.write_snapshot(snap, w0, w, v, True, True, 1, -1.0, 1.0, "bf16")
    assert cli.main(["-method", "serve", "-load_snapshot", snap, "-test", "no_such_test", "-task", "r"]) == 0
    assert "ERROR: -task r but the snapshot was taken for -task c" in capsys.readouterr().err
    assert cli.main(["-method", "serve", "-load_snapshot", snap, "-test", "no_such_test", "-metrics", "rmse"]) == 0
    assert "ERROR: -metrics knows auc and logloss, not 'rmse'" in capsys.readouterr().err
