"""fp64 / bit-level restatement of the serving snapshots (include/fmx.h "fmx_compact_*"; DESIGN.md sections 19 and 21).  CPU only.

bf16 is the upper half of an fp32.  bf16_round rounds to nearest, ties to even, on bit 16: for a bit pattern u that is not a NaN

    q = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000

so +-0, +-inf and the fp32 subnormals follow the same rule and a finite value above bf16's largest carries into the exponent and
becomes +-inf.  A NaN stays a NaN: its upper half with the quiet bit set.

int8 is row-wise and symmetric.  For the k factors of one feature, in fp64: a = max |v_f|, inv = 127 / a (0 when a = 0),
q_f = clamp(rint(v_f * inv), -127, 127) with ties to even, scale = float32(a / 127).  A factor dequantises to the fp32 product
scale * float32(q_f).  A row with a non-finite factor has scale NaN and codes 0: all of it dequantises to NaN.

CompactModel is what fmx_compact_begin freezes -- w0 and w unchanged, V rounded -- and predicts in fp64 by fm_model::predict
(fm_model.h:105-127), the formula the fp64 oracle's predict_raw restates.  quant_report gives the three numbers of fmx_compact_info.

The pruned snapshot (fmx_compact_begin_pruned) keeps a row only for the features of prune_mask: not dead
(fmx_param_sparsity's dead_features rule, negated) and, with `seen`, met in the keep slot.  Rows stand in ascending id order; directory
is the rank directory {bits, base} per 32 ids, slot_of the lookup through it.  CompactModel(..., keep=mask) packs the kept rows in that
order, scores a dropped id as a row of +0 with w = +0, and reports fmx_compact_prune_info (prune_info) and fmx_compact_info (info).

The snapshot FILE (fmx_compact_save / fmx_compact_load / fmx_serve_open; csrc/fmx_snap_format.h) is restated at
the end: write_snapshot builds the file of a model's snapshot from its fp32 parameters -- the int8 blocks, the bf16 rows and the
directory from the functions above, the header's figures from device_quant_report, which adds the squared errors in the order the
quantising kernels do -- byte for byte what the device writes; read_snapshot verifies and reads one back as a CompactModel;
snapshot_header reads the header alone.
"""
import struct

import numpy as np

from .checkpoint import checksum as _checksum

FORMATS = {"bf16": 1, "int8": 3}      # FMX_COMPACT_*: fmx_compact_opts::format (2 is not assigned)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bf16_bits(a):
    """the bf16 bit patterns (uint16) of a float32 array"""
    u = _bits(a)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (u.astype(np.uint64) + 0x7FFF + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)
    q = np.where(nan, (u >> np.uint32(16)) | np.uint32(0x0040), r.astype(np.uint32))
    return q.astype(np.uint16)


def bf16_round(a):
    """float32 array -> the float32 values of its bf16 rounding"""
    q = bf16_bits(a).astype(np.uint32) << np.uint32(16)
    return q.view(np.float32).reshape(np.shape(a))


def int8_quant(v):
    """factor table v[k][n] (one COLUMN per feature, as get_params returns it) -> (codes int8 [k][n], scale float32 [n])"""
    v32 = np.ascontiguousarray(v, dtype=np.float32)
    if v32.ndim != 2:
        raise ValueError("int8_quant: a [k][n] table")
    n = v32.shape[1]
    bad = ~np.isfinite(v32).all(axis=0) if v32.shape[0] else np.zeros(n, dtype=bool)
    v64 = np.where(bad[None, :], 0.0, v32.astype(np.float64))
    a = np.abs(v64).max(axis=0) if v32.shape[0] else np.zeros(n)
    with np.errstate(divide="ignore"):
        inv = np.where(a > 0.0, 127.0 / np.where(a > 0.0, a, 1.0), 0.0)
    codes = np.clip(np.rint(v64 * inv[None, :]), -127.0, 127.0).astype(np.int8)
    scale = (a / 127.0).astype(np.float32)
    scale[bad] = np.float32(np.nan)
    return codes, scale


def int8_dequant(codes, scale):
    """(codes [k][n], scale [n]) -> float32 [k][n]: one fp32 multiply per factor"""
    with np.errstate(invalid="ignore"):
        return np.asarray(scale, dtype=np.float32)[None, :] * np.asarray(codes).astype(np.float32)


def int8_round(v):
    """float32 table [k][n] -> the float32 values the int8 snapshot holds for it"""
    return int8_dequant(*int8_quant(v))


def row_bytes(format, k):
    """snapshot bytes per feature (fmx_compact_row_bytes): 2 * rs + 4 for bf16, P(k) for int8, 0 for an unknown format"""
    k = int(k)
    if k < 0:
        return 0
    if format in ("bf16", FORMATS["bf16"]):
        kp = 1
        while kp < max(k, 1):
            kp <<= 1
        rs = min(kp, (k + 15) // 16 * 16) if kp >= 32 else kp      # V's row stride in elements
        return 2 * rs + 4
    if format in ("int8", FORMATS["int8"]):
        need = k + 8
        if need > 128:
            return (need + 63) // 64 * 64
        p = 8
        while p < need:
            p <<= 1
        return p
    return 0


def quant_report(v, format="bf16"):
    """(max |v - q(v)|, sum (v - q(v))^2, nonfinite) of a factor table as the device holds it (float32).
    bf16: the maximum and the sum run over the coordinates whose bf16 value is finite, nonfinite counts the others; v - q(v) is
    exact in fp32.  int8 (v[k][n]): they run in fp64 over the rows without a non-finite factor, nonfinite counts k per other row."""
    if format == "int8":
        v32 = np.ascontiguousarray(v, dtype=np.float32)
        if v32.ndim != 2 or v32.shape[0] == 0:
            return 0.0, 0.0, 0
        q = int8_round(v32)
        fin = np.isfinite(v32).all(axis=0)
        err = np.abs(v32[:, fin].astype(np.float64) - q[:, fin].astype(np.float64)).reshape(-1)
        return (float(err.max()) if err.size else 0.0), float(np.sum(err * err)), int((~fin).sum()) * v32.shape[0]
    if format != "bf16":
        raise ValueError("unknown serving format %r (%s)" % (format, " | ".join(FORMATS)))
    v32 = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    q = bf16_round(v32)
    fin = np.isfinite(q)
    with np.errstate(invalid="ignore"):
        err = np.abs(v32[fin] - q[fin]).astype(np.float64)
    return (float(err.max()) if err.size else 0.0), float(np.sum(err * err)), int((~fin).sum())


SLOT_NONE = 0xFFFFFFFF      # slot_of: a dropped id


def dead_mask(w, v, k1):
    """bool [n]: the features that contribute to no prediction -- all k factors == 0.0f (-0 counts, NaN does not; with k = 0 every
    factor row counts as all zero) and (w_j == 0.0f or not k1).  Its sum is fmx_sparsity::dead_features."""
    w32 = np.asarray(w, dtype=np.float32).reshape(-1)
    v32 = np.asarray(v, dtype=np.float32)
    vz = (v32 == 0).all(axis=0) if v32.ndim == 2 and v32.shape[0] > 0 else np.ones(len(w32), dtype=bool)
    return vz & ((w32 == 0) | (not k1))


def seen_mask(n, ids):
    """bool [n]: the ids that stand in at least one entry (ids: the entry stream's ids, any order, repeats allowed)"""
    m = np.zeros(int(n), dtype=bool)
    m[np.asarray(ids, dtype=np.int64)] = True
    return m


def prune_mask(w, v, k1, seen=None):
    """bool [n]: the features a pruned snapshot keeps -- not dead, and (with seen, a bool [n]) seen"""
    keep = ~dead_mask(w, v, k1)
    if seen is not None:
        keep &= np.asarray(seen, dtype=bool)
    return keep


def directory(mask):
    """the rank directory of a keep mask: uint32 [ceil(n / 32)][2], column 0 = bits (bit b: id 32 j + b is kept), column 1 = base (the
    kept ids below 32 j)"""
    m = np.asarray(mask, dtype=bool).reshape(-1)
    nw = (len(m) + 31) // 32
    pad = np.zeros(nw * 32, dtype=np.uint64)
    pad[:len(m)] = m
    bits = (pad.reshape(nw, 32) << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    cnt = pad.reshape(nw, 32).sum(axis=1, dtype=np.uint64)
    base = np.cumsum(cnt) - cnt
    return np.stack([bits, base], axis=1).astype(np.uint32)


def _popc(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    c = np.zeros(x.shape, dtype=np.uint32)
    for _ in range(32):
        c += x & np.uint32(1)
        x >>= np.uint32(1)
    return c


def slot_of(dir, ids):
    """the slot of each id through the directory (one pair per id: base + popcount of the bits below it), SLOT_NONE for a dropped id"""
    d = np.asarray(dir, dtype=np.uint32).reshape(-1, 2)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    bits, base = d[ids >> 5, 0], d[ids >> 5, 1]
    b = (ids & 31).astype(np.uint32)
    below = bits & ((np.uint32(1) << b) - np.uint32(1))
    kept = ((bits >> b) & np.uint32(1)) != 0
    return np.where(kept, base + _popc(below), np.uint32(SLOT_NONE)).astype(np.uint32)


class CompactModel:
    """the snapshot of a model (w0, w[n], v[k][n]): w0 and w as given, v rounded to the format (bf16 | int8) from its fp32 value.
    keep (a bool [n], prune_mask): the pruned snapshot -- rows_w / rows_v hold the kept rows in slot order, dir is the directory, and
    w / v (what predict and rows read) are those rows looked up through it, +0 for a dropped id."""

    def __init__(self, w0, w, v, k0=True, k1=True, format="bf16", keep=None, seen=None):
        if format not in FORMATS:
            raise ValueError("unknown serving format %r (%s)" % (format, " | ".join(FORMATS)))
        self.format = format
        self.w0 = float(w0)
        self.keep = None
        if keep is not None:
            self._init_pruned(w, v, k0, k1, np.asarray(keep, dtype=bool).reshape(-1), seen)
            return
        self.w = np.array(w, dtype=np.float64)
        v32 = np.asarray(v, dtype=np.float32)
        if format == "int8" and v32.ndim == 2 and v32.shape[0] > 0:
            self.v = int8_round(v32).astype(np.float64)
        elif format == "int8":
            self.v = v32.astype(np.float64)
        else:
            self.v = bf16_round(v32).astype(np.float64)
        self.k0, self.k1 = bool(k0), bool(k1)
        self.k, self.n = (self.v.shape if self.v.ndim == 2 else (0, len(self.w)))

    def _init_pruned(self, w, v, k0, k1, keep, seen):
        w64 = np.array(w, dtype=np.float64).reshape(-1)
        v32 = np.asarray(v, dtype=np.float32)
        n = len(w64)
        if v32.ndim != 2 or v32.shape[0] == 0:
            v32 = np.zeros((0, n), dtype=np.float32)
        if len(keep) != n:
            raise ValueError("CompactModel: keep has %d entries for %d features" % (len(keep), n))
        self.keep = keep
        self.dir = directory(keep)
        kept_ids = np.flatnonzero(keep)
        packed = CompactModel(self.w0, w64[kept_ids], v32[:, kept_ids], k0, k1, self.format)    # the rows, in slot order
        self.rows_w, self.rows_v = packed.w, (packed.v if packed.v.ndim == 2 else np.zeros((0, len(kept_ids))))
        slots = slot_of(self.dir, np.arange(n))
        assert np.array_equal(slots[kept_ids], np.arange(len(kept_ids), dtype=np.uint32)) and np.all(slots[~keep] == SLOT_NONE)
        at = np.where(keep, slots, 0).astype(np.int64)
        zw, zv = np.append(self.rows_w, 0.0), np.concatenate([self.rows_v, np.zeros((v32.shape[0], 1))], axis=1)
        at[~keep] = len(kept_ids)                                        # a dropped id reads the row of +0 behind the kept ones
        self.w, self.v = zw[at], zv[:, at]
        self.k0, self.k1 = bool(k0), bool(k1)
        self.k, self.n = v32.shape[0], n
        dead = dead_mask(w64, v32, k1)
        gone_unseen = (~dead & ~np.asarray(seen, dtype=bool)) if seen is not None else np.zeros(n, dtype=bool)
        kept = int(keep.sum())
        self.prune_info = {"features": n, "kept": kept, "dropped_dead": int(dead.sum()), "dropped_unseen": int(gone_unseen.sum()),
                           "bytes_directory": 8 * ((n + 31) // 32), "bytes_rows": kept * row_bytes(self.format, self.k)}
        mx, ss, nf = quant_report(v32[:, kept_ids], self.format)                  # over the kept rows only
        self.info = {"features": n, "bytes_compact": self.prune_info["bytes_directory"] + self.prune_info["bytes_rows"],
                     "nonfinite": nf, "max_abs_err": mx, "sum_sq_err": ss}

    def slot_of(self, ids):
        return slot_of(self.dir, ids)

    def predict(self, entries, row_ptr):
        """raw scores of the rows (entries: structured id / value, row_ptr), fp64: fm_model::predict"""
        rp = np.asarray(row_ptr, dtype=np.int64)
        n = len(rp) - 1
        ids = entries["id"].astype(np.int64)
        xs = entries["value"].astype(np.float32).astype(np.float64)
        row = np.repeat(np.arange(n), np.diff(rp))
        out = np.full(n, self.w0 if self.k0 else 0.0)
        if self.k1:
            out += np.bincount(row, weights=self.w[ids] * xs, minlength=n)
        for f in range(self.k):
            d = self.v[f, ids] * xs
            s = np.bincount(row, weights=d, minlength=n)
            out += 0.5 * (s * s - np.bincount(row, weights=d * d, minlength=n))
        return out


# ---- the snapshot file (csrc/fmx_snap_format.h) ------------------------------------------------------------------------------
# Little-endian.  A 256-byte header:
#      0  char[8] magic b"FMXSNAP\0"
#      8  u32 version (1)          12  u32 format (1 bf16, 3 int8)
#     16  u64 num_attribute        24  u32 num_factor    28  u32 k0    32  u32 k1    36  u32 task
#     40  f64 min_target           48  f64 max_target
#     56  u32 pruned               60  u32 P (bytes of an int8 block; 0 for bf16)
#     64  u64 kept (0 unless pruned)
#     72  u64 nonfinite            80  f64 max_abs_err   88  f64 sum_sq_err
#     96  u64 dropped_dead        104  u64 dropped_unseen
#    112  u32 number of sections  116  u32 0
#    120  4 x {u32 kind, u32 0, u64 offset, u64 bytes, u64 checksum}, unused entries all zero
#    248  u64 checksum of bytes 0 .. 247
# then the sections in the order of their kinds, the first at byte 256, each padded with zero bytes to a multiple of 8
# (rows = kept when pruned, num_attribute otherwise):
#     1 w0 one f64     2 dir (pruned) [ceil(n / 32)] {u32 bits, u32 base}     3 rows (int8) [rows][P] bytes
#     4 w (bf16) [rows] f32     5 V (bf16) [rows][num_factor] u16
# The checksums are the checkpoint's (checkpoint.checksum).
SNAP_MAGIC = b"FMXSNAP\0"
SNAP_VERSION = 1
SNAP_HEADER_BYTES = 256
SNAP_MAX_SECTIONS = 4
SNAP_W0, SNAP_DIR, SNAP_ROWS, SNAP_W, SNAP_V = 1, 2, 3, 4, 5
SNAP_SECTION_NAMES = {SNAP_W0: "w0", SNAP_DIR: "dir", SNAP_ROWS: "rows", SNAP_W: "w", SNAP_V: "V"}
FORMAT_NAMES = {code: name for name, code in FORMATS.items()}


class SnapshotError(ValueError):
    pass


def _wave_sum(x):
    """wave_sum_d of fmx_kernels.h on [..., 64] lanes: x += x[lane ^ o] for o = 32, 16, ..., 1; every lane ends with the same sum"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ o]
    return x


def device_sum_sq(v, format="bf16", keep=None):
    """sum (v - q(v))^2 of a factor table v[k][n] with the partial sums added in the order of k_compact_quant / k_compact_quant8 and
    k_compact_final (fmx_compact_kernels.h), so that the result has fmx_compact_info::sum_sq_err's bits: L lanes share a feature and
    each adds its own coordinates in turn, the 64 lanes of a wavefront fold by a butterfly, the four wavefronts of a block as
    (0 + 1) + (2 + 3), and one wavefront folds the blocks -- lane l the blocks l, l + 64, ... in order -- and butterflies again.  Every
    squared error is exact in fp64 (bf16: the square of an fp32; int8: v and its dequantised value are fp32 values at most two binades
    apart), so only the order of the additions matters.  keep (bool [n]): the rows a pruned snapshot holds; the others add nothing."""
    v32 = np.ascontiguousarray(v, dtype=np.float32)
    if v32.ndim != 2 or v32.shape[0] == 0:
        return 0.0
    k, n = v32.shape
    with np.errstate(invalid="ignore", over="ignore"):
        if format == "int8":
            fin = np.isfinite(v32).all(axis=0)
            err = np.abs(v32.astype(np.float64) - int8_round(v32).astype(np.float64))
            err[:, ~fin] = 0.0
            p = row_bytes("int8", k)
            L = 2
            while L < 64 and L < p // 4:
                L <<= 1
        else:
            q = bf16_round(v32)
            err = np.where(np.isfinite(q), np.abs(v32 - q), np.float32(0)).astype(np.float64)
            kp = 1
            while kp < k:
                kp <<= 1
            L = min(kp, 64)
    if keep is not None:
        err[:, ~np.asarray(keep, dtype=bool).reshape(-1)] = 0.0
    sq = np.concatenate([err * err, np.zeros((1, n))], axis=0)      # row k: the zero a lane without a coordinate adds
    rpw = 64 // L
    waves = (n + rpw - 1) // rpw
    nblk = min((waves + 3) // 4, 8192)
    nwaves = nblk * 4
    lane = np.arange(64)
    grp, sub = lane // L, lane % L
    ss = np.zeros((nwaves, 64))
    wave = np.arange(nwaves)[:, None]
    for r0 in range(0, n, nwaves * rpw):
        j = wave * rpw + r0 + grp[None, :]
        live = j < n
        jj = np.where(live, j, 0)
        if format == "int8":
            for t in range(5):                                     # QUANT8_T dwords of the block per lane; dword d holds factors 4 (d - 2) ..
                d = sub + t * L
                for i in range(4):
                    f = 4 * (d - 2) + i
                    ok = (d >= 2) & (d < p // 4) & (f < k)
                    ss += np.where(live & ok[None, :], sq[np.where(ok, f, k)[None, :], jj], 0.0)
        else:
            for f0 in range(0, k, L):
                f = f0 + sub
                ok = f < k
                ss += np.where(live & ok[None, :], sq[np.where(ok, f, k)[None, :], jj], 0.0)
    per_wave = _wave_sum(ss)[:, 0].reshape(nblk, 4)
    part = (per_wave[:, 0] + per_wave[:, 1]) + (per_wave[:, 2] + per_wave[:, 3])
    fold = np.zeros(64)
    for b0 in range(0, nblk, 64):
        chunk = part[b0:b0 + 64]
        fold[:len(chunk)] += chunk
    return float(_wave_sum(fold)[0])


def device_quant_report(v, format="bf16", keep=None):
    """quant_report over the kept rows with the sum in the device's order: (max_abs_err, sum_sq_err, nonfinite) bit for bit as
    fmx_compact_info reports them"""
    v32 = np.ascontiguousarray(v, dtype=np.float32)
    if v32.ndim != 2 or v32.shape[0] == 0:
        return 0.0, 0.0, 0
    rows = v32 if keep is None else v32[:, np.asarray(keep, dtype=bool).reshape(-1)]
    mx, _, nf = quant_report(rows, format)
    return mx, device_sum_sq(v32, format, keep), nf


def int8_blocks(w, v):
    """the int8 snapshot's table: uint8 [n][P], one block per feature -- scale (f32), w (f32), the k codes, zeros up to P"""
    w32 = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    n = len(w32)
    v32 = np.asarray(v, dtype=np.float32)
    if v32.ndim != 2 or v32.shape[0] == 0:
        v32 = np.zeros((0, n), dtype=np.float32)
    k = v32.shape[0]
    codes, scale = int8_quant(v32)
    blocks = np.zeros((n, row_bytes("int8", k)), dtype=np.uint8)
    blocks[:, 0:4] = scale.astype("<f4").view(np.uint8).reshape(n, 4)
    blocks[:, 4:8] = w32.astype("<f4").view(np.uint8).reshape(n, 4)
    blocks[:, 8:8 + k] = codes.T.view(np.uint8)
    return blocks


def _snap_plan(format, n, k, pruned, kept, p):
    rows = kept if pruned else n
    secs, off = [], SNAP_HEADER_BYTES

    def add(kind, nbytes):
        nonlocal off
        secs.append((kind, off, nbytes))
        off += nbytes + (-nbytes % 8)
    add(SNAP_W0, 8)
    if pruned:
        add(SNAP_DIR, (n + 31) // 32 * 8)
    if format == FORMATS["int8"]:
        add(SNAP_ROWS, rows * p)
    else:
        add(SNAP_W, rows * 4)
        add(SNAP_V, rows * k * 2)
    return secs, off


def _snap_header(hd, table):
    head = bytearray(SNAP_HEADER_BYTES)
    head[0:8] = SNAP_MAGIC
    struct.pack_into("<IIQIIIIddIIQQddQQII", head, 8, SNAP_VERSION, hd["format"], hd["num_attribute"], hd["num_factor"], hd["k0"],
                     hd["k1"], hd["task"], hd["min_target"], hd["max_target"], hd["pruned"], hd["P"], hd["kept"], hd["nonfinite"],
                     hd["max_abs_err"], hd["sum_sq_err"], hd["dropped_dead"], hd["dropped_unseen"], len(table), 0)
    for i, (kind, off, nbytes, cs) in enumerate(table):
        struct.pack_into("<IIQQQ", head, 120 + 32 * i, kind, 0, off, nbytes, cs)
    struct.pack_into("<Q", head, 248, _checksum(head[:248]))
    return bytes(head)


def write_snapshot(path, w0, w, v, k0, k1, task, min_target, max_target, format, keep=None, seen=None):
    """write the snapshot file of the model (w0, w[n], v[k][n]) -- what fmx_compact_begin[_pruned] + fmx_compact_save write for it, byte
    for byte.  format: "bf16" | "int8" (or the FMX_COMPACT_* code).  keep (bool [n]): a pruned snapshot of exactly these rows; it has
    to be prune_mask(w, v, k1, seen), seen being the keep slot's seen_mask or None.  Returns the number of bytes."""
    fmt = FORMAT_NAMES.get(format, format)
    if fmt not in FORMATS:
        raise SnapshotError("unknown serving format %r (%s)" % (format, " | ".join(FORMATS)))
    w32 = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    n = len(w32)
    v32 = np.asarray(v, dtype=np.float32)
    if v32.ndim != 2 or v32.shape[0] == 0:
        v32 = np.zeros((0, n), dtype=np.float32)
    k = v32.shape[0]
    if v32.shape[1] != n or not 0 < n < 2 ** 32 or k > 1024:
        raise SnapshotError("w has %d entries, v the shape %r" % (n, v32.shape))
    pruned = keep is not None
    dd = du = 0
    ids = np.arange(n)
    body = {SNAP_W0: struct.pack("<d", float(w0))}
    if pruned:
        keep = np.asarray(keep, dtype=bool).reshape(-1)
        if len(keep) != n or not np.array_equal(keep, prune_mask(w32, v32, k1, seen)):
            raise SnapshotError("keep is not prune_mask(w, v, k1, seen): the header's counts would not add up")
        dead = dead_mask(w32, v32, k1)
        dd = int(dead.sum())
        du = int((~dead & ~np.asarray(seen, dtype=bool)).sum()) if seen is not None else 0
        ids = np.flatnonzero(keep)
        body[SNAP_DIR] = directory(keep).astype("<u4").tobytes()
    mx, ss, nf = device_quant_report(v32, fmt, keep)
    if fmt == "int8":
        body[SNAP_ROWS] = int8_blocks(w32[ids], v32[:, ids]).tobytes()
    else:
        body[SNAP_W] = w32[ids].astype("<f4").tobytes()
        body[SNAP_V] = np.ascontiguousarray(bf16_bits(v32[:, ids]).T).astype("<u2").tobytes()
    hd = dict(format=FORMATS[fmt], num_attribute=n, num_factor=k, k0=int(bool(k0)), k1=int(bool(k1)), task=int(task),
              min_target=float(min_target), max_target=float(max_target), pruned=int(pruned), P=row_bytes("int8", k) if fmt == "int8" else 0,
              kept=len(ids) if pruned else 0, nonfinite=nf, max_abs_err=mx, sum_sq_err=ss, dropped_dead=dd, dropped_unseen=du)
    secs, total = _snap_plan(hd["format"], n, k, pruned, hd["kept"], hd["P"])
    table = [(kind, off, nbytes, _checksum(body[kind])) for kind, off, nbytes in secs]
    with open(path, "wb") as f:
        f.write(_snap_header(hd, table))
        for kind, off, nbytes in secs:
            assert f.tell() == off and len(body[kind]) == nbytes
            f.write(body[kind] + b"\0" * (-nbytes % 8))
        assert f.tell() == total
    return total


def parse_snapshot_header(data, file_len=None):
    """the header of a file's first bytes (at least 256) as a dict: the fields above by name, rows, total (the planned length) and
    sections = [(kind, offset, bytes, checksum)].  Refuses what csrc/fmx_snap_format.h's parser refuses (SnapshotError names the
    field); with file_len, also a planned length other than it."""
    if len(data) < SNAP_HEADER_BYTES:
        raise SnapshotError("the file is shorter than a snapshot header")
    if data[0:8] != SNAP_MAGIC:
        raise SnapshotError("bad magic: not a snapshot file")
    names = ("version", "format", "num_attribute", "num_factor", "k0", "k1", "task", "min_target", "max_target", "pruned", "P", "kept",
             "nonfinite", "max_abs_err", "sum_sq_err", "dropped_dead", "dropped_unseen", "n_sections", "zero")
    hd = dict(zip(names, struct.unpack_from("<IIQIIIIddIIQQddQQII", data, 8)))
    if hd["version"] != SNAP_VERSION:
        raise SnapshotError("snapshot version %d, this module reads version %d" % (hd["version"], SNAP_VERSION))
    if struct.unpack_from("<Q", data, 248)[0] != _checksum(data[:248]):
        raise SnapshotError("the header's checksum does not match")
    n, k = hd["num_attribute"], hd["num_factor"]
    if hd["format"] not in FORMAT_NAMES:
        raise SnapshotError("unknown format %d" % hd["format"])
    if not 0 < n < 2 ** 32 or k > 1024 or hd["k0"] > 1 or hd["k1"] > 1 or hd["task"] > 1 or hd["pruned"] > 1 or hd["zero"]:
        raise SnapshotError("a geometry field (num_attribute, num_factor, k0, k1, task, pruned) is out of range")
    if hd["kept"] > n:
        raise SnapshotError("kept %d > num_attribute %d" % (hd["kept"], n))
    if not hd["pruned"] and hd["kept"]:
        raise SnapshotError("kept %d without pruned" % hd["kept"])
    if hd["P"] != (row_bytes("int8", k) if hd["format"] == FORMATS["int8"] else 0):
        raise SnapshotError("P (bytes of an int8 block) is %d, not what the format and num_factor imply" % hd["P"])
    if (not hd["pruned"] and (hd["dropped_dead"] or hd["dropped_unseen"])) or \
            (hd["pruned"] and hd["kept"] + hd["dropped_dead"] + hd["dropped_unseen"] != n):
        raise SnapshotError("kept + dropped_dead + dropped_unseen is not num_attribute")
    secs, total = _snap_plan(hd["format"], n, k, bool(hd["pruned"]), hd["kept"], hd["P"])
    table = [struct.unpack_from("<IIQQQ", data, 120 + 32 * i) for i in range(SNAP_MAX_SECTIONS)]
    want = [(kind, 0, off, nbytes) for kind, off, nbytes in secs] + [(0, 0, 0, 0)] * (SNAP_MAX_SECTIONS - len(secs))
    if hd["n_sections"] != len(secs) or [t[:4] for t in table] != want or any(t[4] for t in table[len(secs):]):
        raise SnapshotError("the section table does not match the header's fields")
    if file_len is not None and total != file_len:
        raise SnapshotError("the sections end at byte %d but the file has %d bytes (truncated?)" % (total, file_len))
    del hd["zero"]
    hd.update(rows=hd["kept"] if hd["pruned"] else n, total=total, sections=[(t[0], t[2], t[3], t[4]) for t in table[:len(secs)]],
              format_name=FORMAT_NAMES[hd["format"]])
    return hd


def snapshot_header(path):
    """the header of a snapshot file (parse_snapshot_header; the file's length is checked against the plan)"""
    import os
    with open(path, "rb") as f:
        data = f.read(SNAP_HEADER_BYTES)
    return parse_snapshot_header(data, os.path.getsize(path))


def check_directory(dir, n, kept):
    """what the device checks of a loaded directory (k_snap_dir_check): bases = the running popcounts from 0, no bit at or beyond n,
    total = kept"""
    d = np.asarray(dir, dtype=np.uint32).reshape(-1, 2)
    cnt = _popc(d[:, 0]).astype(np.uint64)
    base = np.cumsum(cnt) - cnt
    tail = n - 32 * (len(d) - 1)
    return bool(len(d) == (n + 31) // 32 and np.array_equal(d[:, 1].astype(np.uint64), base) and int(cnt.sum()) == kept and
                (tail == 32 or int(d[-1, 0]) >> tail == 0))


def read_snapshot(path):
    """read and verify a snapshot file (SnapshotError names what is wrong); returns (CompactModel, header): the model holds the file's
    tables -- for a pruned file rows_w / rows_v / dir / keep too -- and scores as the device does from them"""
    with open(path, "rb") as f:
        data = f.read()
    hd = parse_snapshot_header(data, len(data))
    n, k, rows = hd["num_attribute"], hd["num_factor"], hd["rows"]
    raw = {}
    for kind, off, nbytes, cs in hd["sections"]:
        raw[kind] = data[off:off + nbytes]
        if _checksum(raw[kind]) != cs or any(data[off + nbytes:off + nbytes + (-nbytes % 8)]):
            raise SnapshotError("section '%s': checksum mismatch" % SNAP_SECTION_NAMES[kind])
    if hd["format"] == FORMATS["int8"]:
        blocks = np.frombuffer(raw[SNAP_ROWS], dtype=np.uint8).reshape(rows, hd["P"])
        scale = np.ascontiguousarray(blocks[:, 0:4]).view("<f4").reshape(rows)
        rows_w = np.ascontiguousarray(blocks[:, 4:8]).view("<f4").reshape(rows).astype(np.float64)
        codes = np.ascontiguousarray(blocks[:, 8:8 + k]).view(np.int8).T
        rows_v = int8_dequant(codes, scale).astype(np.float64) if k else np.zeros((0, rows))
    else:
        rows_w = np.frombuffer(raw[SNAP_W], dtype="<f4").astype(np.float64)
        bits = np.frombuffer(raw[SNAP_V], dtype="<u2").reshape(rows, k).T.astype(np.uint32) << np.uint32(16)
        rows_v = np.ascontiguousarray(bits).view(np.float32).astype(np.float64)
    m = CompactModel.__new__(CompactModel)
    m.format, m.w0 = hd["format_name"], struct.unpack("<d", raw[SNAP_W0])[0]
    m.k0, m.k1, m.k, m.n, m.keep = bool(hd["k0"]), bool(hd["k1"]), k, n, None
    m.info = {"features": n, "nonfinite": hd["nonfinite"], "max_abs_err": hd["max_abs_err"], "sum_sq_err": hd["sum_sq_err"]}
    if not hd["pruned"]:
        m.w, m.v = rows_w, (rows_v if k else np.zeros((0, n)))
        return m, hd
    m.dir = np.frombuffer(raw[SNAP_DIR], dtype="<u4").reshape(-1, 2).astype(np.uint32)
    if not check_directory(m.dir, n, rows):
        raise SnapshotError("section 'dir': the directory is not consistent with num_attribute and kept")
    slots = slot_of(m.dir, np.arange(n))
    m.keep = slots != SLOT_NONE
    m.rows_w, m.rows_v = rows_w, rows_v
    at = np.where(m.keep, slots, rows).astype(np.int64)              # a dropped id reads the row of +0 behind the kept ones
    m.w, m.v = np.append(rows_w, 0.0)[at], np.concatenate([rows_v, np.zeros((k, 1))], axis=1)[:, at]
    m.prune_info = {"features": n, "kept": rows, "dropped_dead": hd["dropped_dead"], "dropped_unseen": hd["dropped_unseen"],
                    "bytes_directory": 8 * ((n + 31) // 32), "bytes_rows": rows * row_bytes(m.format, k)}
    m.info["bytes_compact"] = m.prune_info["bytes_directory"] + m.prune_info["bytes_rows"]
    return m, hd
