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
"""
import numpy as np

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
