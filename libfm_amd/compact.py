"""fp64 / bit-level restatement of the bf16 serving snapshot (include/fmx.h "fmx_compact_*").  CPU only.

bf16 is the upper half of an fp32.  bf16_round rounds to nearest, ties to even, on bit 16: for a bit pattern u that is not a NaN

    q = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000

so +-0, +-inf and the fp32 subnormals follow the same rule and a finite value above bf16's largest carries into the exponent and
becomes +-inf.  A NaN stays a NaN: its upper half with the quiet bit set.

CompactModel is what fmx_compact_begin freezes -- w0 and w unchanged, V rounded -- and predicts in fp64 by fm_model::predict
(fm_model.h:105-127), the formula the fp64 oracle's predict_raw restates.  quant_report gives the three numbers of fmx_compact_info.
"""
import numpy as np

FORMATS = {"bf16": 1}      # FMX_COMPACT_*: fmx_compact_opts::format


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


def quant_report(v):
    """(max |v - q(v)|, sum (v - q(v))^2, nonfinite) of a factor table as the device holds it (float32): the maximum and the sum run
    over the coordinates whose bf16 value is finite, nonfinite counts the others.  v - q(v) is exact in fp32."""
    v32 = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    q = bf16_round(v32)
    fin = np.isfinite(q)
    with np.errstate(invalid="ignore"):
        err = np.abs(v32[fin] - q[fin]).astype(np.float64)
    return (float(err.max()) if err.size else 0.0), float(np.sum(err * err)), int((~fin).sum())


class CompactModel:
    """the snapshot of a model (w0, w[n], v[k][n]): w0 and w as given, v rounded to bf16 from its fp32 value"""

    def __init__(self, w0, w, v, k0=True, k1=True):
        self.w0 = float(w0)
        self.w = np.array(w, dtype=np.float64)
        self.v = bf16_round(np.asarray(v, dtype=np.float32)).astype(np.float64)
        self.k0, self.k1 = bool(k0), bool(k1)
        self.k, self.n = (self.v.shape if self.v.ndim == 2 else (0, len(self.w)))

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
