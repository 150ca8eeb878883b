"""CPU: the int8 row-wise format of the serving snapshot (FMX_COMPACT_INT8; include/fmx.h) as libfm_amd/compact.py
restates it, and what of it can be checked without a device: the properties of the symmetric code, the bytes of a block, the report,
CompactModel against the fp64 oracle, the exported helper, the ABI version and the CLI's refusals.

The error bound.  For a finite row with a = max |v_f| and step = a / 127 (fp64): the code is q = rint(v / step) up to the fp64
roundings of 127 / a and of the product, each 2^-53 relative on a quotient of at most 127, so |v - step q| <= step (0.5 + 2^-44).
The stored scale is fl32(step) = step (1 + d1) and the value fl32(scale q) = scale q (1 + d2), |d1|, |d2| <= u = 2^-24, |q| <= 127:
|step q - deq| <= 127 step (2 u + u^2).  Together |v - deq| <= step (0.5 + EPS), EPS = 127 (2 u + u^2) + 2^-44 = 1.514e-5.  Where scale
or the product is an fp32 subnormal a rounding is absolute, at most 2^-150 each, 127 of the first and one of the second: + 128 * 2^-150."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

U32 = 2.0 ** -24
EPS = 127.0 * (2.0 * U32 + U32 * U32) + 2.0 ** -44
TINY = 128.0 * 2.0 ** -150
ROW_BYTES = {0: 8, 1: 16, 8: 16, 9: 32, 24: 32, 25: 64, 56: 64, 57: 128, 64: 128, 120: 128, 121: 192, 128: 192, 256: 320, 1000: 1024}


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def table(seed, k=None, n=64):
    """a seeded [k][n] table: every feature (column) has a binade of its own out of the whole fp32 exponent range, zeros are planted, and
    the first columns are the special rows: all zero, subnormal, a / 127 underflowing to 0, one +inf, one -inf, one NaN"""
    rng = np.random.default_rng(seed)
    k = int(rng.integers(1, 131)) if k is None else k
    expo = rng.integers(-140, 120, size=n).astype(np.float64)
    v = (rng.standard_normal((k, n)) * 2.0 ** expo[None, :]).astype(np.float32)
    v[rng.random((k, n)) < 0.15] = 0.0
    v[:, 0] = 0.0                                              # an all-zero row
    v[:, 1] = f32(rng.integers(1, 0x00800000, size=k, dtype=np.uint64).astype(np.uint32))     # a subnormal row
    v[:, 2] = 0.0
    v[0, 2] = f32(0x00000007)                                  # a = 7 * 2^-149: a / 127 is below half the smallest subnormal
    v[k - 1, 3] = np.inf
    v[0, 4] = -np.inf
    v[k // 2, 5] = np.nan
    v[0, 6] = -0.0
    return v


SPECIAL_NONFINITE = (3, 4, 5)


@pytest.mark.parametrize("seed", range(24))
def test_properties_of_the_symmetric_code(seed):
    from libfm_amd import compact
    v = table(seed)
    k, n = v.shape
    q, s = compact.int8_quant(v)
    d = compact.int8_dequant(q, s)
    assert q.dtype == np.int8 and q.shape == (k, n) and s.dtype == np.float32 and s.shape == (n,) and d.dtype == np.float32
    fin = np.isfinite(v).all(axis=0)
    assert list(np.nonzero(~fin)[0]) == list(SPECIAL_NONFINITE)
    # rows with a non-finite factor: scale NaN, codes 0, every factor NaN
    assert np.all(np.isnan(s[~fin])) and not np.any(q[:, ~fin]) and np.all(np.isnan(d[:, ~fin]))
    assert np.all(np.isfinite(s[fin])) and np.all(np.isfinite(d[:, fin]))
    vf, qf, sf, df = v[:, fin], q[:, fin], s[fin], d[:, fin]
    a = np.abs(vf.astype(np.float64)).max(axis=0)
    # an exactly-zero factor stays exactly zero; an all-zero row has scale 0
    assert np.all(df[vf == 0] == 0) and np.all(qf[vf == 0] == 0)
    assert np.all(sf[a == 0] == 0) and s[0] == 0
    # the largest factor of a non-zero row has code +-127, no code is -128
    assert np.all(np.abs(qf.astype(np.int32)).max(axis=0)[a > 0] == 127) and qf.min() >= -127
    big = np.abs(vf.astype(np.float64)) == a[None, :]
    assert np.all(np.abs(qf.astype(np.int32))[big & (a[None, :] > 0)] == 127)
    # the error bound of the docstring
    step = a / 127.0
    err = np.abs(vf.astype(np.float64) - df.astype(np.float64))
    assert np.all(err <= step[None, :] * (0.5 + EPS) + TINY)
    normal = sf >= np.finfo(np.float32).tiny * 2 ** 8          # scale and every non-zero product normal: the relative bound alone
    assert np.all(err[:, normal] <= step[None, normal] * (0.5 + EPS))
    # quantising the dequantised table again returns the same values, and the same codes and scale wherever scale > 0
    q2, s2 = compact.int8_quant(df)
    d2 = compact.int8_dequant(q2, s2)
    assert np.array_equal(d2.view(np.uint32), df.view(np.uint32))
    live = sf > 0
    assert np.array_equal(q2[:, live], qf[:, live]) and np.array_equal(s2[live].view(np.uint32), sf[live].view(np.uint32))
    # the row whose a / 127 underflows: scale 0, everything 0
    assert s[2] == 0 and not np.any(d[:, 2])
    assert np.array_equal(compact.int8_round(v).view(np.uint32), d.view(np.uint32))


def test_ties_round_to_even_and_the_codes_are_signed():
    from libfm_amd import compact
    # a = 127: step 1, inv 1 -- the codes are rint(v)
    v = np.array([[127.0], [0.5], [1.5], [2.5], [-0.5], [-1.5], [-126.5], [126.5], [-127.0], [0.49999997], [3.0]], dtype=np.float32)
    q, s = compact.int8_quant(v)
    assert s[0] == 1.0
    assert list(q[:, 0]) == [127, 0, 2, 2, 0, -2, -126, 126, -127, 0, 3]
    assert np.array_equal(compact.int8_dequant(q, s)[:, 0], q[:, 0].astype(np.float32))
    assert compact.int8_quant(np.zeros((0, 4), dtype=np.float32))[0].shape == (0, 4)


def test_row_bytes():
    from libfm_amd import compact
    for k, want in ROW_BYTES.items():
        assert compact.row_bytes("int8", k) == want == compact.row_bytes(compact.FORMATS["int8"], k), k
    for k in range(0, 1100):
        p = compact.row_bytes("int8", k)
        assert p >= k + 8 and p % 8 == 0
        assert (p & (p - 1)) == 0 and p < 2 * (k + 8) if k + 8 <= 128 else p % 64 == 0 and p - (k + 8) < 64
    assert [compact.row_bytes("bf16", k) for k in (0, 1, 8, 32, 64, 100, 128, 300, 1000)] == [6, 6, 20, 68, 132, 228, 260, 612, 2020]
    assert compact.row_bytes("fp8", 8) == 0 and compact.row_bytes(2, 8) == 0 and compact.row_bytes("int8", -1) == 0
    assert compact.FORMATS == {"bf16": 1, "int8": 3}


def test_quant_report_int8():
    from libfm_amd import compact
    # three features (columns): a = 127 with one tie and one off-grid value; one with an inf; one all zero
    v = np.array([[127.0, np.inf, 0.0], [0.5, 1.0, 0.0], [3.25, 2.0, 0.0]], dtype=np.float32)
    mx, ss, nf = compact.quant_report(v, format="int8")
    assert nf == 3                                             # all k coordinates of the row with the inf
    assert mx == 0.5 and ss == 0.5 ** 2 + 0.25 ** 2
    assert compact.quant_report(v[:, 2:], "int8") == (0.0, 0.0, 0)
    assert compact.quant_report(np.zeros((0, 5), dtype=np.float32), "int8") == (0.0, 0.0, 0)
    assert compact.quant_report(v) == compact.quant_report(v, format="bf16")          # the default is bf16, as it was
    with pytest.raises(ValueError):
        compact.quant_report(v, format="fp8")


@pytest.mark.parametrize("k, k0, k1", [(0, True, True), (1, True, True), (8, True, False), (5, False, True), (64, True, True)])
def test_compact_model_int8_predicts_as_the_oracle_from_the_dequantised_factors(oracle, k, k0, k1):
    from libfm_amd import compact
    rng = np.random.default_rng(21 + k)
    n, rows = 97, 40
    sizes = rng.integers(0, 9, size=rows)
    sizes[:3] = (0, 1, 8)
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ent = np.zeros(int(rp[-1]), dtype=oracle.ENTRY_DTYPE)
    ent["id"] = rng.integers(0, n, size=len(ent))
    ent["value"] = rng.standard_normal(len(ent)).astype(np.float32)
    ent["id"][int(rp[2]):int(rp[2]) + 2] = 5                          # row 2 repeats an id
    m = oracle.Model(n, k, k0, k1)
    m.w0, m.w[:], m.v[:] = 0.3, rng.standard_normal(n), rng.standard_normal((k, n)) * 0.3
    cm = compact.CompactModel(m.w0, m.w, m.v, k0, k1, format="int8")
    assert cm.format == "int8" and cm.w0 == m.w0 and np.array_equal(cm.w, m.w) and cm.k == k
    if k:
        assert np.array_equal(cm.v, compact.int8_round(m.v.astype(np.float32)).astype(np.float64))
    if k >= 5:                                                        # (k = 1: a row's only factor is its maximum, code 127)
        assert np.abs(cm.v - m.v).max() > 1e-4                        # (the rounding is visible at this scale)
    mq = m.copy()
    mq.v[:] = cm.v
    want = oracle.predict_raw(mq, oracle.Data(ent, rp, np.zeros(rows, dtype=np.float32)))
    np.testing.assert_allclose(cm.predict(ent, rp), want, rtol=1e-12, atol=1e-13)
    assert compact.CompactModel(m.w0, m.w, m.v, k0, k1).format == "bf16"               # the default is bf16, as it was
    with pytest.raises(ValueError):
        compact.CompactModel(m.w0, m.w, m.v, format="fp8")


@pytest.fixture(scope="module")
def lib():
    from libfm_amd import build, capi
    build.build()
    return capi.load()


def test_row_bytes_is_exported_and_equals_the_python_rule(lib):
    from libfm_amd import capi, compact
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    assert re.search(r"\buint32_t\s+fmx_compact_row_bytes\s*\(\s*uint32_t format\s*,\s*int num_factor\s*\)\s*;", txt)
    assert re.search(r"#define\s+FMX_COMPACT_INT8\s+3u", txt) and capi.COMPACT_INT8 == 3 and capi.COMPACT_BF16 == 1
    bound = {name: (res, args) for name, res, args in capi.SYMBOLS}
    assert bound["fmx_compact_row_bytes"] == (C.c_uint32, [C.c_uint32, C.c_int])
    for k, want in ROW_BYTES.items():
        assert lib.fmx_compact_row_bytes(capi.COMPACT_INT8, k) == want, k
    for k in range(0, 1100):
        assert lib.fmx_compact_row_bytes(capi.COMPACT_INT8, k) == compact.row_bytes("int8", k), k
        assert lib.fmx_compact_row_bytes(capi.COMPACT_BF16, k) == compact.row_bytes("bf16", k), k
    for fmt in (0, 2, 4, 99):
        assert lib.fmx_compact_row_bytes(fmt, 8) == 0
    assert lib.fmx_compact_row_bytes(capi.COMPACT_INT8, -1) == 0


def test_abi_version_is_still_11(lib):
    assert lib.fmx_abi_version() == 11


def test_a_null_handle_is_refused_for_int8_too(lib):
    from libfm_amd import capi
    opts, info = capi.CompactOpts(capi.COMPACT_INT8, 0), capi.CompactInfo()
    assert lib.fmx_compact_begin(None, C.byref(opts), C.byref(info)) == -1


@pytest.mark.parametrize("argv, text", [
    (["-method", "sgd", "-serve", "fp8"], "ERROR: -serve knows bf16, not 'fp8' (also: int8)"),
    (["-method", "sgd", "-serve", "int4"], "ERROR: -serve knows bf16, not 'int4' (also: int8)"),
    (["-method", "mcmc", "-serve", "int8"], "ERROR: -serve is not supported with -method mcmc"),
    (["-serve", "int8"], "ERROR: -serve is not supported with -method mcmc"),                     # (mcmc is the default method)
    (["-method", "als", "-serve", "int8", "-relation", "rel"], "ERROR: -serve is not supported with -relation"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    # (the files do not exist: a refusal that came later than the argument checks would be a different error)
    assert cli.main(["-task", "r", "-train", "no_such_train", "-test", "no_such_test", "-learn_rate", "0.01"] + argv) == 0
    assert text in capsys.readouterr().err


def test_cli_accepts_int8_up_to_the_missing_file(capsys):
    from libfm_amd import cli
    cli.main(["-task", "r", "-train", "no_such_train", "-test", "no_such_test", "-learn_rate", "0.01", "-method", "sgd", "-serve", "int8"])
    assert "-serve" not in capsys.readouterr().err


def test_learner_views_take_the_format():
    from libfm_amd import learner as L
    with pytest.raises(ValueError, match="unknown serving format"):
        L.CompactView(L.FMLearnSGD(), "int4")
