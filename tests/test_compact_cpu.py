"""CPU: the bf16 format of the serving snapshot and its restatement (libfm_amd/compact.py), and what of fmx_compact_* can be checked
without a device: the declarations, the binding, the ABI version, the refusals of a NULL handle and the CLI's refusals.

bf16_round is pinned bit for bit to torch's float32 -> bfloat16 -> float32 conversion on the CPU (round to nearest, ties to even):
two independent statements of the format."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FUNCTIONS = {
    "fmx_compact_begin": "fmx_handle h, const fmx_compact_opts *opts, fmx_compact_info *info",
    "fmx_compact_predict": "fmx_handle h, int slot, double *out",
    "fmx_compact_evaluate": "fmx_handle h, int slot, fmx_eval *out",
    "fmx_compact_evaluate_ex": "fmx_handle h, int slot, const fmx_eval_opts *opts, fmx_eval_ex *out",
    "fmx_compact_topk": "fmx_handle h, int query_slot, int cand_slot, const fmx_topk_opts *opts, uint32_t *idx_out, double *score_out, "
                        "fmx_topk_stats *stats",
    "fmx_compact_get_rows": "fmx_handle h, const uint32_t *ids, uint32_t count, double *w_out, double *v_out",
    "fmx_compact_end": "fmx_handle h",
}


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def planted():
    """(values, what each must round to or None): the ties, +-0, fp32 subnormals, the overflow to inf, +-inf"""
    cases = [
        (np.float32(1.0 + 2.0 ** -8), np.float32(1.0)),                        # a tie: down to the even mantissa
        (np.float32(1.0 + 3.0 * 2.0 ** -8), np.float32(1.0 + 2.0 ** -6)),      # a tie: up to the even mantissa
        (np.float32(0.0), np.float32(0.0)), (np.float32(-0.0), np.float32(-0.0)),
        (f32(0x00000001), np.float32(0.0)),                                    # the smallest subnormal: below half a bf16 step
        (f32(0x00008000), np.float32(0.0)),                                    # a tie between 0 and the smallest bf16 subnormal: even
        (f32(0x00008001), f32(0x00010000)),                                    # just above that tie
        (f32(0x007FFFFF), f32(0x00800000)),                                    # the largest subnormal carries into the normals
        (f32(0x80018000), f32(0x80020000)),                                    # a negative subnormal tie: up to the even
        (np.float32(3.4e38), np.float32(np.inf)), (np.float32(-3.4e38), np.float32(-np.inf)),
        (np.float32(np.inf), np.float32(np.inf)), (np.float32(-np.inf), np.float32(-np.inf)),
    ]
    return np.array([c[0] for c in cases], dtype=np.float32), np.array([c[1] for c in cases], dtype=np.float32)


def sample(n=100000, seed=7):
    """seeded values over the whole exponent range, both signs"""
    rng = np.random.default_rng(seed)
    wide = rng.integers(0, 2 ** 32, size=n // 2, dtype=np.uint64).astype(np.uint32).view(np.float32)
    near = (rng.standard_normal(n - n // 2) * 0.1).astype(np.float32)
    x = np.concatenate([wide, near])
    return x[~np.isnan(x)]


def test_bf16_round_matches_torch_bit_for_bit():
    import torch
    from libfm_amd import compact
    px, want = planted()
    x = np.concatenate([sample(), px])
    got = compact.bf16_round(x)
    ref = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    assert got.dtype == np.float32 and got.shape == x.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(got[-len(px):].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(compact.bf16_bits(x), (got.view(np.uint32) >> 16).astype(np.uint16))
    assert not np.any(got.view(np.uint32) & 0xFFFF)


def test_nan_stays_nan_with_the_quiet_bit():
    import torch
    from libfm_amd import compact
    nans = f32([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFF80FFFF, 0x7FFFFFFF])
    got = compact.bf16_round(nans)
    assert np.all(np.isnan(got))
    assert np.all(compact.bf16_bits(nans) & 0x0040)
    assert np.all(np.isnan(torch.from_numpy(nans.copy()).to(torch.bfloat16).to(torch.float32).numpy()))
    assert np.array_equal(np.signbit(got), np.signbit(nans))


def test_idempotent_and_relative_error():
    from libfm_amd import compact
    x = np.concatenate([sample(), planted()[0]])
    q = compact.bf16_round(x)
    assert np.array_equal(compact.bf16_round(q).view(np.uint32), q.view(np.uint32))
    normal = np.isfinite(q) & (np.abs(x) >= np.finfo(np.float32).tiny)
    xd, qd = x[normal].astype(np.float64), q[normal].astype(np.float64)
    assert np.all(np.abs(xd - qd) <= 2.0 ** -8 * np.abs(xd))
    assert np.max(np.abs(xd - qd) / np.abs(xd)) > 2.0 ** -9.5         # (and the bound is the format's, not a loose one)


def test_quant_report():
    from libfm_amd import compact
    v = np.array([[1.0 + 2.0 ** -8, -0.5, 3.4e38], [np.inf, 0.1, np.nan]], dtype=np.float32)
    mx, ss, nf = compact.quant_report(v)
    e = abs(float(np.float32(0.1)) - float(compact.bf16_round(np.float32(0.1))))
    assert nf == 3
    assert mx == 2.0 ** -8
    assert ss == pytest.approx(2.0 ** -16 + e * e, rel=1e-15)
    assert compact.quant_report(np.zeros((0, 5), dtype=np.float32)) == (0.0, 0.0, 0)


@pytest.mark.parametrize("k, k0, k1", [(0, True, True), (1, True, True), (8, True, False), (5, False, True)])
def test_compact_model_predicts_as_the_oracle_from_the_rounded_factors(oracle, k, k0, k1):
    """CompactModel keeps w0 and w, rounds v, and predicts as the pinned fp64 restatement (oracle.predict_raw) fed those values"""
    from libfm_amd import compact
    rng = np.random.default_rng(11 + k)
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
    cm = compact.CompactModel(m.w0, m.w, m.v, k0, k1)
    assert cm.w0 == m.w0 and np.array_equal(cm.w, m.w)
    assert np.array_equal(cm.v, compact.bf16_round(m.v.astype(np.float32)).astype(np.float64))
    if k:
        assert np.abs(cm.v - m.v).max() > 1e-4                        # (the rounding is visible at this scale)
    mq = m.copy()
    mq.v[:] = cm.v
    want = oracle.predict_raw(mq, oracle.Data(ent, rp, np.zeros(rows, dtype=np.float32)))
    np.testing.assert_allclose(cm.predict(ent, rp), want, rtol=1e-12, atol=1e-13)


def header_text():
    txt = open(os.path.join(ROOT, "include", "fmx.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_and_capi_binds_the_seven_functions():
    from libfm_amd import capi
    txt = header_text()
    ctype = {"fmx_handle": C.c_void_p, "int": C.c_int, "uint32_t": C.c_uint32}
    structs = {"fmx_compact_opts": capi.CompactOpts, "fmx_compact_info": capi.CompactInfo, "fmx_eval": capi.Eval,
               "fmx_eval_opts": capi.EvalOpts, "fmx_eval_ex": capi.EvalEx, "fmx_topk_opts": capi.TopkOpts, "fmx_topk_stats": capi.TopkStats}
    bound = {name: (res, args) for name, res, args in capi.SYMBOLS}
    for name, params in FUNCTIONS.items():
        mt = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert mt, name
        got = [" ".join(p.split()) for p in mt.group(1).split(",")]
        assert got == [" ".join(p.split()) for p in params.split(",")], name
        res, args = bound[name]
        assert res is C.c_int and len(args) == len(got), name
        for p, a in zip(got, args):
            base = p.replace("const ", "").split()[0]
            if "*" not in p:
                assert a is ctype[base], (name, p)
            elif base in structs:
                assert a is C.POINTER(structs[base]), (name, p)
            else:
                assert a is C.c_void_p, (name, p)              # arrays of scalars travel as addresses
    assert re.search(r"#define\s+FMX_COMPACT_BF16\s+1u", txt) and capi.COMPACT_BF16 == 1
    assert C.sizeof(capi.CompactOpts) == 8 and [f for f, _ in capi.CompactOpts._fields_] == ["format", "flags"]
    assert C.sizeof(capi.CompactInfo) == 48 and [f for f, _ in capi.CompactInfo._fields_] == [
        "features", "bytes_compact", "bytes_params", "nonfinite", "max_abs_err", "sum_sq_err"]
    for m in ("compact_begin", "compact_predict", "compact_evaluate", "compact_evaluate_ex", "compact_topk", "compact_rows", "compact_end"):
        assert callable(getattr(capi.Handle, m))


@pytest.fixture(scope="module")
def lib():
    from libfm_amd import build, capi
    build.build()
    return capi.load()


def test_abi_version_is_still_11(lib):
    assert lib.fmx_abi_version() == 11
    assert re.search(r"#define\s+FMX_ABI_VERSION\s+11\b", open(os.path.join(ROOT, "include", "fmx.h")).read())
    for name in FUNCTIONS:
        assert hasattr(lib, name), name


def test_bad_arguments_are_rejected_before_touching_the_device(lib):
    """without a handle there is nothing to score and nowhere to leave a message: FMX_E_ARG, whatever else is passed"""
    from libfm_amd import capi
    opts, info = capi.CompactOpts(capi.COMPACT_BF16, 0), capi.CompactInfo()
    buf = np.zeros(4, dtype=np.float64)
    ids = np.zeros(1, dtype=np.uint32)
    ev, evx, eo = capi.Eval(), capi.EvalEx(), capi.EvalOpts(0, 0)
    to, ts = capi.TopkOpts(1, 0, 0, 1, 0, None, None), capi.TopkStats()
    assert lib.fmx_compact_begin(None, C.byref(opts), C.byref(info)) == -1
    assert lib.fmx_compact_begin(None, None, None) == -1
    assert lib.fmx_compact_predict(None, 0, buf.ctypes.data) == -1
    assert lib.fmx_compact_evaluate(None, 0, C.byref(ev)) == -1
    assert lib.fmx_compact_evaluate_ex(None, 0, C.byref(eo), C.byref(evx)) == -1
    assert lib.fmx_compact_topk(None, 0, 1, C.byref(to), ids.ctypes.data, buf.ctypes.data, C.byref(ts)) == -1
    assert lib.fmx_compact_get_rows(None, ids.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data) == -1
    assert lib.fmx_compact_end(None) == -1


@pytest.mark.parametrize("argv, text", [
    (["-method", "sgd", "-serve", "fp8"], "ERROR: -serve knows bf16, not 'fp8'"),
    (["-method", "als", "-serve", "fp16"], "ERROR: -serve knows bf16, not 'fp16'"),
    (["-method", "sgd", "-serve"], "ERROR: -serve knows bf16, not ''"),
    (["-method", "mcmc", "-serve", "bf16"], "ERROR: -serve is not supported with -method mcmc"),
    (["-serve", "bf16"], "ERROR: -serve is not supported with -method mcmc"),                     # (mcmc is the default method)
    (["-method", "als", "-serve", "bf16", "-relation", "rel"], "ERROR: -serve is not supported with -relation"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    # (the files do not exist: a refusal that came later than the argument checks would be a different error)
    assert cli.main(["-task", "r", "-train", "no_such_train", "-test", "no_such_test", "-learn_rate", "0.01"] + argv) == 0
    assert text in capsys.readouterr().err


def test_learners():
    from libfm_amd import learner as L
    for cls in (L.FMLearnSGD, L.FMLearnSGDA, L.FMLearnPairSGD, L.FMLearnALS):
        assert callable(cls.compact)
    with pytest.raises(NotImplementedError, match="average over the draws"):
        L.FMLearnMCMC().compact()
    with pytest.raises(ValueError, match="unknown serving format"):
        L.CompactView(L.FMLearnSGD(), "fp16")
    for m in ("predict", "evaluate", "evaluate_ex", "recommend", "close"):
        assert callable(getattr(L.CompactView, m))
