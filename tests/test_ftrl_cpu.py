"""CPU: the numpy restatement of FTRL-proximal with L1 on the minibatch rule (libfm_amd/ftrl.py) -- pinned to the AdaGrad restatement
by the identity of include/fmx.h, to literals worked out from the formulas, to its start state and to the hot-feature case -- and the
command line's and the learners' refusals around -optimizer ftrl.  The device path is held to this restatement in
tests/test_gpu_ftrl.py, which takes its absolute tolerances on z and n from ftrl_gaps() below."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from test_adagrad_cpu import hot_case

PARITY = dict(alpha=0.05, beta=1.0, l1_w=0.5, l1_v=0.3, l2_w=0.01, l2_v=0.01)     # the options of the device's parity tests


def parity_case(k, k0=True, k1=True, n=6400, rows=512, nnz=32):
    d = O.synth_rows(7, 0, rows, nnz, n)
    m = O.Model(n, k, k0, k1, 0.01, 0.002, 0.001)
    m.v[:] = O.init_values(1, n, k, 0.05)
    if k1:
        m.w[:] = O.init_values(2, n, 1, 0.02)[0]
    m.w0 = 0.03 if k0 else 0.0
    return d, m


def ftrl_gaps(d, m, task, lr, batch, chunk, epochs, opts):
    """largest absolute gaps (theta, z, n) between the restatement in fp32 and in fp64 after `epochs` epochs: what rounding alone costs
    at this shape.  n starts at init_acc (0 by default), so a gradient sum that cancels leaves an n whose RELATIVE gap is unbounded: the
    device tests take their absolute term on z and n from here."""
    from libfm_amd import ftrl
    res = []
    for dt in (np.float64, np.float32):
        c = m.copy()
        st = ftrl.FtrlState(c, **opts)
        for _ in range(epochs):
            ftrl.epoch(c, d, task, lr, -1.0, 1.0, batch, chunk, st, dtype=dt)
        res.append((c, st))
    (a, sa), (b, sb) = res

    def gap(x, y):
        return float(np.abs(x - y).max()) if x.size else 0.0
    return (max(gap(a.v, b.v), gap(a.w, b.w)), max(gap(sa.z_v, sb.z_v), gap(sa.z_w, sb.z_w)), max(gap(sa.n_v, sb.n_v), gap(sa.n_w, sb.n_w)))


@pytest.mark.parametrize("task", [0, 1])
def test_adagrad_identity(task):
    """l1 = l2 = beta = 0, init_acc = a > 0, alpha = eta, regw = regv = 0: the rule IS AdaGrad (theta' = theta - eta g / sqrt(n'))"""
    from libfm_amd import adaptive, ftrl
    n, k, eta, a0 = 6400, 8, 0.05, 0.5
    d = O.synth_rows(7, 0, 512, 32, n)
    m = O.Model(n, k, True, True, 0.01, 0.0, 0.0)
    m.v[:] = O.init_values(1, n, k, 0.05)
    m.w[:] = O.init_values(2, n, 1, 0.02)[0]
    a, b = m.copy(), m.copy()
    sa = adaptive.AdaptState(n, k, a0)
    sb = ftrl.FtrlState(b, eta, 0.0, init_acc=a0)
    for _ in range(3):
        adaptive.epoch(a, d, task, 0.01, -1.0, 1.0, 64, 16, sa, eta=eta)
        ftrl.epoch(b, d, task, 0.01, -1.0, 1.0, 64, 16, sb)
    print("gaps: v %.3g  w %.3g  n_v %.3g" % (np.abs(a.v - b.v).max(), np.abs(a.w - b.w).max(), np.abs(sa.n_v - sb.n_v).max()))
    np.testing.assert_allclose(b.v, a.v, rtol=1e-9)
    np.testing.assert_allclose(b.w, a.w, rtol=1e-9)
    np.testing.assert_allclose(b.w0, a.w0, rtol=1e-9)
    np.testing.assert_allclose(sb.n_v, sa.n_v, rtol=1e-9)
    np.testing.assert_allclose(sb.n_w, sa.n_w, rtol=1e-9)
    assert np.abs(a.v - m.v).max() > 1e-3                        # (the epochs moved something)


def test_hand_sized_case():
    """two rows that share feature 0, row 1 repeats id 2, feature 3 is never touched; k = 2, regression, one batch per epoch, the bias
    in one micro-chunk; two epochs (z and n carry over).  Every number below is the formula written out.  w_1 is driven to exactly 0
    by l1_w in the first epoch and revived, with the other sign, in the second."""
    from libfm_amd import ftrl
    rows = [[(0, 1.0), (1, 2.0)], [(0, 0.5), (2, 1.0), (2, -1.5)]]
    y = [0.7, -0.4]
    lr, alpha, beta, reg0, init_acc = 0.1, 0.3, 1.0, 0.01, 0.25
    l1 = {"w": 0.25, "v": 0.004}
    l2 = {"w": 0.02, "v": 0.03}
    w0, w = 0.05, [0.1, -0.15, 0.3, 0.4]
    v = [[0.1, -0.1, 0.2, 0.5], [0.05, 0.15, -0.05, -0.3]]     # [f][j]
    d = O.Data.from_rows(rows, np.array(y, dtype=np.float32))
    y = [float(t) for t in d.target]                             # (the targets as the data holds them: fp32)
    m = O.Model(4, 2, True, True, reg0, 0.7, 0.9)                # (regw, regv are not read by the rule)
    m.w0, m.w[:], m.v[:] = w0, w, v
    st = ftrl.FtrlState(m, alpha, beta, l1["w"], l1["v"], l2["w"], l2["v"], init_acc)

    def sgn(t):
        return (t > 0) - (t < 0)

    def step(theta, z, n, g, kind):
        n1 = n + g * g
        z1 = z + g - (math.sqrt(n1) - math.sqrt(n)) / alpha * theta
        D = (beta + math.sqrt(n1)) / alpha + l2[kind]
        return (0.0 if abs(z1) <= l1[kind] else -(z1 - sgn(z1) * l1[kind]) / D), z1, n1

    D0 = {kind: (beta + math.sqrt(init_acc)) / alpha + l2[kind] for kind in ("w", "v")}
    z_w = [-t * D0["w"] - sgn(t) * l1["w"] for t in w]
    z_v = [[-t * D0["v"] - sgn(t) * l1["v"] for t in v[f]] for f in range(2)]
    n_w, n_v = [init_acc] * 4, [[init_acc] * 4 for _ in range(2)]
    np.testing.assert_allclose(st.z_w, z_w, rtol=1e-13)
    np.testing.assert_allclose(st.z_v, z_v, rtol=1e-13)
    w1_seen = []
    for _ in range(2):
        ftrl.epoch(m, d, 0, lr, -1.0, 1.0, 2, 2, st)
        S, mult = [], []
        for r, row in enumerate(rows):
            s = [sum(v[f][j] * x for j, x in row) for f in range(2)]
            q = [sum((v[f][j] * x) ** 2 for j, x in row) for f in range(2)]
            rest = sum(w[j] * x for j, x in row) + sum(0.5 * (s[f] * s[f] - q[f]) for f in range(2))
            p = min(1.0, max(-1.0, w0 + rest))                   # both examples see the bias of the chunk start
            S.append(s)
            mult.append(-(y[r] - p))
        new_w0 = w0 - lr * (mult[0] + mult[1] + 2 * reg0 * w0)
        new_w, new_v = list(w), [list(v[0]), list(v[1])]
        for j in (0, 1, 2):
            occ = [(r, x) for r, row in enumerate(rows) for jj, x in row if jj == j]
            g = sum(mult[r] * x for r, x in occ)
            new_w[j], z_w[j], n_w[j] = step(w[j], z_w[j], n_w[j], g, "w")
            for f in range(2):
                g = sum(mult[r] * (S[r][f] * x - v[f][j] * x * x) for r, x in occ)
                new_v[f][j], z_v[f][j], n_v[f][j] = step(v[f][j], z_v[f][j], n_v[f][j], g, "v")
        w0, w, v = new_w0, new_w, new_v
        np.testing.assert_allclose(m.w0, w0, rtol=1e-13)
        np.testing.assert_allclose(m.w, w, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(m.v, v, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(st.z_w, z_w, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(st.z_v, z_v, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(st.n_w, n_w, rtol=1e-13)
        np.testing.assert_allclose(st.n_v, n_v, rtol=1e-13)
        w1_seen.append(float(m.w[1]))
    print("w_1 after the two epochs:", w1_seen, " z_w:", z_w)
    assert w1_seen[0] == 0.0 and not np.signbit(w1_seen[0]) and w1_seen[1] > 0.0      # (start -0.15: driven to +0, revived beyond)
    assert m.w[3] == 0.4 and m.v[0, 3] == 0.5 and m.v[1, 3] == -0.3
    assert st.n_w[3] == init_acc and st.n_v[0, 3] == init_acc and st.z_w[3] == z_w[3] and st.z_v[1, 3] == z_v[1][3]
    assert len({n_w[0], n_w[1], n_w[2]}) == 3 and min(n_w[:3]) > init_acc      # (the case exercises what it says)


def test_start_state_and_untouched_features():
    """z0 reproduces theta0 through the closed form (so with l1 = 0 every step is theta' = theta - g / D'); zeros start at z0 = 0; a
    feature no batch touches keeps theta, z and n exactly"""
    from libfm_amd import ftrl
    d, m = parity_case(8, rows=300)
    m.w[::7] = 0.0
    m.v[:, ::5] = 0.0
    for init_acc, beta in ((0.0, 1.0), (0.5, 1.0), (1.0, 0.0)):
        st = ftrl.FtrlState(m, 0.05, beta, 0.5, 0.3, 0.01, 0.02, init_acc)
        for theta, z, l1, l2 in ((m.w, st.z_w, 0.5, 0.01), (m.v, st.z_v, 0.3, 0.02)):
            D0 = (beta + math.sqrt(init_acc)) / 0.05 + l2
            back = np.where(np.abs(z) <= l1, 0.0, -(z - np.sign(z) * l1) / D0)
            np.testing.assert_allclose(back, theta, rtol=1e-12, atol=0)
            assert np.all(z[theta == 0.0] == 0.0) and np.all(np.abs(z[theta != 0.0]) > l1)
        assert np.all(st.n_w == init_acc) and np.all(st.n_v == init_acc)
    touched = np.zeros(m.n, dtype=bool)
    touched[d.entries["id"]] = True
    assert touched.any() and not touched.all()
    st = ftrl.FtrlState(m, **PARITY)
    z_w0, z_v0 = st.z_w.copy(), st.z_v.copy()
    c = m.copy()
    step = ftrl.epoch(c, d, 1, 0.01, -1.0, 1.0, 64, 16, st)
    assert step > 0.0
    assert np.array_equal(c.w[~touched], m.w[~touched]) and np.array_equal(c.v[:, ~touched], m.v[:, ~touched])
    assert np.array_equal(st.z_w[~touched], z_w0[~touched]) and np.array_equal(st.z_v[:, ~touched], z_v0[:, ~touched])
    assert np.all(st.n_w[~touched] == 0.0) and np.all(st.n_v[:, ~touched] == 0.0)
    assert (st.n_w[touched] > 0.0).all() and (c.w[touched] != m.w[touched]).mean() > 0.9
    for bad in (dict(alpha=0.0), dict(alpha=0.05, beta=0.0), dict(alpha=0.05, l1_w=-1.0), dict(alpha=0.05, l2_v=float("nan")),
                dict(alpha=float("inf"))):
        with pytest.raises(ValueError):
            ftrl.FtrlState(m, **bad)


def test_k1_off_leaves_the_linear_weights_alone():
    from libfm_amd import ftrl
    d, m = parity_case(4, k1=False, rows=128)
    m.w[:] = 0.25
    st = ftrl.FtrlState(m, **PARITY)
    z0 = st.z_w.copy()
    ftrl.epoch(m, d, 0, 0.01, -1.0, 1.0, 64, 16, st)
    assert np.all(m.w == 0.25) and np.array_equal(st.z_w, z0) and np.all(st.n_w == 0.0)


def test_hot_feature_case_stays_bounded():
    """one id in every row at batch 512, where the plain batch rule diverges (tests/test_adagrad_cpu.py): FTRL's per-coordinate D keeps it
    bounded.  Recorded with these options: max |v| = 0.27 after 6 epochs."""
    from libfm_amd import ftrl
    d, m = hot_case()
    st = ftrl.FtrlState(m, 0.05, 1.0)
    rmse = []
    for _ in range(6):
        ftrl.epoch(m, d, 0, 0.05, -1.0, 1.0, 512, 8, st)
        rmse.append(O.evaluate(m, d, 0, -1.0, 1.0)[0])
    print("ftrl:", rmse, "max |v|", np.abs(m.v).max(), "max n", st.n_v.max())
    assert np.isfinite(m.v).all() and np.abs(m.v).max() < 1.0
    assert rmse[-1] < rmse[0]


@pytest.mark.parametrize("task", [0, 1])
def test_float32_restatement_stays_close(task):
    """dtype=float32 runs the sums and the step in fp32: what rounding can cost at the parity shape.  Parameters an order of magnitude
    inside the tolerances tests/test_gpu_ftrl.py holds the device to; z and n to rtol 1e-5 plus the absolute terms recorded when the
    rule was specified (z 4e-6, n 9e-6 -- n starts at 0, so its relative gap alone is unbounded), and the zero pattern away from the
    threshold."""
    from libfm_amd import ftrl
    d, m = parity_case(8)
    res = {}
    for dt in (np.float64, np.float32):
        c = m.copy()
        st = ftrl.FtrlState(c, **PARITY)
        for _ in range(3):
            ftrl.epoch(c, d, task, 0.01, -1.0, 1.0, 64, 16, st, dtype=dt)
        res[dt] = (c, st)
    (a, sa), (b, sb) = res[np.float64], res[np.float32]
    print("gaps: v %.3g w %.3g z_v %.3g z_w %.3g n_v %.3g n_w %.3g; zero share v %.3f w %.3f" % (
        np.abs(a.v - b.v).max(), np.abs(a.w - b.w).max(), np.abs(sa.z_v - sb.z_v).max(), np.abs(sa.z_w - sb.z_w).max(),
        np.abs(sa.n_v - sb.n_v).max(), np.abs(sa.n_w - sb.n_w).max(), (a.v == 0).mean(), (a.w == 0).mean()))
    np.testing.assert_allclose(b.v, a.v, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(b.w, a.w, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(sb.z_v, sa.z_v, rtol=1e-5, atol=4e-6)
    np.testing.assert_allclose(sb.z_w, sa.z_w, rtol=1e-5, atol=4e-6)
    np.testing.assert_allclose(sb.n_v, sa.n_v, rtol=1e-5, atol=9e-6)
    np.testing.assert_allclose(sb.n_w, sa.n_w, rtol=1e-5, atol=9e-6)
    assert 0.01 < (a.v == 0).mean() < 0.5 and 0.05 < (a.w == 0).mean() < 0.5      # (L1 produced zeros, and not only zeros)
    for x64, x32, z64, l1 in ((a.v, b.v, sa.z_v, 0.3), (a.w, b.w, sa.z_w, 0.5)):
        near = np.abs(np.abs(z64) - l1) <= 1e-4 * (1.0 + l1)
        assert near.mean() <= 1e-3
        assert np.array_equal((x64 == 0)[~near], (x32 == 0)[~near])


@pytest.mark.parametrize("argv, text", [
    (["-optimizer", "ftrl", "-method", "als"], "ERROR: -optimizer / -init_acc belong to -method sgd, not -method als"),
    (["-optimizer", "ftrl", "-method", "sgda"], "ERROR: -optimizer / -init_acc belong to -method sgd, not -method sgda"),
    (["-l1", "0.1,0.1", "-method", "mcmc"], "ERROR: -optimizer / -init_acc belong to -method sgd, not -method mcmc"),
    (["-optimizer", "foo", "-method", "sgd"], "ERROR: -optimizer knows sgd and adagrad, not 'foo'"),
    (["-optimizer", "foo", "-method", "sgd"], "ftrl"),
    (["-optimizer", "ftrl", "-method", "sgd", "-gpu_mode", "sequential"], "ERROR: -optimizer ftrl runs on the minibatch rule"),
    (["-optimizer", "ftrl", "-method", "sgd", "-gpu_mode", "hogwild"], "ERROR: -optimizer ftrl runs on the minibatch rule"),
    (["-optimizer", "ftrl", "-method", "sgd", "-init_acc", "0.5"], "ERROR: -init_acc belongs to -optimizer adagrad"),
    (["-optimizer", "adagrad", "-method", "sgd", "-l1", "0.1,0.1"], "ERROR: -l1 belongs to -optimizer ftrl"),
    (["-method", "sgd", "-ftrl_alpha", "0.1"], "ERROR: -ftrl_alpha belongs to -optimizer ftrl"),
    (["-optimizer", "sgd", "-method", "sgd", "-ftrl_beta", "1"], "ERROR: -ftrl_beta belongs to -optimizer ftrl"),
    (["-optimizer", "ftrl", "-method", "sgd", "-ftrl_alpha", "0"], "ERROR: -ftrl_alpha needs a finite value > 0"),
    (["-optimizer", "ftrl", "-method", "sgd", "-ftrl_beta", "inf"], "ERROR: -ftrl_beta needs a finite value > 0"),
    (["-optimizer", "ftrl", "-method", "sgd", "-l1", "0.1"], "ERROR: -l1 needs 2 finite values >= 0"),
    (["-optimizer", "ftrl", "-method", "sgd", "-l1", "0.1,-1"], "ERROR: -l1 needs 2 finite values >= 0"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    # (the files do not exist: a refusal that came later than the argument checks would be a different error)
    assert cli.main(["-task", "r", "-train", "no_such_train", "-test", "no_such_test", "-learn_rate", "0.01"] + argv) == 0
    assert text in capsys.readouterr().err


def test_learners():
    from libfm_amd import learner as L
    assert L.FMLearnSGD.OPTIMIZERS == ("sgd", "adagrad", "ftrl")
    for cls in (L.FMLearnSGDA, L.FMLearnPairSGD):
        l = cls()
        l.optimizer = "ftrl"
        l.learn_rate = 0.01
        with pytest.raises(ValueError, match="unknown optimizer"):
            l.init()
    l = L.FMLearnSGD()
    assert (l.ftrl_alpha, l.ftrl_beta, l.l1_w, l.l1_v, l.l2_w, l.l2_v) == (0.0, 1.0, 0.0, 0.0, None, None)
    for mode in ("sequential", "hogwild"):
        l.optimizer, l.learn_rate, l.mode = "ftrl", 0.01, mode
        with pytest.raises(ValueError, match="optimizer ftrl runs on the minibatch rule"):
            l.init()
    assert callable(l.sparsity)


def test_binding_structs_match_the_header():
    """fmx_ftrl_opts is two uint32 and seven doubles, fmx_sparsity six uint64: the sizes the header's declarations give"""
    import ctypes as C
    from libfm_amd import capi
    assert C.sizeof(capi.FtrlOpts) == 8 + 7 * 8 and capi.FtrlOpts.alpha.offset == 8 and capi.FtrlOpts.init_acc.offset == 56
    assert C.sizeof(capi.Sparsity) == 48 and [f for f, _ in capi.Sparsity._fields_] == [
        "features", "w_zero", "v_coords", "v_zero", "v_zero_rows", "dead_features"]
    names = [n for n, _, _ in capi.SYMBOLS]
    for fn in ("fmx_ftrl_begin", "fmx_ftrl_epoch", "fmx_ftrl_get_state_rows", "fmx_ftrl_end", "fmx_param_sparsity"):
        assert names.count(fn) == 1
