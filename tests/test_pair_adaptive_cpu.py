"""CPU: the numpy restatements of the pairwise batch rule stepped per coordinate (libfm_amd/adaptive.py pair_epoch, libfm_amd/ftrl.py
pair_epoch) -- pinned to tests/bpr_oracle.py's batch rule, to literals worked out from the formulas, to the FTRL / AdaGrad identity and
to the popularity-skewed case that motivates them -- and the refusals of the learner and the command line, reached before any device.
The device path is held to these restatements in tests/test_gpu_pair_adaptive.py."""
import math

import numpy as np
import pytest

import bpr_oracle as B
import pair_adaptive_cases as PC
from oracle import oracle as O
from test_gpu_bpr import rows_and_pairs


@pytest.mark.parametrize("batch", [1, 7, 64, 600])
def test_sgd_rule_is_the_oracles_batch_rule(batch):
    from libfm_amd import adaptive
    n, k, lr = 50, 8, 0.05
    ent, rp, pa, pb = rows_and_pairs(n, 150, 500, 9, 31)
    m0 = PC.start_model(n, k)
    a, b = m0.copy(), m0.copy()
    st = adaptive.AdaptState(n, k, 1.0)
    B.pair_epoch_batch(a, ent, rp, pa, pb, lr, batch)
    step = adaptive.pair_epoch(b, ent, rp, pa, pb, lr, batch, st, rule="sgd")
    print("gaps: v %.3g  w %.3g  w0 %.3g" % (PC.gap(a.v, b.v), PC.gap(a.w, b.w), abs(a.w0 - b.w0)))
    np.testing.assert_allclose(b.v, a.v, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b.w, a.w, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b.w0, a.w0, rtol=1e-12)
    assert np.all(st.n_w == 1.0) and np.all(st.n_v == 1.0)      # the plain rule leaves the accumulators alone
    assert step > 1e-4 and a.w0 != m0.w0


def hand_case():
    """rows 0: {0: 1, 1: 2}, 1: {0: 0.5, 2: 1, 2: -1.5} (id 2 repeated), 2: {1: -1}; pairs (0, 1) and (2, 0) in ONE batch; feature 3 is
    never touched; k = 2.  Returns (rows, entries, row_ptr, pa, pb, w, v)"""
    rows = [[(0, 1.0), (1, 2.0)], [(0, 0.5), (2, 1.0), (2, -1.5)], [(1, -1.0)]]
    d = O.Data.from_rows(rows, np.zeros(3, dtype=np.float32))
    w = [0.1, -0.2, 0.3, 0.4]
    v = [[0.1, -0.1, 0.2, 0.5], [0.05, 0.15, -0.05, -0.3]]     # [f][j]
    return rows, d.entries, d.row_ptr, np.array([0, 2], np.uint32), np.array([1, 0], np.uint32), w, v


def hand_sums(rows, pairs, w, v, regw, regv):
    """per feature the sum over the pairs that contain it of mult_t grad_tj (+ reg theta), written out from the formulas:
    ({j: g_w}, {(f, j): g_v}); reg 0 leaves the terms out"""
    gw, gv = {}, {}
    for a, b in pairs:
        y, S = [], []
        for r in (a, b):
            s = [sum(v[f][j] * x for j, x in rows[r]) for f in range(2)]
            q = [sum((v[f][j] * x) ** 2 for j, x in rows[r]) for f in range(2)]
            y.append(sum(w[j] * x for j, x in rows[r]) + sum(0.5 * (s[f] * s[f] - q[f]) for f in range(2)))
            S.append(s)
        mult = -(1.0 - 1.0 / (1.0 + math.exp(-(y[0] - y[1]))))
        for j in sorted({j for r in (a, b) for j, _ in rows[r]}):
            xa = [x for jj, x in rows[a] if jj == j]
            xb = [x for jj, x in rows[b] if jj == j]
            gw[j] = gw.get(j, 0.0) + mult * (sum(xa) - sum(xb)) + regw * w[j]
            for f in range(2):
                g = sum(S[0][f] * x - v[f][j] * x * x for x in xa) - sum(S[1][f] * x - v[f][j] * x * x for x in xb)
                gv[(f, j)] = gv.get((f, j), 0.0) + mult * g + regv * v[f][j]
    return gw, gv


def test_hand_sized_case_adagrad():
    from libfm_amd import adaptive
    rows, ent, rp, pa, pb, w, v = hand_case()
    eta, reg0, regw, regv, init_acc = 0.3, 0.01, 0.02, 0.03, 0.5
    m = O.Model(4, 2, True, True, reg0, regw, regv)
    m.w0, m.w[:], m.v[:] = 0.05, w, v
    st = adaptive.AdaptState(4, 2, init_acc)
    n_w, n_v, w0 = [init_acc] * 4, [[init_acc] * 4 for _ in range(2)], 0.05
    for _ in range(2):                                          # (the accumulators carry over)
        adaptive.pair_epoch(m, ent, rp, pa, pb, eta, 2, st)
        gw, gv = hand_sums(rows, [(0, 1), (2, 0)], w, v, regw, regv)
        new_w, new_v = list(w), [list(v[0]), list(v[1])]
        for j in (0, 1, 2):
            n_w[j] += gw[j] ** 2
            new_w[j] = w[j] - eta * gw[j] / math.sqrt(n_w[j])
            for f in range(2):
                n_v[f][j] += gv[(f, j)] ** 2
                new_v[f][j] = v[f][j] - eta * gv[(f, j)] / math.sqrt(n_v[f][j])
        w, v = new_w, new_v
        w0 = (w0 - reg0 * w0)
        w0 = (w0 - reg0 * w0)                                    # once per pair, no learning rate
        np.testing.assert_allclose(m.w, w, rtol=1e-12)
        np.testing.assert_allclose(m.v, v, rtol=1e-12)
        np.testing.assert_allclose(st.n_w, n_w, rtol=1e-12)
        np.testing.assert_allclose(st.n_v, n_v, rtol=1e-12)
        assert m.w0 == w0
    assert m.w[3] == 0.4 and m.v[0, 3] == 0.5 and st.n_w[3] == init_acc and st.n_v[1, 3] == init_acc
    assert len({n_w[0], n_w[1], n_w[2]}) == 3 and min(n_w[:3]) > init_acc


def test_hand_sized_case_ftrl():
    from libfm_amd import ftrl
    rows, ent, rp, pa, pb, w, v = hand_case()
    alpha, beta, init_acc = 0.3, 1.0, 0.25
    l1, l2 = {"w": 0.05, "v": 0.004}, {"w": 0.02, "v": 0.03}
    m = O.Model(4, 2, False, True, 0.0, 0.7, 0.9)                # (regw, regv are not read by the rule)
    m.w[:], m.v[:] = w, v
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
    for _ in range(2):
        ftrl.pair_epoch(m, ent, rp, pa, pb, 2, st)
        gw, gv = hand_sums(rows, [(0, 1), (2, 0)], w, v, 0.0, 0.0)
        new_w, new_v = list(w), [list(v[0]), list(v[1])]
        for j in (0, 1, 2):
            new_w[j], z_w[j], n_w[j] = step(w[j], z_w[j], n_w[j], gw[j], "w")
            for f in range(2):
                new_v[f][j], z_v[f][j], n_v[f][j] = step(v[f][j], z_v[f][j], n_v[f][j], gv[(f, j)], "v")
        w, v = new_w, new_v
        np.testing.assert_allclose(m.w, w, rtol=1e-11, atol=1e-15)
        np.testing.assert_allclose(m.v, v, rtol=1e-11, atol=1e-15)
        np.testing.assert_allclose(st.z_w, z_w, rtol=1e-11, atol=1e-15)
        np.testing.assert_allclose(st.z_v, z_v, rtol=1e-11, atol=1e-15)
        np.testing.assert_allclose(st.n_w, n_w, rtol=1e-12)
        np.testing.assert_allclose(st.n_v, n_v, rtol=1e-12)
    assert m.w[3] == 0.4 and m.v[1, 3] == -0.3 and st.n_w[3] == init_acc and st.z_v[0, 3] == z_v[0][3]
    assert min(n_w[:3]) > init_acc


@pytest.mark.parametrize("batch", [7, 600])
def test_ftrl_is_adagrad_under_the_identity(batch):
    """l1 = l2 = beta = 0, init_acc = a, alpha = eta and reg 0: the proximal step IS theta - eta g / sqrt(n')"""
    from libfm_amd import adaptive, ftrl
    n, k, eta, a0 = 50, 8, 0.05, 0.5
    ent, rp, pa, pb = rows_and_pairs(n, 150, 500, 9, 31)
    m0 = PC.start_model(n, k, reg=(0.01, 0.0, 0.0))
    a, b = m0.copy(), m0.copy()
    sa, sb = adaptive.AdaptState(n, k, a0), ftrl.FtrlState(b, eta, 0.0, init_acc=a0)
    for _ in range(3):
        adaptive.pair_epoch(a, ent, rp, pa, pb, eta, batch, sa)
        ftrl.pair_epoch(b, ent, rp, pa, pb, batch, sb)
    print("gaps: v %.3g  w %.3g  n_v %.3g" % (PC.gap(a.v, b.v), PC.gap(a.w, b.w), PC.gap(sa.n_v, sb.n_v)))
    np.testing.assert_allclose(b.v, a.v, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(b.w, a.w, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(sb.n_v, sa.n_v, rtol=1e-9)
    np.testing.assert_allclose(sb.n_w, sa.n_w, rtol=1e-9)
    assert b.w0 == a.w0 and PC.gap(a.v, m0.v) > 1e-3


def test_the_plain_rule_diverges_where_adagrad_converges():
    """popularity-skewed items at B = 2 048 and rate 0.5: a popular item's segment sums hundreds of pair gradients"""
    from libfm_amd import adaptive
    ent, rp, pa, pb, m0 = PC.skewed_case()
    start = PC.pair_loss(m0, ent, rp, pa, pb)
    plain = m0.copy()
    with np.errstate(all="ignore"):
        adaptive.pair_epoch(plain, ent, rp, pa, pb, PC.SKEW_ETA, PC.SKEW_B, adaptive.AdaptState(m0.n, m0.k, 1.0), rule="sgd")
    plain_loss = PC.pair_loss(plain, ent, rp, pa, pb)
    m, st, losses, steps = m0.copy(), adaptive.AdaptState(m0.n, m0.k, 1.0), [start], []
    for _ in range(6):
        steps.append(adaptive.pair_epoch(m, ent, rp, pa, pb, PC.SKEW_ETA, PC.SKEW_B, st))
        losses.append(PC.pair_loss(m, ent, rp, pa, pb))
    print("start %.4f  plain after one epoch %.4g  adagrad %s  largest steps %s" % (start, plain_loss, np.round(losses[1:], 4), np.round(steps, 4)))
    assert plain_loss > start
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert max(steps) <= PC.SKEW_ETA


@pytest.mark.parametrize("rule", ["adagrad", "ftrl"])
def test_float32_step_stays_close(rule):
    """step_dtype float32 (the device's arithmetic: g32, fp32 theta and state) against float64 after three epochs: test_adagrad_cpu's
    bound on theta"""
    n, k = 50, 8
    ent, rp, pa, pb = rows_and_pairs(n, 150, 500, 9, 31)
    m0 = PC.start_model(n, k)
    g_theta, g_state, (a, _), (b, _) = PC.step_gaps(rule, m0, [(ent, rp, pa, pb)] * 3, 64)
    print("gaps %s: theta %.3g  state %s" % (rule, g_theta, ["%.3g" % g for g in g_state]))
    np.testing.assert_allclose(b.v, a.v, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(b.w, a.w, rtol=1e-5, atol=2e-6)
    assert b.v.dtype == np.float64 and PC.gap(a.v, m0.v) > 1e-3


def test_ftrl_options_of_the_parity_tests_leave_zeros():
    """the device tests' FTRL options at B = 64: a share of both tables is exactly zero and no coordinate sits in the exclusion band"""
    n, k = 50, 8
    ent, rp, pa, pb = rows_and_pairs(n, 150, 500, 9, 31)
    m, st = PC.restate("ftrl", PC.start_model(n, k), [(ent, rp, pa, pb)] * 3, 64)
    print("zero share: v %.3f  w %.3f" % ((m.v == 0).mean(), (m.w == 0).mean()))
    assert 0.02 < (m.v == 0).mean() < 0.5 and 0.02 < (m.w == 0).mean() < 0.5
    for z, l1 in ((st.z_v, PC.FTRL["l1_v"]), (st.z_w, PC.FTRL["l1_w"])):
        assert (np.abs(np.abs(z) - l1) <= 1e-4 * (1.0 + l1)).mean() <= 1e-3


def test_untouched_features_and_bad_arguments():
    from libfm_amd import adaptive, ftrl
    n, k = 50, 4
    ent, rp, pa, pb = rows_and_pairs(n, 150, 40, 3, 33)
    touched = np.zeros(n, dtype=bool)
    for t in range(len(pa)):
        for r in (pa[t], pb[t]):
            touched[ent["id"][int(rp[r]):int(rp[r + 1])]] = True
    assert touched.any() and not touched.all()
    m0 = PC.start_model(n, k)
    for rule in ("adagrad", "ftrl"):
        m = m0.copy()
        st = PC.make_state(rule, m)
        before = [x.copy() for x in PC.state_arrays(rule, st)]
        PC.rule_epoch(rule, m, st, ent, rp, pa, pb, 16)
        assert np.array_equal(m.w[~touched], m0.w[~touched]) and np.array_equal(m.v[:, ~touched], m0.v[:, ~touched])
        for x, y in zip(PC.state_arrays(rule, st), before):
            assert np.array_equal(x[..., ~touched], y[..., ~touched])
        assert (m.w[touched] != m0.w[touched]).mean() > 0.8
    with pytest.raises(ValueError):
        adaptive.pair_epoch(m0.copy(), ent, rp, pa, pb, 0.05, 16, adaptive.AdaptState(n, k, 1.0), rule="adam")
    with pytest.raises(ValueError):
        adaptive.pair_epoch(m0.copy(), ent, rp, pa, pb, 0.05, 0, adaptive.AdaptState(n, k, 1.0))
    with pytest.raises(ValueError):
        ftrl.pair_epoch(m0.copy(), ent, rp, pa, pb, 0, ftrl.FtrlState(m0, 0.05))


def test_learner_refusals_before_any_device():
    from libfm_amd import learner as L
    assert L.FMLearnPairAdaptive.OPTIMIZERS == L.FMLearnSGD.OPTIMIZERS == ("sgd", "adagrad", "ftrl")
    assert issubclass(L.FMLearnPairAdaptive, L.FMLearnPairSGD) and L.FMLearnPairSGD.OPTIMIZERS == ("sgd",)
    l = L.FMLearnPairAdaptive()
    assert l.mode == "minibatch" and l.optimizer == "sgd"
    l.learn_rate = 0.01
    for opt in ("adagrad", "ftrl"):
        l.optimizer, l.mode = opt, "sequential"
        with pytest.raises(ValueError, match="optimizer %s runs on the minibatch rule" % opt):
            l.init()
    l.optimizer, l.mode = "rmsprop", "minibatch"
    with pytest.raises(ValueError, match="unknown optimizer"):
        l.init()
    assert l._h is None


@pytest.mark.parametrize("argv, text", [
    (["-optimizer", "adagrad", "-gpu_mode", "sequential"], "ERROR: -optimizer adagrad runs on the minibatch rule"),
    (["-optimizer", "ftrl", "-gpu_mode", "sequential"], "ERROR: -optimizer ftrl runs on the minibatch rule"),
    (["-optimizer", "foo"], "ERROR: -optimizer knows sgd and adagrad, not 'foo'"),
    (["-optimizer", "sgd", "-init_acc", "0.5"], "ERROR: -init_acc belongs to -optimizer adagrad"),
    (["-optimizer", "adagrad", "-l1", "0.1,0.1"], "ERROR: -l1 belongs to -optimizer ftrl"),
    (["-optimizer", "ftrl", "-l1", "0.1"], "ERROR: -l1 needs 2 finite values >= 0"),
    (["-optimizer", "adagrad", "-init_acc", "0"], "ERROR: -init_acc needs a finite value > 0"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    # (the files do not exist: a refusal that came later than the argument checks would be a different error)
    base = ["-method", "bpr", "-train", "no_such_train", "-test", "no_such_test", "-train_pairs", "no_such_a", "-test_pairs", "no_such_b",
            "-learn_rate", "0.01"]
    assert cli.main(base + argv) == 0
    assert text in capsys.readouterr().err


def test_cli_accepts_the_optimizers_for_bpr(capsys):
    """-method bpr -optimizer adagrad passes the argument checks (the refusal is the missing file)"""
    from libfm_amd import cli
    assert cli.main(["-method", "bpr", "-train", "no_such_train", "-test", "no_such_test", "-train_pairs", "a", "-test_pairs", "b",
                     "-learn_rate", "0.01", "-optimizer", "adagrad", "-init_acc", "0.5"]) == 0
    err = capsys.readouterr().err
    assert "belong to -method sgd" not in err and "no_such_train" in err


def test_capi_lists_each_new_symbol_once():
    from libfm_amd import capi
    names = [s[0] for s in capi.SYMBOLS]
    for name in ("fmx_adapt_pair_epoch", "fmx_adapt_pair_epoch_sampled", "fmx_ftrl_pair_epoch", "fmx_ftrl_pair_epoch_sampled"):
        assert names.count(name) == 1
    for meth in ("adapt_pair_epoch", "adapt_pair_epoch_sampled", "ftrl_pair_epoch", "ftrl_pair_epoch_sampled"):
        assert callable(getattr(capi.Handle, meth))
