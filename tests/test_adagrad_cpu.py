"""CPU: the numpy restatement of AdaGrad on the minibatch rule (libfm_amd/adaptive.py) -- pinned to the oracle's batch rule, to
literals worked out from the formulas, to its identities and to the hot-feature case that motivates it -- and the command line's
refusals of -optimizer.  The device path is held to this restatement in tests/test_gpu_adagrad.py."""
import math

import numpy as np
import pytest

from oracle import oracle as O


def hot_case():
    """600 rows of 12 ids over 2000 features: id 0 in every row, ids 1..3 cycling, every fifth row with a repeated id"""
    n, k, nnz, rows = 2000, 8, 12, 600
    d0 = O.synth_rows(9, 0, rows, nnz, n)
    ent = d0.entries.copy().reshape(rows, nnz)
    ent["id"][:, 0] = 0
    ent["id"][:, 1] = 1 + (np.arange(rows) % 3)
    ent["id"][::5, 2] = ent["id"][::5, 3]
    d = O.Data(ent.reshape(-1), d0.row_ptr, d0.target.copy())
    m = O.Model(n, k, True, True, 0.0, 0.002, 0.001)
    m.v[:] = O.init_values(1, n, k, 0.05)
    return d, m


@pytest.mark.parametrize("task", [0, 1])
def test_sgd_rule_is_the_oracles_batch_rule(task):
    from libfm_amd import adaptive
    n, k = 6400, 8
    d = O.synth_rows(7, 0, 300, 32, n)
    m = O.Model(n, k, True, True, 0.01, 0.002, 0.001)
    m.v[:] = O.init_values(1, n, k, 0.05)
    a, b = m.copy(), m.copy()
    st = adaptive.AdaptState(n, k, 1.0)
    for _ in range(2):
        O.sgd_epoch_minibatch(a, d, task, 0.01, -1.0, 1.0, 64, 16, bias_lag=False)     # 300 rows: a tail batch of 44
        adaptive.epoch(b, d, task, 0.01, -1.0, 1.0, 64, 16, st, rule="sgd")
    np.testing.assert_allclose(b.v, a.v, rtol=1e-10)
    np.testing.assert_allclose(b.w, a.w, rtol=1e-10)
    np.testing.assert_allclose(b.w0, a.w0, rtol=1e-10)
    assert np.all(st.n_w == 1.0) and np.all(st.n_v == 1.0)      # the plain rule leaves the accumulators alone
    assert np.abs(a.v - m.v).max() > 1e-5                       # (the epochs moved something)


def test_hand_sized_case():
    """two rows that share feature 0, row 1 repeats id 2, feature 3 is never touched; k = 2, regression, one batch per epoch, the bias
    in one micro-chunk; init_acc 0.5, two epochs (the accumulators carry over).  Every number below is the formula written out."""
    from libfm_amd import adaptive
    rows = [[(0, 1.0), (1, 2.0)], [(0, 0.5), (2, 1.0), (2, -1.5)]]
    y = [0.7, -0.4]
    lr, eta, reg0, regw, regv, init_acc = 0.1, 0.3, 0.01, 0.02, 0.03, 0.5
    w0, w = 0.05, [0.1, -0.2, 0.3, 0.4]
    v = [[0.1, -0.1, 0.2, 0.5], [0.05, 0.15, -0.05, -0.3]]     # [f][j]
    d = O.Data.from_rows(rows, np.array(y, dtype=np.float32))
    y = [float(t) for t in d.target]                             # (the targets as the data holds them: fp32)
    m = O.Model(4, 2, True, True, reg0, regw, regv)
    m.w0, m.w[:], m.v[:] = w0, w, v
    st = adaptive.AdaptState(4, 2, init_acc)
    n_w, n_v = [init_acc] * 4, [[init_acc] * 4 for _ in range(2)]
    for _ in range(2):
        adaptive.epoch(m, d, 0, lr, -1.0, 1.0, 2, 2, st, eta=eta)
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
            g = sum(mult[r] * x for r, x in occ) + len(occ) * regw * w[j]
            n_w[j] += g * g
            new_w[j] = w[j] - eta * g / math.sqrt(n_w[j])
            for f in range(2):
                g = sum(mult[r] * (S[r][f] * x - v[f][j] * x * x) for r, x in occ) + len(occ) * regv * v[f][j]
                n_v[f][j] += g * g
                new_v[f][j] = v[f][j] - eta * g / math.sqrt(n_v[f][j])
        w0, w, v = new_w0, new_w, new_v
        np.testing.assert_allclose(m.w0, w0, rtol=1e-13)
        np.testing.assert_allclose(m.w, w, rtol=1e-13)
        np.testing.assert_allclose(m.v, v, rtol=1e-13)
        np.testing.assert_allclose(st.n_w, n_w, rtol=1e-13)
        np.testing.assert_allclose(st.n_v, n_v, rtol=1e-13)
    assert m.w[3] == 0.4 and m.v[0, 3] == 0.5 and m.v[1, 3] == -0.3
    assert st.n_w[3] == init_acc and st.n_v[0, 3] == init_acc and st.n_v[1, 3] == init_acc
    assert len({n_w[0], n_w[1], n_w[2]}) == 3 and min(n_w[:3]) > init_acc      # (the case exercises what it says)


def test_identities():
    from libfm_amd import adaptive
    n, k, eta = 6400, 8, 0.05
    d = O.synth_rows(7, 0, 300, 32, n)
    m0 = O.Model(n, k, True, True, 0.01, 0.002, 0.001)
    m0.v[:] = O.init_values(1, n, k, 0.05)
    m0.w[:] = O.init_values(2, n, 1, 0.05)[0]
    touched = np.zeros(n, dtype=bool)
    touched[d.entries["id"]] = True
    assert touched.any() and not touched.all()
    # untouched features keep parameters and init_acc exactly; every coordinate moves by less than eta per batch
    a, sa = m0.copy(), adaptive.AdaptState(n, k, 0.25)
    step = adaptive.epoch(a, d, 1, 0.01, -1.0, 1.0, 64, 16, sa, eta=eta)
    assert 0.0 < step < eta
    assert np.array_equal(a.w[~touched], m0.w[~touched]) and np.array_equal(a.v[:, ~touched], m0.v[:, ~touched])
    assert np.all(sa.n_w[~touched] == 0.25) and np.all(sa.n_v[:, ~touched] == 0.25)
    assert np.all(sa.n_w[touched] > 0.25) and np.all(a.w[touched] != m0.w[touched])
    # a second epoch continues from the state: it differs from an epoch that restarts the accumulators
    cont, restart = a.copy(), a.copy()
    adaptive.epoch(cont, d, 1, 0.01, -1.0, 1.0, 64, 16, sa, eta=eta)
    adaptive.epoch(restart, d, 1, 0.01, -1.0, 1.0, 64, 16, adaptive.AdaptState(n, k, 0.25), eta=eta)
    assert np.abs(cont.v - a.v)[:, touched].max() < np.abs(restart.v - a.v)[:, touched].max()
    assert np.all(sa.n_v[:, touched] >= 0.25)
    two, st2 = m0.copy(), adaptive.AdaptState(n, k, 0.25)
    for _ in range(2):
        adaptive.epoch(two, d, 1, 0.01, -1.0, 1.0, 64, 16, st2, eta=eta)
    assert np.array_equal(two.v, cont.v) and np.array_equal(st2.n_v, sa.n_v) and two.w0 == cont.w0
    with pytest.raises(ValueError):
        adaptive.epoch(two, d, 1, 0.01, -1.0, 1.0, 64, 16, st2, rule="adam")
    with pytest.raises(ValueError):
        adaptive.AdaptState(n, k, 0.0)


def test_hot_feature_case():
    """one id in every row at batch 512: the plain batch rule diverges, AdaGrad at the same batch and rate converges"""
    from libfm_amd import adaptive
    d, m = hot_case()
    rmse = {}
    final = {}
    for rule in ("sgd", "adagrad"):
        c, st = m.copy(), adaptive.AdaptState(m.n, m.k, 1.0)
        rmse[rule] = []
        for _ in range(6):
            with np.errstate(all="ignore"):
                step = adaptive.epoch(c, d, 0, 0.05, -1.0, 1.0, 512, 8, st, eta=0.05, rule=rule)
            if rule == "adagrad":
                assert step < 0.05
            rmse[rule].append(O.evaluate(c, d, 0, -1.0, 1.0)[0])
        final[rule] = c
    print("plain batch rule:", rmse["sgd"], "max |v|", np.abs(final["sgd"].v).max())
    print("adagrad         :", rmse["adagrad"], "max |v|", np.abs(final["adagrad"].v).max())
    assert all(b < a for a, b in zip(rmse["adagrad"], rmse["adagrad"][1:]))
    assert np.abs(final["adagrad"].v).max() < 1.0
    assert rmse["sgd"][5] > rmse["sgd"][0]


def test_float32_restatement_stays_close():
    """dtype=float32 runs the sums in fp32: what the device's rounding can cost at the parity shape, an order of magnitude inside the
    tolerances tests/test_gpu_adagrad.py holds the device to"""
    from libfm_amd import adaptive
    n, k = 6400, 8
    d = O.synth_rows(7, 0, 512, 32, n)
    m = O.Model(n, k, True, True, 0.0, 0.0, 0.001)
    m.v[:] = O.init_values(1, n, k, 0.05)
    res = {}
    for dt in (np.float64, np.float32):
        c, st = m.copy(), adaptive.AdaptState(n, k, 1.0)
        for _ in range(3):
            adaptive.epoch(c, d, 1, 0.01, -1.0, 1.0, 64, 16, st, eta=0.05, dtype=dt)
        res[dt] = (c, st)
    (a, sa), (b, sb) = res[np.float64], res[np.float32]
    np.testing.assert_allclose(b.v, a.v, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(b.w, a.w, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(sb.n_v, sa.n_v, rtol=1e-5)
    np.testing.assert_allclose(sb.n_w, sa.n_w, rtol=1e-5)


@pytest.mark.parametrize("argv, text", [
    (["-optimizer", "adagrad", "-method", "als"], "ERROR: -optimizer / -init_acc belong to -method sgd, not -method als"),
    (["-optimizer", "adagrad", "-method", "mcmc"], "ERROR: -optimizer / -init_acc belong to -method sgd, not -method mcmc"),
    (["-optimizer", "adagrad", "-method", "sgda"], "ERROR: -optimizer / -init_acc belong to -method sgd, not -method sgda"),
    (["-optimizer", "foo", "-method", "sgd"], "ERROR: -optimizer knows sgd and adagrad, not 'foo'"),
    (["-optimizer", "adagrad", "-method", "sgd", "-gpu_mode", "sequential"], "ERROR: -optimizer adagrad runs on the minibatch rule"),
    (["-optimizer", "sgd", "-method", "sgd", "-init_acc", "0.5"], "ERROR: -init_acc belongs to -optimizer adagrad"),
    (["-optimizer", "adagrad", "-method", "sgd", "-init_acc", "0"], "ERROR: -init_acc needs a finite value > 0"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    # (the files do not exist: a refusal that came later than the argument checks would be a different error)
    assert cli.main(["-task", "r", "-train", "no_such_train", "-test", "no_such_test", "-learn_rate", "0.01"] + argv) == 0
    assert text in capsys.readouterr().err


def test_learners_refuse_other_optimizers():
    from libfm_amd import learner as L
    for cls in (L.FMLearnSGDA, L.FMLearnPairSGD):
        l = cls()
        l.optimizer = "adagrad"
        l.learn_rate = 0.01
        with pytest.raises(ValueError, match="unknown optimizer"):
            l.init()
    l = L.FMLearnSGD()
    assert l.optimizer == "sgd" and l.init_acc == 0.0 and l.adapt_learn_rate == 0.0
    l.optimizer, l.learn_rate, l.mode = "adagrad", 0.01, "sequential"
    with pytest.raises(ValueError, match="minibatch"):
        l.init()
    l.optimizer, l.mode = "rmsprop", "minibatch"
    with pytest.raises(ValueError, match="unknown optimizer"):
        l.init()
