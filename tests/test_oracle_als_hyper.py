"""CPU: the ALS restatement at the hyper-priors the MCMC learner's sweep runs at -- alpha != 1 and prior means mu != 0 -- against
the REAL reference (fm_learn_mcmc with do_sample = do_multilevel = 0, alpha_0 and mu_0 set after init(): fixtures hyp_*, made by
tests/golden/make_golden.py).  The fixtures have features without a training column in the middle of the id range and above the
train's maximum, so the prior draws of those features are pinned too.  Main-table cases bit for bit, block-structured ones on the
flat rows to accumulated fp64 rounding (as tests/test_oracle_relations.py)."""
import numpy as np
import pytest

from common import Golden
from conftest import golden_cases
from test_oracle_relations import flat

CASES = [c for c in golden_cases() if c.startswith("hyp_als_")]
REL_CASES = [c for c in golden_cases() if c.startswith("hyp_rel_als_")]


def _learn(O, g, tr, te):
    m = g.model(O, "init")
    if "group" in g.z.files:
        group, wl, vl = g.z["group"], g.z["w_lambda_g"], np.repeat(g.z["v_lambda_g"][:, None], g.k, axis=1)
    else:
        group, wl, vl = None, [g.reg[1]], g.reg[2]
    G = len(np.atleast_1d(wl))
    mu = float(g.z["mu0"])
    pred, metric = O.als_learn_ex(m, tr, te, g.task, g.iters, wl, vl, g.min_target, g.max_target, group=group,
                                  alpha=float(g.z["alpha0"]), w_mu_g=np.full(G, mu), v_mu_gf=np.full((G, g.k), mu))
    out = np.clip(pred, g.min_target, g.max_target) if g.task == 0 else np.clip(pred, 0.0, 1.0)
    return m, out, metric


def test_fixtures_cover_the_prior_draws():
    assert len(CASES) >= 3 and REL_CASES
    for name in CASES:
        g = Golden(name)
        assert float(g.z["alpha0"]) != 1.0 and float(g.z["mu0"]) != 0.0
        ids_tr = g.z["train_entries"]["id"]
        seen = np.zeros(g.n, dtype=bool)
        seen[ids_tr] = True
        hole = np.flatnonzero(~seen[:ids_tr.max()])
        assert len(hole) >= 5, name                                  # no training column, inside the train's id range ...
        assert g.n > ids_tr.max() + 1, name                          # ... and above it
        assert np.isin(hole, g.z["test_entries"]["id"]).any(), name  # present in the test rows


@pytest.mark.parametrize("name", CASES)
def test_hyper_prior_als_bit_exact(oracle, name):
    O = oracle
    g = Golden(name)
    m, out, metric = _learn(O, g, g.data(O, "train"), g.data(O, "test"))
    assert m.w0 == float(g.z["final_w0"])
    assert np.array_equal(m.w, g.z["final_w"])
    assert np.array_equal(m.v, g.z["final_v"])
    assert np.array_equal(out, g.z["pred_out"])
    assert np.isfinite(metric).all()
    # the prior means reached the unseen features: with mu_0 != 0 their draws are mu_0 (sigma^2 = 1 / lambda, no data)
    seen = np.zeros(g.n, dtype=bool)
    seen[g.z["train_entries"]["id"]] = True
    np.testing.assert_allclose(m.w[~seen], float(g.z["mu0"]), rtol=1e-15)
    np.testing.assert_allclose(m.v[:, ~seen], float(g.z["mu0"]), rtol=1e-15)


@pytest.mark.parametrize("name", REL_CASES)
def test_hyper_prior_flat_als_equals_block_structured_reference(oracle, name):
    O = oracle
    g = Golden(name)
    tr, _ = flat(g, O, "train")
    te, _ = flat(g, O, "test")
    m, out, _ = _learn(O, g, tr, te)
    assert abs(m.w0 - float(g.z["final_w0"])) <= 1e-6 * max(1.0, abs(m.w0))
    np.testing.assert_allclose(m.w, g.z["final_w"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(m.v, g.z["final_v"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(out, g.z["pred_out"], rtol=1e-6, atol=1e-9)


def test_alpha_one_mu_zero_is_the_plain_sweep(oracle):
    """the generalised sweep at alpha = 1, mu = 0 (explicit tables) is the plain ALS sweep, bit for bit"""
    O = oracle
    g = Golden("als_reg_ml_groups")
    vl = np.repeat(g.z["v_lambda_g"][:, None], g.k, axis=1)
    m1, m2 = g.model(O, "init"), g.model(O, "init")
    tr, te = g.data(O, "train"), g.data(O, "test")
    p1, _ = O.als_learn_groups(m1, tr, te, g.task, g.iters, g.z["group"], g.z["w_lambda_g"], vl, g.min_target, g.max_target)
    p2, _ = O.als_learn_ex(m2, tr, te, g.task, g.iters, g.z["w_lambda_g"], vl, g.min_target, g.max_target, group=g.z["group"],
                           alpha=1.0, w_mu_g=np.zeros(2), v_mu_gf=np.zeros((2, g.k)))
    assert m1.w0 == m2.w0 and np.array_equal(m1.w, m2.w) and np.array_equal(m1.v, m2.v) and np.array_equal(p1, p2)


def test_noise_restatement_basics(oracle):
    """the keyed noise: stream layout disjoint for k <= 1024, and z = gauss_hash is N(0,1) with the 24-bit uniform's support"""
    O = oracle
    streams = {}
    for fam, fs in ((O.MCMC_V, range(1024)), (O.MCMC_W, [0]), (O.MCMC_W_UNSEEN, [0]), (O.MCMC_TARGETS, [0]), (O.MCMC_V_UNSEEN, range(1024))):
        for f in fs:
            s = O.mcmc_stream(3, fam, f)
            assert s not in streams, (fam, f, streams.get(s))
            streams[s] = (fam, f)
    assert max(streams) < O.mcmc_stream(4, O.MCMC_V, 0) and min(streams) >= O.mcmc_stream(3, O.MCMC_V, 0)
    z = O.gauss_hash(7, 11, np.arange(200000))
    assert abs(z.mean()) < 5 / np.sqrt(len(z)) and abs(z.var() - 1) < 5 * np.sqrt(2 / len(z))
    assert np.abs(z).max() < 5.8
    assert abs(np.corrcoef(z, O.gauss_hash(7, 12, np.arange(200000)))[0, 1]) < 5 / np.sqrt(len(z))
    assert O.w0_noise(1, 0) != O.w0_noise(1, 1) and O.w0_noise(5, 2) == O.w0_noise(5, 2)
