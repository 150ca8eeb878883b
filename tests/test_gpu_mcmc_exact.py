"""GPU: the Gibbs sampler (fmx_als_sweep with do_sample = 1, FMLearnMCMC) draw for draw against the fp64 oracle.

The coordinate noise is a counter hash keyed by (seed, stream of the (sweep, family), global feature id) and the bias noise a
seeded std::mt19937_64, so a sampled chain is deterministic and oracle/fm_oracle_als.c follows it (fmo_als_learn_ex with the
keyed noise of oracle/fm_oracle_noise.c).  The oracle's sweep at alpha != 1 and mu != 0 is pinned against the real reference
(tests/test_oracle_als_hyper.py); here the device is held to it at the tolerances of tests/test_gpu_als.py: rtol 1e-4, atol 2e-5
on parameters, 5e-5 on predictions.  The host's logf / cosf differ from the device's __logf / __cosf by at most ~1.4e-6 in z; the
noise test below measures that gap directly."""
import io

import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

RTOL, ATOL, ATOL_PRED = 1e-4, 2e-5, 5e-5


def _split(monkeypatch, v):
    from libfm_amd import capi as _c
    monkeypatch.setattr(_c, "ALS_SPLIT_MIN", _c.ALS_SPLIT_NEVER if str(v) == "0" else int(v))


@pytest.fixture(params=["fused", "split"])
def draw_form(request, monkeypatch):
    """fused draws, or the split step (k_als_rows) forced on every level"""
    _split(monkeypatch, "1" if request.param == "split" else "0")
    return request.param


def _handle(n, k, task, k0, k1, reg0, lo, hi, groups=None, world=1):
    from libfm_amd import capi
    if world == 1:
        h = capi.Handle(n, k, k0, k1, task, reg0, 0.0, 0.0, 0.0, lo, hi)
        h.set_groups(groups)
        return h, [h]
    shards = [capi.Handle(n, k, k0, k1, task, reg0, 0.0, 0.0, 0.0, lo, hi, device=0, shard_rank=r, shard_world=world, shard_hash=1)
              for r in range(world)]
    for s in shards:
        s.set_groups(groups)
    return capi.Group(shards), shards


def _device_chain(h, m, ent, rp, y, sweeps, wl, vl, alpha, wmu, vmu, do_sample, seed, rel=None):
    h.set_params(m.w0, m.w, m.v)
    if rel is None:
        h.upload_rows(0, ent, rp, y)
    else:
        h.upload_block_rows(0, ent, rp, y, rel, keep=True)
    h.als_begin(0)
    for _ in range(sweeps):
        h.als_sweep(wl, vl, alpha, wmu, vmu, do_sample, seed)
    yhat = h.predict(0, len(y))
    h.als_end()
    w0, w, v = h.get_params()
    return w0, w, v, yhat


def _close(handles):
    for x in handles:
        x.close()


def _data(n_feat, n, rows, seed, task, hole=(40, 25)):
    """one-hot field rows over n_feat ids, the ids from hole[0] on moved up by hole[1] (no training column in the middle), in a
    model of n > every train id (none above the train's maximum either)"""
    ent, rp, y = datagen.onehot_fields(n_feat, 6, rows, seed=seed, classification=bool(task))
    ent = ent.copy()
    ent["id"] = np.where(ent["id"] >= hole[0], ent["id"] + hole[1], ent["id"]).astype(np.uint32)
    assert int(ent["id"].max()) + 1 < n
    return ent, rp, y


def _priors(rng, G, k):
    wl = rng.uniform(0.5, 4.0, G)
    wmu = rng.uniform(-0.4, 0.4, G)
    vl = rng.uniform(1.0, 8.0, (G, k))
    vmu = rng.uniform(-0.3, 0.3, (G, k))
    return wl, wmu, vl, vmu


def _oracle_chain(O, m, ent, rp, y, task, sweeps, groups, wl, vl, alpha, wmu, vmu, do_sample, seed, lo, hi):
    d = O.Data(ent, rp, y)
    O.als_learn_ex(m, d, d, task, sweeps, wl, vl, lo, hi, group=groups, alpha=alpha, w_mu_g=wmu, v_mu_gf=vmu,
                   do_sample=do_sample, seed=seed)
    return O.predict_raw(m, d)


def _assert_model(w0, w, v, yhat, m, want_yhat):
    assert abs(w0 - m.w0) <= RTOL * abs(m.w0) + ATOL, (w0, m.w0)
    np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(yhat, want_yhat, rtol=RTOL, atol=ATOL_PRED)


# ---- the noise itself ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 3])
def test_unseen_draws_are_the_keyed_noise(oracle, G):
    """mu = 0, lambda = 1: a feature without a training column is drawn as z itself (k_als_unseen, k_als_unseen_v -- one group
    takes a separate fast path).  Every unseen w and v_f against the oracle's gauss_hash under the stream of its family."""
    O = oracle
    n, k, rows, seed = 5000, 33, 64, 4321
    ent = np.zeros(rows, dtype=O.ENTRY_DTYPE)
    ent["id"] = np.arange(rows, dtype=np.uint32) * 7                # every 7th feature below 448 has a column
    ent["value"] = 1.0
    rp = np.arange(rows + 1, dtype=np.uint64)
    groups = None if G == 1 else (np.arange(n) % G).astype(np.uint32)
    h, hs = _handle(n, k, 0, True, True, 0.0, -1.0, 1.0, groups)
    m = O.Model(n, k)
    w0, w, v, _ = _device_chain(h, m, ent, rp, np.zeros(rows, dtype=np.float32), 1, 1.0, 1.0, 1.0, 0.0, 0.0, True, seed)
    _close(hs)
    unseen = np.setdiff1d(np.arange(n), ent["id"])
    # the gap between host logf / cosf and the device's __logf / __cosf: <= 1.4e-6 measured over these 167 824 draws (fp32 rounding of
    # the stored value included); a wrong key, stream or scale is an O(1) difference
    tol = dict(rtol=0, atol=3e-6)
    np.testing.assert_allclose(w[unseen], O.gauss_hash(seed, O.mcmc_stream(0, O.MCMC_W_UNSEEN), unseen), **tol)
    for f in range(k):
        np.testing.assert_allclose(v[f, unseen], O.gauss_hash(seed, O.mcmc_stream(0, O.MCMC_V_UNSEEN, f), unseen), err_msg="factor %d" % f, **tol)


# ---- deterministic sweeps at alpha != 1, mu != 0 -------------------------------------------------------------------------------

VARIANTS = {1: (0, 1, 1), 8: (1, 1, 1), 33: (0, 0, 1), 64: (1, 1, 0), 100: (0, 1, 1), 300: (1, 0, 0)}   # k: (task, k0, k1)


@pytest.mark.parametrize("k", sorted(VARIANTS))
def test_hyper_prior_sweep_matches_oracle(oracle, k, draw_form):
    """do_sample = 0 with alpha = 1.7, per-group w_mu / w_lambda and per-(group, factor) v_mu / v_lambda: the alpha * sum h^2 and
    mu * lambda terms of k_als_draw, the split step, the prior draws of features without a column (middle and top of the id
    range) and the w0 draw.  k covers several padded row widths and the wide rows that re-predict through LDS."""
    O = oracle
    task, k0, k1 = VARIANTS[k]
    n, G = 700, 2
    ent, rp, y = _data(600, n, 500, 70 + k, task)
    groups = (np.arange(n) >= 300).astype(np.uint32)
    wl, wmu, vl, vmu = _priors(np.random.default_rng(k), G, k)
    m = O.Model(n, k, bool(k0), bool(k1), 0.3)
    m.v[:] = O.init_values(3 + k, n, k, 0.1)
    m.w[:] = O.init_values(5 + k, n, 1, 0.1)[0]
    m.w0 = 0.2
    lo, hi = float(y.min()), float(y.max())
    h, hs = _handle(n, k, task, k0, k1, 0.3, lo, hi, groups)
    got = _device_chain(h, m, ent, rp, y, 3, wl, vl, 1.7, wmu, vmu, False, 0)
    _close(hs)
    want_yhat = _oracle_chain(O, m, ent, rp, y, task, 3, groups, wl, vl, 1.7, wmu, vmu, False, 0, lo, hi)
    _assert_model(*got, m, want_yhat)
    unseen = np.setdiff1d(np.arange(n), ent["id"])
    if k1:                                                          # the prior draw of a feature without a column is its mean
        np.testing.assert_allclose(got[1][unseen], wmu[groups[unseen]], rtol=1e-6)


# ---- sampled chains ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("task,k", [(0, 8), (1, 8), (0, 64), (1, 40)])
def test_sampled_chain_matches_oracle(oracle, task, k, draw_form):
    """4 sweeps of the Gibbs chain (fixed hyper-parameters, alpha = 1.3, prior means per group and factor): every coordinate
    draw, the w0 draw and -- probit -- the truncated-normal targets, against the oracle driven by the same keyed noise"""
    O = oracle
    n, G, seed = 700, 2, 2024 + k
    ent, rp, y = _data(600, n, 500, 90 + k + task, task)
    groups = (np.arange(n) % 2).astype(np.uint32)
    wl, wmu, vl, vmu = _priors(np.random.default_rng(7 + k), G, k)
    m = O.Model(n, k, True, True, 0.5)
    m.v[:] = O.init_values(11, n, k, 0.1)
    m.w[:] = O.init_values(12, n, 1, 0.1)[0]
    lo, hi = float(y.min()), float(y.max())
    h, hs = _handle(n, k, task, True, True, 0.5, lo, hi, groups)
    got = _device_chain(h, m, ent, rp, y, 4, wl, vl, 1.3, wmu, vmu, True, seed)
    _close(hs)
    init_v = m.v.copy()
    want_yhat = _oracle_chain(O, m, ent, rp, y, task, 4, groups, wl, vl, 1.3, wmu, vmu, True, seed, lo, hi)
    assert np.abs(m.v - init_v).max() > 0.1                        # the chain moved
    _assert_model(*got, m, want_yhat)


def test_sampled_chain_on_kept_blocks_matches_oracle(oracle):
    """relation blocks kept apart (k_rel_draw over per-block-row caches) against the oracle's sampled chain on the joined rows"""
    from common import Golden
    from test_oracle_relations import flat
    from test_gpu_relations import blocks_of
    O = oracle
    g = Golden("hyp_rel_als_reg")
    z = g.z
    offs = [int(z["n_main"])]
    for _, _, nf in blocks_of(z)[:-1]:
        offs.append(offs[-1] + nf)
    rel = [(be, bp, z["rel%d_train" % i], off) for i, ((be, bp, _), off) in enumerate(zip(blocks_of(z), offs))]
    alpha, mu, seed = float(z["alpha0"]), float(z["mu0"]), 77
    m = g.model(O, "init")
    h, hs = _handle(g.n, g.k, g.task, True, True, g.reg[0], g.min_target, g.max_target)
    got = _device_chain(h, m, z["train_entries"], z["train_row_ptr"], g.train_target, 3, g.reg[1], g.reg[2], alpha, mu, mu, True, seed, rel=rel)
    _close(hs)
    tr, _ = flat(g, O, "train")
    seen = np.zeros(g.n, dtype=np.uint8)                            # the device's columns: main train ids, every block attribute
    seen[z["train_entries"]["id"]] = 1
    for (be, _, _, off) in rel:
        seen[be["id"].astype(np.int64) + off] = 1
    O.als_learn_ex(m, tr, tr, g.task, 3, [g.reg[1]], g.reg[2], g.min_target, g.max_target, alpha=alpha, w_mu_g=[mu],
                   v_mu_gf=np.full((1, g.k), mu), do_sample=True, seed=seed, seen=seen)
    assert np.abs(m.v - g.model(O, "init").v).max() > 0.05
    _assert_model(*got, m, O.predict_raw(m, tr))


@pytest.mark.parametrize("world", [2, 3])
def test_sampled_chain_on_feature_shards_matches_oracle(oracle, world):
    """two and three feature shards on one device (capi.Group): the noise is keyed by the GLOBAL id, so the sharded chain is the
    oracle's chain"""
    O = oracle
    n, k, G, seed, task = 700, 8, 2, 99, 1
    ent, rp, y = _data(600, n, 500, 130 + world, task)
    groups = (np.arange(n) >= 350).astype(np.uint32)
    wl, wmu, vl, vmu = _priors(np.random.default_rng(world), G, k)
    m = O.Model(n, k, True, True, 0.5)
    m.v[:] = O.init_values(21, n, k, 0.1)
    m.w[:] = O.init_values(22, n, 1, 0.1)[0]
    h, hs = _handle(n, k, task, True, True, 0.5, -1.0, 1.0, groups, world=world)
    got = _device_chain(h, m, ent, rp, y, 3, wl, vl, 1.4, wmu, vmu, True, seed)
    h.close()
    _close(hs)
    want_yhat = _oracle_chain(O, m, ent, rp, y, task, 3, groups, wl, vl, 1.4, wmu, vmu, True, seed, -1.0, 1.0)
    _assert_model(*got, m, want_yhat)


# ---- the whole learner: hyper-prior draws on the host ---------------------------------------------------------------------------

class _Recorder:
    """wraps the learner's numpy generator: every gamma / standard_normal call with its variates"""

    def __init__(self, seed):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.calls = []

    def gamma(self, shape):
        x = self.rng.gamma(shape)
        self.calls.append(("gamma", np.array(shape, dtype=np.float64, copy=True), np.array(x, dtype=np.float64, copy=True)))
        return x

    def standard_normal(self, size=None):
        x = self.rng.standard_normal(size)
        self.calls.append(("normal", size, np.array(x, dtype=np.float64, copy=True)))
        return x


@pytest.mark.parametrize("grouped", [False, True])
def test_mcmc_learner_matches_oracle(oracle, monkeypatch, grouped):
    """FMLearnMCMC, 3 iterations: the recorded variates of the learner's generator are fed to a restatement of draw_alpha,
    draw_w_lambda, draw_w_mu, draw_v_lambda and draw_v_mu in the reference's loop form and order (fm_learn_mcmc.h:911-1097; w_lambda
    from the old w_mu, w_mu from the new w_lambda), with the rates from the oracle's own fp64 model; the sweeps are the oracle's
    sampled chain.  alpha, w_mu and w_lambda per iteration, the final v_mu and v_lambda, the parameters and pred_sum_all must match."""
    from libfm_amd import learner as L
    O = oracle
    n, k, iters, seed = 400, 6, 3, 5
    ent, rp, y = datagen.movielens_shaped(150, 100, 900, seed=31)
    ent2, rp2, y2 = datagen.movielens_shaped(150, 100, 200, seed=32)
    n = max(n, int(ent["id"].max()) + 1, int(ent2["id"].max()) + 1)
    groups = (np.arange(n) >= 150).astype(np.uint32) if grouped else None
    G = 2 if grouped else 1
    lo, hi = float(y.min()), float(y.max())
    m = O.Model(n, k, True, True, 0.0)
    m.v[:] = O.init_values(41, n, k, 0.1)
    fm = L.FMModel()
    fm.num_attribute, fm.num_factor = n, k
    fm.w0, fm.w, fm.v = m.w0, m.w.copy(), m.v.copy()
    l = L.FMLearnMCMC()
    l.fm, l.task, l.num_iter, l.min_target, l.max_target, l.seed = fm, 0, iters, lo, hi, seed
    l.w_lambda, l.v_lambda, l.groups = 2.0, 3.0, groups
    l.out = io.StringIO()
    l.init()
    rec = []
    monkeypatch.setattr(L.np.random, "default_rng", lambda s: rec.append(_Recorder(s)) or rec[-1])
    l.learn(L.Data(ent, rp, y), L.Data(ent2, rp2, y2))
    monkeypatch.undo()
    l.close()
    assert len(rec) == 1
    calls = rec[0].calls
    assert len(calls) == 5 * iters
    # the oracle: the reference's hyper-prior step from ITS model, then its sampled sweep
    a0 = g0 = b0 = 1.0
    m0 = 0.0
    grp = np.zeros(n, dtype=np.int64) if groups is None else groups.astype(np.int64)
    n_g = np.bincount(grp, minlength=G).astype(np.float64)
    N = len(y)
    tr, te = O.Data(ent, rp, y), O.Data(ent2, rp2, y2)
    w_mu, w_lambda = np.zeros(G), np.full(G, 2.0)
    v_mu, v_lambda = np.zeros((G, k)), np.full((G, k), 3.0)
    pred_sum = np.zeros(len(y2))
    for it in range(iters):
        (c_a, c_wl, c_wm, c_vl, c_vm) = calls[5 * it:5 * it + 5]
        assert c_a[0] == "gamma" and c_a[1] == (a0 + N) / 2.0                             # draw_alpha :916-922
        e = O.predict_raw(m, tr) - y
        gamma_n = g0
        for c in range(N):
            gamma_n += e[c] * e[c]
        alpha = float(c_a[2]) / (gamma_n / 2.0)
        assert abs(l.log[it]["alpha"] - alpha) <= RTOL * alpha
        assert c_wl[0] == "gamma" and np.array_equal(c_wl[1], (a0 + n_g + 1) / 2.0)       # draw_w_lambda :985-997
        gam = b0 * (w_mu - m0) * (w_mu - m0) + g0
        for i in range(n):
            gam[grp[i]] += (m.w[i] - w_mu[grp[i]]) * (m.w[i] - w_mu[grp[i]])
        w_lambda = c_wl[2] / (gam / 2.0)
        assert c_wm[0] == "normal"                                                         # draw_w_mu :946-959, new w_lambda
        s = np.zeros(G)
        for i in range(n):
            s[grp[i]] += m.w[i]
        w_mu = (s + b0 * m0) / (n_g + b0) + c_wm[2] * np.sqrt(1.0 / ((n_g + b0) * w_lambda))
        assert c_vl[0] == "gamma" and np.array_equal(np.asarray(c_vl[1])[:, 0], (a0 + n_g + 1) / 2.0)
        gam = b0 * (v_mu - m0) * (v_mu - m0) + g0                                          # draw_v_lambda :1065-1080
        for f in range(k):
            for i in range(n):
                gam[grp[i], f] += (m.v[f, i] - v_mu[grp[i], f]) ** 2
        v_lambda = c_vl[2] / (gam / 2.0)
        sv = np.zeros((G, k))                                                              # draw_v_mu :1026-1039
        for f in range(k):
            for i in range(n):
                sv[grp[i], f] += m.v[f, i]
        v_mu = (sv + b0 * m0) / (n_g[:, None] + b0) + c_vm[2] * np.sqrt(1.0 / ((n_g[:, None] + b0) * v_lambda))
        for g in range(G):
            np.testing.assert_allclose([l.log[it]["wmu[%d]" % g], l.log[it]["wlambda[%d]" % g]], [w_mu[g], w_lambda[g]], rtol=RTOL, atol=ATOL)
        O.als_learn_ex(m, tr, tr, 0, 1, w_lambda, v_lambda, lo, hi, group=groups, alpha=alpha, w_mu_g=w_mu, v_mu_gf=v_mu,
                       do_sample=True, seed=seed * 7919 + 13, iter0=it)
        pred_sum += np.clip(O.predict_raw(m, te), lo, hi)
    np.testing.assert_allclose(l.v_mu[:, :k], v_mu, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(l.v_lambda_last, v_lambda, rtol=RTOL)
    assert abs(l.fm.w0 - m.w0) <= RTOL * abs(m.w0) + ATOL
    np.testing.assert_allclose(l.fm.w, m.w, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(l.fm.v, m.v, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(l.pred_sum_all, pred_sum, rtol=RTOL, atol=iters * ATOL_PRED)


# ---- independence of the noise families ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [520, 1010])
def test_noise_families_are_independent(oracle, k):
    """every (sweep, family) draws from its own stream: the linear weights and each factor, of the features with and without a
    training column, must be uncorrelated over the features (|r| < 5 / sqrt(n)).  With streams iter * 1024 + {f, 1000, 1001,
    512 + f} an unseen w_j and v_{j,489} were the same N(0,1) draw for k >= 490, and a seen w_j and v_{j,1000} for k >= 1001."""
    O = oracle
    n, n_seen, seed = 4000, 1000, 555
    perm = np.random.default_rng(3).permutation(n_seen).astype(np.uint32)
    ent = np.zeros(n_seen, dtype=O.ENTRY_DTYPE)
    ent["id"] = perm                                                # 250 rows x 4 distinct features: ids 0 .. 999 seen once each
    ent["value"] = 0.01                                             # tiny values: a seen draw is ~ its noise as well
    rp = np.arange(0, n_seen + 1, 4, dtype=np.uint64)
    h, hs = _handle(n, k, 0, False, True, 0.0, -1.0, 1.0)
    m = O.Model(n, k, False, True)
    _, w, v, _ = _device_chain(h, m, ent, rp, np.zeros(len(rp) - 1, dtype=np.float32), 1, 1.0, 1.0, 1.0, 0.0, 0.0, True, seed)
    _close(hs)
    seen = np.zeros(n, dtype=bool)
    seen[perm] = True
    for name, sel in (("seen", seen), ("unseen", ~seen)):
        cnt = int(sel.sum())
        ws = (w[sel] - w[sel].mean()) / w[sel].std()
        vs = v[:, sel]
        vs = (vs - vs.mean(axis=1, keepdims=True)) / vs.std(axis=1, keepdims=True)
        r = vs @ ws / cnt                                           # corr(w, v_f) for every f
        bad = np.flatnonzero(np.abs(r) >= 5 / np.sqrt(cnt))
        assert len(bad) == 0, "%s features: w correlates with v_f for f = %s (r = %s)" % (name, bad[:5], r[bad[:5]])
        rf = np.einsum("fi,fi->f", vs[:-1], vs[1:]) / cnt           # neighbouring factors
        assert np.abs(rf).max() < 5 / np.sqrt(cnt), name
