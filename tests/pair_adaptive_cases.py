"""Shared by tests/test_pair_adaptive_cpu.py and tests/test_gpu_pair_adaptive.py: the options of the parity tests, the
popularity-skewed case on which the plain pairwise batch rule diverges, and the float64 / float32 restatement runs
(libfm_amd/adaptive.py pair_epoch, libfm_amd/ftrl.py pair_epoch)."""
import functools

import numpy as np

import bpr_oracle as B
import datagen
from oracle import oracle as O

ADA = dict(eta=0.05, init_acc=1.0)
FTRL = dict(alpha=0.05, beta=1.0, l1_w=2.0, l1_v=1.0, l2_w=0.01, l2_v=0.02, init_acc=0.0)


def make_state(rule, m, opts=None):
    from libfm_amd import adaptive, ftrl
    if rule == "adagrad":
        return adaptive.AdaptState(m.n, m.k, (opts or ADA)["init_acc"])
    return ftrl.FtrlState(m, **(opts or FTRL))


def rule_epoch(rule, m, st, ent, rp, pa, pb, batch, step_dtype=np.float64, opts=None):
    """one epoch of the restatement in place on (m, st); returns the largest |change|"""
    from libfm_amd import adaptive, ftrl
    if rule == "adagrad":
        return adaptive.pair_epoch(m, ent, rp, pa, pb, (opts or ADA)["eta"], batch, st, step_dtype=step_dtype)
    return ftrl.pair_epoch(m, ent, rp, pa, pb, batch, st, step_dtype=step_dtype)


def restate(rule, m0, epochs_pairs, batch, step_dtype=np.float64, opts=None):
    """the restatement over a list of per-epoch (ent, rp, pa, pb) from the start model m0: (model, state)"""
    m = m0.copy()
    st = make_state(rule, m, opts)
    for ent, rp, pa, pb in epochs_pairs:
        rule_epoch(rule, m, st, ent, rp, pa, pb, batch, step_dtype, opts)
    return m, st


def state_arrays(rule, st):
    """the state as the device hands it out: adagrad (n_w, n_v); ftrl (z_w, z_v, n_w, n_v)"""
    return (st.n_w, st.n_v) if rule == "adagrad" else (st.z_w, st.z_v, st.n_w, st.n_v)


def gap(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) if a.size else 0.0


def step_gaps(rule, m0, epochs_pairs, batch, opts=None):
    """largest gaps between the restatement with the float32 step and with the float64 step: (theta, [one per state array])"""
    a, sa = restate(rule, m0, epochs_pairs, batch, np.float64, opts)
    b, sb = restate(rule, m0, epochs_pairs, batch, np.float32, opts)
    return max(gap(a.v, b.v), gap(a.w, b.w)), [gap(x, y) for x, y in zip(state_arrays(rule, sa), state_arrays(rule, sb))], (a, sa), (b, sb)


def pair_loss(m, ent, rp, pa, pb):
    return B.pair_metrics(B.pair_d(m, ent, rp, pa, pb))[1]


def start_model(n, k, k0=True, k1=True, reg=(0.01, 0.01, 0.02), seed=3):
    """tests/test_gpu_bpr.py's start model: fp32-exact values, w0 = 0.25, w and V ~ N(0, 0.1)"""
    rng = np.random.default_rng(seed)
    m = O.Model(n, k, k0, k1, *reg)
    m.w0 = 0.25
    m.w[:] = np.asarray(rng.normal(0, 0.1, n), np.float32)
    m.v[:] = np.asarray(rng.normal(0, 0.1, (k, n)), np.float32)
    return m


SKEW_ETA, SKEW_B = 0.5, 2048


@functools.lru_cache(maxsize=None)
def skewed_case():
    """48 users x 24 items, one row per (user, item) with two one-hot ids, item popularity proportional to 1 / (1 + i)^1.2; 2 048
    pairs of one user's two items preferring the one with the higher planted score; k = 8, V ~ N(0, 0.1) from seed 3, w = 0, no
    bias, reg (0, 0.001, 0.001).  Returns (entries, row_ptr, pair_a, pair_b, start model)."""
    nu, ni, P, k = 48, 24, 2048, 8
    ids = [[u, nu + i] for u in range(nu) for i in range(ni)]
    ent, rp, _ = datagen._pack(ids, [[1.0, 1.0]] * len(ids), [0.0] * len(ids))
    rng = np.random.default_rng(5)
    score = rng.normal(0, 1, (nu, 4)) @ rng.normal(0, 1, (4, ni)) + rng.normal(0, 0.5, ni)
    pop = 1.0 / (1.0 + np.arange(ni)) ** 1.2
    pop /= pop.sum()
    pa, pb = np.zeros(P, np.uint32), np.zeros(P, np.uint32)
    for t in range(P):
        u = int(rng.integers(0, nu))
        i, j = rng.choice(ni, 2, replace=False, p=pop)
        hi, lo = (i, j) if score[u, i] > score[u, j] else (j, i)
        pa[t], pb[t] = u * ni + hi, u * ni + lo
    m = O.Model(nu + ni, k, False, True, 0.0, 0.001, 0.001)
    m.v[:] = np.asarray(np.random.default_rng(3).normal(0, 0.1, (k, nu + ni)), np.float32)
    return ent, rp, pa, pb, m
