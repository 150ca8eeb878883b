"""The data of the DeepFM tests: ragged rows with real values over 600 features in F fields -- every 9th row empty, a repeated id in every
row of two and more -- a model whose V keeps |x v| below about 0.5, and a start net whose b1 stays 0.45 off zero (S W1 has a standard
deviation of 0.12 and reaches 0.9: of the 8 / 24 / 80 units 1 / 7 / 11 change their mask from row to row, the others are on or off
throughout).  TRAIN lists the training cases of tests/test_gpu_dfm.py; tests/test_dfm_cpu.py holds each of them to the kink condition,
which the seed below was chosen to meet (closest approach over all cases: 1.02e-4)."""
import numpy as np

import datagen

N = 600
LR, ETA, ROWS_T = 0.01, 0.05, 503
SHAPES = [(4, 3, 8), (5, 17, 24), (3, 33, 80)]
# (k, F, H, batch, task, rows): three epochs each; the last two: 2 233 rows in one batch, past FMFM_MSPLIT x FMFM_MCHUNK = 1 024
TRAIN = [s + (b, t, ROWS_T) for s in SHAPES for b in (1, 7, 0, 202) for t in (0, 1)] + [(5, 17, 24, 0, t, 2233) for t in (0, 1)]


def make(O, k, F, H, task=0, rows=300, seed=9):
    from libfm_amd import dfm
    ent, row_ptr, y = datagen.ragged_real(N, rows, 10, seed + 131 * k + F, classification=bool(task), empty_every=9, duplicates=True)
    rng = np.random.default_rng(seed + 7 * k + F + 1000 * H)
    m = O.Model(N, k, True, True, 0.01, 0.002, 0.001)
    m.v[:], m.w[:], m.w0 = rng.normal(0.0, 0.1, size=(k, N)), rng.normal(0.0, 0.05, size=N), 0.03
    groups = (np.arange(N) % F).astype(np.uint32)
    return m, groups, dfm.random_net(F, k, H, rng), O.Data(ent, row_ptr, y if task else np.clip(y, -1.0, 1.0))


def train_reference(O, case, dtype=np.float64):
    """three epochs of dfm.epoch on a training case: (model, state, net, n_net, groups, data, the smallest |pre-activation| met)"""
    from libfm_amd import adaptive, dfm
    k, F, H, batch, task, rows = case
    m, groups, net, d = make(O, k, F, H, task, rows)
    st, n_net = adaptive.AdaptState(m.n, k, 1.0), tuple(np.ones_like(a) for a in net)
    closest = min(dfm.epoch(m, st, net, n_net, groups, d, task, LR, -1.0, 1.0, batch, 16, eta=ETA, dtype=dtype) for _ in range(3))
    return m, st, net, n_net, groups, d, closest
