"""The data of the third-order FM's tests: ragged rows with real values over 700 features -- every 9th row empty, rows of one and two
entries, a repeated id in every row of two and more -- and a model of k2 + k3 columns whose V keeps |x v| below about 0.5."""
import numpy as np

import datagen

N = 700


def make(O, k2, k3, task=0, rows=300, seed=11):
    ent, row_ptr, y = datagen.ragged_real(N, rows, 10, seed + k2 + 131 * k3, classification=bool(task), empty_every=9, duplicates=True)
    rng = np.random.default_rng(seed + 7 * k2 + k3)
    m = O.Model(N, k2 + k3, True, True, 0.01, 0.002, 0.001)
    m.v[:], m.w[:], m.w0 = rng.normal(0.0, 0.1, size=(k2 + k3, N)), rng.normal(0.0, 0.05, size=N), 0.03
    return m, O.Data(ent, row_ptr, y if task else np.clip(y, -1.0, 1.0))
