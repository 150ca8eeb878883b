"""The data set of the FwFM tests: 203 rows over 600 features in F fields, non-unit values; in front the rows that reach every edge of k_fwfm_rows:
empty, one entry, all entries in one field, one field with more entries than a wave-wide round (70 > 64: also the long row), a repeated id."""
import numpy as np

N = 600


def make(O, k, F, task=0, seed=5):
    rng = np.random.default_rng(seed + 131 * k + F)
    groups = (np.arange(N) % F).astype(np.uint32)
    in0 = np.flatnonzero(groups == 0)
    rows = [[], [(17, 1.5)], [(int(j), 0.5 + 0.1 * i) for i, j in enumerate(in0[:6])],
            [(int(in0[i % len(in0)]), 0.25 + 0.01 * i) for i in range(70)], [(3, 1.0), (40, -0.5), (3, 2.0)]]
    for _ in range(198):
        ids = rng.integers(0, N, size=int(rng.integers(1, 13)))
        rows.append([(int(j), float(x)) for j, x in zip(ids, rng.uniform(-2.0, 2.0, size=len(ids)))])
    y = rng.uniform(-1.0, 1.0, size=len(rows))
    data = O.Data.from_rows(rows, np.where(y < 0, -1.0, 1.0) if task else y)
    m = O.Model(N, k, True, True, 0.01, 0.002, 0.001)
    m.v[:] = rng.normal(0.0, 0.1, size=(k, N))
    m.w[:] = rng.normal(0.0, 0.05, size=N)
    m.w0 = 0.03
    r = rng.normal(0.5, 1.0, size=(F, F))
    r = 0.5 * (r + r.T)
    r[np.abs(r) < 0.2] = 0.0                                     # (some pairs of fields do not interact; others repel)
    return m, groups, r, data
