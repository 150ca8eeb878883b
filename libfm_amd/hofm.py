"""The third-order FM (the higher-order FM of Blondel et al., NIPS 2016, at order 3) restated in numpy: the CPU reference of
fmx_hofm_predict / fmx_hofm_epoch (include/fmx.h "fmx_hofm_*").

    y(x) = w0 + sum_j w_j x_j + sum_{c < k2} sum_{a<b} z_a z_b + sum_{c >= k2} sum_{a<b<d} z_a z_b z_d,     z_a = x_a v[c][j_a]

model.v is [k2 + k3][n]: rows [0, k2) are the pairwise factors, rows [k2, k2 + k3) the third-order factors; a, b, d are the row's
entries in row order, and an id repeated inside a row counts as separate entries.  With the power sums p_m[c] = sum_a z_a^m:
    E2 = 1/2 (p1^2 - p2)      E3 = 1/3 (E2 p1 - p1 p2 + p3) = (p1^3 - 3 p1 p2 + 2 p3) / 6      dE3/dv[c][j_a] = x_a (E2 - z_a p1 + z_a^2)
k3 = 0 is the plain FM.

One epoch is adaptive.epoch's batch rule with these sums: per batch, from the batch-start parameters, (1) the power sums and rest_e;
(2) the bias in micro-chunks (adaptive.bias_steps); (3) AdaGrad on w and every column of V on the accumulators of `state`, with
    g_jc = sum_occ mult_e x p1_e - v sum_occ mult_e x^2                                        [+ nocc regv v]     (c <  k2)
    g_jc = sum_occ mult_e x E2_e - v sum_occ mult_e x^2 p1_e + v^2 sum_occ mult_e x^3          [+ nocc regv v]     (c >= k2)"""
import numpy as np

from . import adaptive


def power_sums(model, data, r0, nb, dtype=np.float64):
    """(ids, xs, ex, p1, p2, p3), each p [nb][k], of rows [r0, r0 + nb) from the parameters `model` holds now"""
    row_ptr = data.row_ptr.astype(np.int64)
    a, b = row_ptr[r0], row_ptr[r0 + nb]
    ids = data.entries["id"][a:b].astype(np.int64)
    xs = data.entries["value"][a:b].astype(dtype)
    ex = np.repeat(np.arange(nb), np.diff(row_ptr[r0:r0 + nb + 1]))
    z = (model.v.astype(dtype)[:, ids].T * xs[:, None]).astype(dtype)               # [entries][k]
    ps = []
    for zm in (z, z * z, z * z * z):
        p = np.zeros((nb, int(model.k)), dtype=dtype)
        np.add.at(p, ex, zm)
        ps.append(p)
    return (ids, xs, ex) + tuple(ps)


def _split(model, k3):
    k3 = int(k3)
    if not 0 <= k3 <= int(model.k):
        raise ValueError("hofm: %d third-order factors in a model of %d columns" % (k3, int(model.k)))
    return int(model.k) - k3


def _rest(model, k2, ids, xs, ex, p1, p2, p3, dtype):
    """(y-hat minus the bias, E2[nb][k])"""
    Tp = np.dtype(dtype).type
    e2 = (Tp(0.5) * (p1 * p1 - p2)).astype(dtype)
    e3 = ((e2 * p1 - p1 * p2 + p3) / Tp(3)).astype(dtype)
    rest = (e2[:, :k2].sum(axis=1, dtype=dtype) + e3[:, k2:].sum(axis=1, dtype=dtype)).astype(dtype)
    if model.k1:
        np.add.at(rest, ex, model.w.astype(dtype)[ids] * xs)
    return rest, e2


def predict(model, k3, rows):
    """y-hat of every row (no clamp, as fmx_predict)"""
    k2 = _split(model, k3)
    ids, xs, ex, p1, p2, p3 = power_sums(model, rows, 0, int(rows.n_rows))
    return _rest(model, k2, ids, xs, ex, p1, p2, p3, np.float64)[0] + (model.w0 if model.k0 else 0.0)


def batch_gradients(model, k3, mult, ids, xs, ex, p1, e2, dtype=np.float64):
    """the gradient sums of sum_e mult_e y_e over a batch, without regularisation: (feats, nocc, g_w[feats], g_v[feats][k]);
    occurrences in row order"""
    k2 = _split(model, k3)
    feats, inv = np.unique(ids, return_inverse=True)
    nocc = np.bincount(inv, minlength=len(feats)).astype(dtype)
    mx = mult[ex] * xs
    mxx = mx * xs
    gw = np.zeros(len(feats), dtype=dtype)
    np.add.at(gw, inv, mx)
    H = np.concatenate([p1[:, :k2], e2[:, k2:]], axis=1)                            # an occurrence's first row ...
    G = np.zeros((len(feats), int(model.k)), dtype=dtype)
    G2 = np.zeros((len(feats), int(model.k)), dtype=dtype)
    A = np.zeros(len(feats), dtype=dtype)
    A3 = np.zeros(len(feats), dtype=dtype)
    np.add.at(G, inv, mx[:, None] * H[ex])
    np.add.at(G2, inv, mxx[:, None] * p1[ex])                                       # ... and its second, read in the columns >= k2
    np.add.at(A, inv, mxx)
    np.add.at(A3, inv, mxx * xs)
    vj = model.v.astype(dtype)[:, feats].T
    gv = G - vj * A[:, None]
    gv[:, k2:] = (G - vj * G2 + vj * vj * A3[:, None])[:, k2:]
    return feats, nocc, gw, gv.astype(dtype)


def epoch(model, state, k3, rows, task, lr, min_target, max_target, batch, w0_chunk, eta=None, dtype=np.float64):
    """one epoch, in place on model and state (adaptive.AdaptState of model.k = k2 + k3 columns).  eta None = lr.  dtype=np.float32 runs
    the sums, the products and the steps in fp32 (the bias stays a double, as on the device)."""
    Tp = np.dtype(dtype).type
    eta = Tp(lr if eta is None else eta)
    k2, n_rows = _split(model, k3), int(rows.n_rows)
    batch = n_rows if (batch == 0 or batch > n_rows) else int(batch)
    regw, regv = Tp(model.regw), Tp(model.regv)
    for r0 in range(0, n_rows, batch):
        nb = min(batch, n_rows - r0)
        ids, xs, ex, p1, p2, p3 = power_sums(model, rows, r0, nb, dtype)
        rest, e2 = _rest(model, k2, ids, xs, ex, p1, p2, p3, dtype)
        mult = adaptive.bias_steps(model, rest, rows.target[r0:r0 + nb], task, lr, min_target, max_target, batch, w0_chunk, dtype)
        feats, nocc, gw, gv = batch_gradients(model, k3, mult, ids, xs, ex, p1, e2, dtype)
        if model.k1:
            wj = model.w.astype(dtype)[feats]
            gw = gw + nocc * regw * wj
            nw = (state.n_w[feats].astype(dtype) + gw * gw).astype(dtype)
            state.n_w[feats] = nw
            model.w[feats] = (wj - eta * gw / np.sqrt(nw)).astype(dtype)
        vj = model.v.astype(dtype)[:, feats].T                                      # [feats][k]
        gv = gv + nocc[:, None] * regv * vj
        nv = (state.n_v[:, feats].T.astype(dtype) + gv * gv).astype(dtype)
        state.n_v[:, feats] = nv.T
        model.v[:, feats] = (vj - eta * gv / np.sqrt(nv)).astype(dtype).T
