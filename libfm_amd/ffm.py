"""The field-aware FM (FFM; Juan et al., RecSys 2016) restated in numpy: the CPU reference of fmx_ffm_predict / fmx_ffm_epoch
(include/fmx.h "fmx_ffm_*").

    y(x) = w0 + sum_j w_j x_j + sum_{a<b} < v_ja[g(jb)], v_jb[g(ja)] > x_a x_b          (a, b: the row's entries, in row order)

groups[j] = g(j) is feature j's field, F the number of fields, k_f the latent factors per vector.  model.v is [F k_f][n]: row
c = h k_f + f is factor f of the vector a feature uses against field h; v_j[h] is that block of k_f values.  With the field tile
Q[h] = sum_{b: g(jb) = h} x_b V[jb] of a row (Q[h][g]: block g of row h) and D = sum_b x_b^2 |v_jb[g(jb)]|^2:
    pair term = 1/2 sum_{g,h} <Q[h][g], Q[g][h]> - 1/2 D          d/dv_ja[h] = x_a (Q[h][g(ja)] - [h = g(ja)] x_a v_ja[g(ja)])
An id repeated inside a row counts as separate entries.  F = 1 is the plain FM of width k_f.

One epoch is adaptive.epoch's batch rule with these sums: per batch, from the batch-start parameters, (1) Q, D and rest_e; (2) the
bias in micro-chunks (adaptive.bias_steps); (3) AdaGrad on w and every column of V on the accumulators of `state`, with
g_jc = sum_occ mult_e x (Qt_e[g(j)][c] - [c in block g(j)] v_jc x) + nocc regv v_jc, Qt_e[g] = (Q_e[0][g], ..., Q_e[F-1][g]).
This is the library's minibatch rule, not libffm's online loop, and there is no instance normalisation."""
import numpy as np

from . import adaptive


def field_tiles(model, groups, k_f, data, r0, nb, F, dtype=np.float64):
    """(ids, xs, ex, fld, Q[nb][F][F][k_f], D[nb]) of rows [r0, r0 + nb) from the parameters `model` holds now; Q[e][h][g] is block g
    of the example's tile row h"""
    row_ptr = data.row_ptr.astype(np.int64)
    a, b = row_ptr[r0], row_ptr[r0 + nb]
    ids = data.entries["id"][a:b].astype(np.int64)
    xs = data.entries["value"][a:b].astype(dtype)
    ex = np.repeat(np.arange(nb), np.diff(row_ptr[r0:r0 + nb + 1]))
    fld = np.asarray(groups, dtype=np.int64)[ids]
    d = (model.v.astype(dtype)[:, ids].T * xs[:, None]).reshape(len(ids), F, k_f)    # [entries][field][k_f]
    Q = np.zeros((nb, F, F, k_f), dtype=dtype)
    np.add.at(Q, (ex, fld), d)
    own = d[np.arange(len(ids)), fld]                                               # the block an entry uses against its own field
    D = np.zeros(nb, dtype=dtype)
    np.add.at(D, ex, (own * own).sum(axis=1, dtype=dtype))
    return ids, xs, ex, fld, Q, D


def _rest(model, ids, xs, ex, Q, D, dtype):
    """y-hat minus the bias"""
    Tp = np.dtype(dtype).type
    rest = (Tp(0.5) * (Q * Q.transpose(0, 2, 1, 3)).sum(axis=(1, 2, 3), dtype=dtype) - Tp(0.5) * D).astype(dtype)
    if model.k1:
        np.add.at(rest, ex, model.w.astype(dtype)[ids] * xs)
    return rest


def _fields(groups, k_f, model):
    F = int(model.k) // int(k_f)
    if int(k_f) < 1 or F * int(k_f) != int(model.k) or (len(groups) and int(np.max(groups)) >= F):
        raise ValueError("ffm: the model's %d columns are not (fields of `groups`) x k_f = %d" % (int(model.k), int(k_f)))
    return F


def predict(model, groups, k_f, rows):
    """y-hat of every row (no clamp, as fmx_predict)"""
    F, nb = _fields(groups, k_f, model), int(rows.n_rows)
    ids, xs, ex, _, Q, D = field_tiles(model, groups, k_f, rows, 0, nb, F)
    return _rest(model, ids, xs, ex, Q, D, np.float64) + (model.w0 if model.k0 else 0.0)


def batch_gradients(model, groups, k_f, mult, ids, xs, ex, fld, Q, dtype=np.float64):
    """the gradient sums of sum_e mult_e y_e over a batch, without regularisation: (feats, nocc, g_w[feats], g_v[feats][F k_f]);
    occurrences in row order"""
    F = Q.shape[1]
    feats, inv = np.unique(ids, return_inverse=True)
    nocc = np.bincount(inv, minlength=len(feats)).astype(dtype)
    me_x = mult[ex] * xs
    gw = np.zeros(len(feats), dtype=dtype)
    np.add.at(gw, inv, me_x)
    Qt = Q[ex, :, fld].reshape(len(ids), F * k_f)                                   # an occurrence's row: (Q[0][g], ..., Q[F-1][g])
    G = np.zeros((len(feats), F * k_f), dtype=dtype)
    A = np.zeros(len(feats), dtype=dtype)
    np.add.at(G, inv, me_x[:, None] * Qt)
    np.add.at(A, inv, me_x * xs)
    own = (np.arange(F * k_f)[None, :] // k_f) == np.asarray(groups, dtype=np.int64)[feats][:, None]
    gv = G - model.v.astype(dtype)[:, feats].T * np.where(own, A[:, None], np.dtype(dtype).type(0))
    return feats, nocc, gw, gv


def epoch(model, state, groups, k_f, rows, task, lr, min_target, max_target, batch, w0_chunk, eta=None, dtype=np.float64):
    """one epoch, in place on model and state (adaptive.AdaptState of model.k = F k_f columns).  eta None = lr.  dtype=np.float32 runs
    the sums, the products and the steps in fp32 (the bias stays a double, as on the device)."""
    Tp = np.dtype(dtype).type
    eta = Tp(lr if eta is None else eta)
    F, n_rows = _fields(groups, k_f, model), int(rows.n_rows)
    batch = n_rows if (batch == 0 or batch > n_rows) else int(batch)
    regw, regv = Tp(model.regw), Tp(model.regv)
    for r0 in range(0, n_rows, batch):
        nb = min(batch, n_rows - r0)
        ids, xs, ex, fld, Q, D = field_tiles(model, groups, k_f, rows, r0, nb, F, dtype)
        rest = _rest(model, ids, xs, ex, Q, D, dtype)
        mult = adaptive.bias_steps(model, rest, rows.target[r0:r0 + nb], task, lr, min_target, max_target, batch, w0_chunk, dtype)
        feats, nocc, gw, gv = batch_gradients(model, groups, k_f, mult, ids, xs, ex, fld, Q, dtype)
        if model.k1:
            wj = model.w.astype(dtype)[feats]
            gw = gw + nocc * regw * wj
            nw = (state.n_w[feats].astype(dtype) + gw * gw).astype(dtype)
            state.n_w[feats] = nw
            model.w[feats] = (wj - eta * gw / np.sqrt(nw)).astype(dtype)
        vj = model.v.astype(dtype)[:, feats].T                                      # [feats][F k_f]
        gv = gv + nocc[:, None] * regv * vj
        nv = (state.n_v[:, feats].T.astype(dtype) + gv * gv).astype(dtype)
        state.n_v[:, feats] = nv.T
        model.v[:, feats] = (vj - eta * gv / np.sqrt(nv)).astype(dtype).T
