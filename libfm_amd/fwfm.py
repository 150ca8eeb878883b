"""The field-weighted FM (Pan et al., WWW 2018) restated in numpy: the CPU reference of fmx_fwfm_predict / fmx_fwfm_epoch
(include/fmx.h "fmx_fwfm_*").

    y(x) = w0 + sum_j w_j x_j + sum_{i<j} r[g(i)][g(j)] <v_i, v_j> x_i x_j

groups[j] is feature j's field, r a symmetric [F][F] matrix.  With the field sums S_g = sum_{i in g} v_i x_i of a row, T = r S and
D_g = sum_{i in g} |v_i|^2 x_i^2:
    pair term = 1/2 sum_g <S_g, T_g> - 1/2 sum_g r_gg D_g
    d/dv_i = x_i (T_g(i) - r_g(i)g(i) v_i x_i)       d/dr_gh = <S_g, S_h> (g != h)       d/dr_gg = 1/2 (|S_g|^2 - D_g)
An id repeated inside a row counts as separate entries of its field.

One epoch is adaptive.epoch's batch rule with these sums: per batch, from the batch-start parameters, (1) S, D, T and rest_e;
(2) the bias in micro-chunks (adaptive.bias_steps); (3) AdaGrad on w and V with g_vf = sum_occ mult_e x (T_e,g(j),f - r_gg v_jf x)
+ nocc regv v_jf on the accumulators of `state`; (4) AdaGrad on r from the batch-start r: g_gh = sum_e mult_e d y_e / d r_gh
+ reg_r r_gh (once per batch), n_r += g^2, r -= eta_r g / sqrt(n_r) on the upper triangle and the diagonal, mirrored."""
import numpy as np

from . import adaptive


def field_sums(model, groups, data, r0, nb, F, dtype=np.float64):
    """(ids, xs, ex, S[nb][F][k], D[nb][F]) of rows [r0, r0 + nb) from the parameters `model` holds now"""
    row_ptr = data.row_ptr.astype(np.int64)
    a, b = row_ptr[r0], row_ptr[r0 + nb]
    ids = data.entries["id"][a:b].astype(np.int64)
    xs = data.entries["value"][a:b].astype(dtype)
    ex = np.repeat(np.arange(nb), np.diff(row_ptr[r0:r0 + nb + 1]))
    d = model.v.astype(dtype)[:, ids].T * xs[:, None]                               # [entries][k]
    S = np.zeros((nb, F, int(model.k)), dtype=dtype)
    D = np.zeros((nb, F), dtype=dtype)
    fld = np.asarray(groups, dtype=np.int64)[ids]
    np.add.at(S, (ex, fld), d)
    np.add.at(D, (ex, fld), (d * d).sum(axis=1, dtype=dtype))
    return ids, xs, ex, fld, S, D


def _rest(model, r, ids, xs, ex, S, D, nb, dtype):
    """y-hat minus the bias, and T = r S"""
    T = np.einsum("gh,ehf->egf", r.astype(dtype), S).astype(dtype)
    rest = (0.5 * (S * T).sum(axis=(1, 2), dtype=dtype) - 0.5 * (D * np.diag(r).astype(dtype)[None, :]).sum(axis=1, dtype=dtype)).astype(dtype)
    if model.k1:
        np.add.at(rest, ex, model.w.astype(dtype)[ids] * xs)
    return rest, T


def predict(model, r, groups, rows):
    """y-hat of every row (no clamp, as fmx_predict)"""
    r = np.asarray(r, dtype=np.float64)
    nb = int(rows.n_rows)
    ids, xs, ex, _, S, D = field_sums(model, groups, rows, 0, nb, r.shape[0])
    rest, _ = _rest(model, r, ids, xs, ex, S, D, nb, np.float64)
    return rest + (model.w0 if model.k0 else 0.0)


def batch_gradients(model, r, groups, mult, ids, xs, ex, fld, S, D, T, dtype=np.float64):
    """the gradient sums of sum_e mult_e y_e over a batch, without regularisation: (feats, nocc, g_w[feats], g_v[feats][k], g_r[F][F]);
    occurrences in row order, g_r with both triangles filled"""
    F, k = r.shape[0], int(model.k)
    feats, inv = np.unique(ids, return_inverse=True)
    nocc = np.bincount(inv, minlength=len(feats)).astype(dtype)
    me_x = mult[ex] * xs
    gw = np.zeros(len(feats), dtype=dtype)
    np.add.at(gw, inv, me_x)
    vj = model.v.astype(dtype)[:, feats].T                                          # [feats][k]
    G = np.zeros((len(feats), k), dtype=dtype)
    A = np.zeros(len(feats), dtype=dtype)
    np.add.at(G, inv, me_x[:, None] * T[ex, fld])
    np.add.at(A, inv, me_x * xs)
    rgg = np.diag(r).astype(dtype)[np.asarray(groups, dtype=np.int64)[feats]]
    gv = G - vj * (A * rgg)[:, None]
    # the field matrix: sum_e mult_e S_e S_e^T, the diagonal with D (fp64 from here on, as the device adds its partials)
    gr = np.einsum("e,egf,ehf->gh", mult, S, S).astype(np.float64)
    gr[np.diag_indices(F)] = 0.5 * (np.diag(gr) - (mult[:, None] * D).sum(axis=0, dtype=np.float64))
    return feats, nocc, gw, gv, gr


def epoch(model, state, r, n_r, groups, rows, task, lr, min_target, max_target, batch, w0_chunk, eta=None, eta_r=None, reg_r=0.0,
          dtype=np.float64):
    """one epoch, in place on model, state (adaptive.AdaptState), r and n_r ([F][F] float64 arrays).  eta None = lr, eta_r None = eta.
    dtype=np.float32 runs the sums, the products and the w / V steps in fp32 (the bias, r and n_r stay doubles, as on the device)."""
    Tp = np.dtype(dtype).type
    eta = Tp(lr if eta is None else eta)
    eta_r = float(eta) if eta_r is None else float(eta_r)
    F, k, n_rows = r.shape[0], int(model.k), int(rows.n_rows)
    batch = n_rows if (batch == 0 or batch > n_rows) else int(batch)
    regw, regv = Tp(model.regw), Tp(model.regv)
    for r0 in range(0, n_rows, batch):
        nb = min(batch, n_rows - r0)
        r_b = r.astype(dtype)                                                       # (the kernels read an fp32 copy of r)
        ids, xs, ex, fld, S, D = field_sums(model, groups, rows, r0, nb, F, dtype)
        rest, T = _rest(model, r_b, ids, xs, ex, S, D, nb, dtype)
        mult = adaptive.bias_steps(model, rest, rows.target[r0:r0 + nb], task, lr, min_target, max_target, batch, w0_chunk, dtype)
        feats, nocc, gw, gv, gr = batch_gradients(model, r_b, groups, mult, ids, xs, ex, fld, S, D, T, dtype)
        w, v = model.w.astype(dtype), model.v.astype(dtype)
        if model.k1:
            wj = w[feats]
            gw = gw + nocc * regw * wj
            nw = (state.n_w[feats].astype(dtype) + gw * gw).astype(dtype)
            state.n_w[feats] = nw
            model.w[feats] = (wj - eta * gw / np.sqrt(nw)).astype(dtype)
        vj = v[:, feats].T                                                          # [feats][k]
        gv = gv + nocc[:, None] * regv * vj
        nv = (state.n_v[:, feats].T.astype(dtype) + gv * gv).astype(dtype)
        state.n_v[:, feats] = nv.T
        model.v[:, feats] = (vj - eta * gv / np.sqrt(nv)).astype(dtype).T
        gr = gr + float(reg_r) * r
        iu = np.triu_indices(F)
        n1 = n_r[iu] + gr[iu] * gr[iu]
        rn = r[iu] - eta_r * gr[iu] / np.sqrt(n1)
        n_r[iu] = n1
        n_r[(iu[1], iu[0])] = n1
        r[iu] = rn
        r[(iu[1], iu[0])] = rn
