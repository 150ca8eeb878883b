"""The field-matrixed FM (FmFM, Sun et al., WWW 2021) restated in numpy: the CPU reference of fmx_fmfm_predict / fmx_fmfm_epoch
(include/fmx.h "fmx_fmfm_*").

    y(x) = w0 + sum_j w_j x_j + sum_{a<b} x_a x_b  v_ja^T M[g(ja)][g(jb)] v_jb

groups[j] is feature j's field; M is [F][F][k][k] with M[h][g] = M[g][h]^T and identity diagonal blocks (not learned).  With the field
sums S_g = sum_{i in g} v_i x_i of a row, T_h = sum_g M[g][h]^T S_g (t = MM s over the concatenated sums) and D = sum_i |v_i x_i|^2:
    pair term = 1/2 sum_g <S_g, T_g> - 1/2 D
    d/dv_i = x_i (T_g(i) - v_i x_i)       d/dM[g][h] = S_g S_h^T  (g < h)
An id repeated inside a row counts as separate entries of its field.

One epoch is adaptive.epoch's batch rule with these sums: per batch, from the batch-start parameters, (1) S, D, T and rest_e;
(2) the bias in micro-chunks (adaptive.bias_steps); (3) AdaGrad on w and V with g_vf = sum_occ mult_e x (T_e,g(j),f - v_jf x)
+ nocc regv v_jf on the accumulators of `state`; (4) AdaGrad on the blocks g < h of M from the batch-start M: g = sum_e mult_e S_e,g
S_e,h^T + reg_m M[g][h] (once per batch), n_M += g^2, M -= eta_m g / sqrt(n_M), the lower blocks written as the transposes."""
import numpy as np

from . import adaptive
from .fwfm import field_sums


def identity(F, k):
    """M of the plain FM: every block the identity"""
    return np.tile(np.eye(k), (F, F, 1, 1))


def random_m(F, k, rng, scale=0.6):
    """a valid M: the upper blocks drawn from N(0, scale^2), the lower blocks mirrored, the diagonal blocks the identity"""
    M = identity(F, k)
    for g in range(F):
        for h in range(g + 1, F):
            M[g, h] = rng.normal(0.0, scale, size=(k, k))
            M[h, g] = M[g, h].T
    return M


def _rest(model, M, ids, xs, ex, S, D, dtype):
    """y-hat minus the bias, and T"""
    nb, F, k = S.shape                                                              # T[e][h][b] = sum_g,a S[e][g][a] M[g][h][a][b]: t = s MM
    T = (S.reshape(nb, F * k) @ M.astype(dtype).transpose(0, 2, 1, 3).reshape(F * k, F * k)).reshape(nb, F, k).astype(dtype)
    rest = (0.5 * (S * T).sum(axis=(1, 2), dtype=dtype) - 0.5 * D.sum(axis=1, dtype=dtype)).astype(dtype)
    if model.k1:
        np.add.at(rest, ex, model.w.astype(dtype)[ids] * xs)
    return rest, T


def predict(model, M, groups, rows, dtype=np.float64):
    """y-hat of every row (no clamp, as fmx_predict)"""
    M = np.asarray(M, dtype=np.float64)
    ids, xs, ex, _, S, D = field_sums(model, groups, rows, 0, int(rows.n_rows), M.shape[0], dtype)
    rest, _ = _rest(model, M, ids, xs, ex, S, D, dtype)
    return rest + (model.w0 if model.k0 else 0.0)


def batch_gradients(model, groups, mult, ids, xs, ex, fld, S, T, dtype=np.float64):
    """the gradient sums of sum_e mult_e y_e over a batch, without regularisation: (feats, nocc, g_w[feats], g_v[feats][k],
    g_M[F][F][k][k]); occurrences in row order, g_M filled for every g != h (the diagonal blocks are not parameters: zeros)"""
    F = S.shape[1]
    feats, inv = np.unique(ids, return_inverse=True)
    nocc = np.bincount(inv, minlength=len(feats)).astype(dtype)
    me_x = mult[ex] * xs
    gw = np.zeros(len(feats), dtype=dtype)
    np.add.at(gw, inv, me_x)
    G = np.zeros((len(feats), int(model.k)), dtype=dtype)
    A = np.zeros(len(feats), dtype=dtype)
    np.add.at(G, inv, me_x[:, None] * T[ex, fld])
    np.add.at(A, inv, me_x * xs)
    gv = G - model.v.astype(dtype)[:, feats].T * A[:, None]
    s = S.reshape(len(S), -1)                                                       # G = s^T diag(mult) s, cut into blocks
    gm = ((s * mult[:, None]).T @ s).reshape(F, S.shape[2], F, S.shape[2]).transpose(0, 2, 1, 3).astype(np.float64)   # (fp64 from here on)
    gm[np.arange(F), np.arange(F)] = 0.0
    return feats, nocc, gw, gv, gm


def epoch(model, state, M, n_M, groups, rows, task, lr, min_target, max_target, batch, w0_chunk, eta=None, eta_m=None, reg_m=0.0,
          dtype=np.float64):
    """one epoch, in place on model, state (adaptive.AdaptState), M and n_M ([F][F][k][k] float64 arrays).  eta None = lr, eta_m None =
    eta.  dtype=np.float32 runs the sums, the products and the w / V steps in fp32 (the bias, M and n_M stay doubles, as on the device)."""
    Tp = np.dtype(dtype).type
    eta = Tp(lr if eta is None else eta)
    eta_m = float(eta) if eta_m is None else float(eta_m)
    F, n_rows = M.shape[0], int(rows.n_rows)
    batch = n_rows if (batch == 0 or batch > n_rows) else int(batch)
    regw, regv = Tp(model.regw), Tp(model.regv)
    up = np.triu(np.ones((F, F), dtype=bool), 1)
    for r0 in range(0, n_rows, batch):
        nb = min(batch, n_rows - r0)
        ids, xs, ex, fld, S, D = field_sums(model, groups, rows, r0, nb, F, dtype)
        rest, T = _rest(model, M, ids, xs, ex, S, D, dtype)                          # (the kernels read an fp32 copy of M)
        mult = adaptive.bias_steps(model, rest, rows.target[r0:r0 + nb], task, lr, min_target, max_target, batch, w0_chunk, dtype)
        feats, nocc, gw, gv, gm = batch_gradients(model, groups, mult, ids, xs, ex, fld, S, T, dtype)
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
        g = gm[up] + float(reg_m) * M[up]                                           # [pairs g < h][k][k]
        n1 = n_M[up] + g * g
        mn = M[up] - eta_m * g / np.sqrt(n1)
        n_M[up], M[up] = n1, mn
        n_M[up.T] = np.swapaxes(n_M, 0, 1).swapaxes(2, 3)[up.T]                     # M[h][g] = M[g][h]^T
        M[up.T] = np.swapaxes(M, 0, 1).swapaxes(2, 3)[up.T]
