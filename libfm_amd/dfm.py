"""DeepFM with one hidden layer (Guo et al., IJCAI 2017) restated in numpy: the CPU reference of fmx_dfm_predict / fmx_dfm_epoch
(include/fmx.h "fmx_dfm_*").

    s    = (S[0], ..., S[F-1])              S[g] = sum_{b: g(j_b) = g} x_b v_jb                    (k floats per field)
    a    = relu(W1^T s + b1)                W1: [F k][H], b1: [H]
    y(x) = w0 + sum_j w_j x_j + 1/2 (|sum_g S[g]|^2 - D) + <w2, a>                                 w2: [H];  D = sum_b |x_b v_jb|^2

groups[j] is feature j's field; the net is the tuple (W1, b1, w2).  The ReLU mask is `pre-activation > 0`, so an all-zero net is the
plain FM and never receives a gradient.  An id repeated inside a row counts as separate entries of its field.  With dh = [a > 0] w2,
z = W1 dh and Stot = sum_g S[g]:
    d/dv_j = x (Stot + z_g(j) - v_j x)        d/dW1 = s dh^T        d/db1 = dh        d/dw2 = a

One epoch is adaptive.epoch's batch rule with these sums: per batch, from the batch-start parameters, (1) S, D, a and rest_e;
(2) the bias in micro-chunks (adaptive.bias_steps); (3) AdaGrad on w and V with g_vc = sum_occ mult_e x (Stot_e,c + z_e,g(j),c - v_jc x)
+ nocc regv v_jc on the accumulators of `state`; (4) AdaGrad on W1, b1 and w2 from the batch-start net: g = sum_e mult_e d y_e / d theta
+ reg_net theta (once per batch), n += g^2, theta -= eta_net g / sqrt(n)."""
import numpy as np

from . import adaptive
from .fwfm import field_sums


def zero_net(F, k, H):
    """the net of the plain FM"""
    return np.zeros((F * k, H)), np.zeros(H), np.zeros(H)


def random_net(F, k, H, rng, stdev=0.3, b1_away=0.45):
    """a start net: W1 and w2 from N(0, stdev^2), and b1 from the same moved b1_away further from zero: units are on for most rows or off
    for most rows, and few rows come near a unit's kink"""
    b1 = rng.normal(0.0, stdev, size=H)
    return rng.normal(0.0, stdev, size=(F * k, H)), b1 + np.where(b1 < 0, -b1_away, b1_away), rng.normal(0.0, stdev, size=H)


def forward(model, net, ids, xs, ex, S, D, dtype):
    """(y-hat minus the bias, the pre-activations [nb][H], a [nb][H], Stot [nb][k])"""
    W1, b1, w2 = (np.asarray(t).astype(dtype) for t in net)
    nb = S.shape[0]
    pre = (S.reshape(nb, -1) @ W1 + b1).astype(dtype)
    a = np.where(pre > 0, pre, 0).astype(dtype)
    Stot = S.sum(axis=1, dtype=dtype)
    rest = (0.5 * (Stot * Stot).sum(axis=1, dtype=dtype) - 0.5 * D.sum(axis=1, dtype=dtype) + a @ w2).astype(dtype)
    if model.k1:
        np.add.at(rest, ex, model.w.astype(dtype)[ids] * xs)
    return rest, pre, a, Stot


def predict(model, net, groups, rows, dtype=np.float64):
    """y-hat of every row (no clamp, as fmx_predict)"""
    F = np.asarray(net[0]).shape[0] // int(model.k)
    ids, xs, ex, _, S, D = field_sums(model, groups, rows, 0, int(rows.n_rows), F, dtype)
    return forward(model, net, ids, xs, ex, S, D, dtype)[0] + (model.w0 if model.k0 else 0.0)


def batch_gradients(model, net, mult, ids, xs, ex, fld, S, pre, a, Stot, dtype=np.float64):
    """the gradient sums of sum_e mult_e y_e over a batch, without regularisation: (feats, nocc, g_w[feats], g_v[feats][k], g_W1, g_b1,
    g_w2); occurrences in row order"""
    W1, w2 = np.asarray(net[0]).astype(dtype), np.asarray(net[2]).astype(dtype)
    nb, F, k = S.shape
    dh = np.where(pre > 0, w2, 0).astype(dtype)                                     # [nb][H]
    R = (Stot[:, None, :] + (dh @ W1.T).reshape(nb, F, k)).astype(dtype)            # the sum row of field g: Stot + z_g
    feats, inv = np.unique(ids, return_inverse=True)
    nocc = np.bincount(inv, minlength=len(feats)).astype(dtype)
    me_x = mult[ex] * xs
    gw = np.zeros(len(feats), dtype=dtype)
    np.add.at(gw, inv, me_x)
    G = np.zeros((len(feats), k), dtype=dtype)
    A = np.zeros(len(feats), dtype=dtype)
    np.add.at(G, inv, me_x[:, None] * R[ex, fld])
    np.add.at(A, inv, me_x * xs)
    gv = G - model.v.astype(dtype)[:, feats].T * A[:, None]
    ms = S.reshape(nb, -1) * mult[:, None]
    return feats, nocc, gw, gv, (ms.T @ dh).astype(np.float64), (mult @ dh).astype(np.float64), (mult @ a).astype(np.float64)


def epoch(model, state, net, n_net, groups, rows, task, lr, min_target, max_target, batch, w0_chunk, eta=None, eta_net=None, reg_net=0.0,
          dtype=np.float64):
    """one epoch, in place on model, state (adaptive.AdaptState), net = (W1, b1, w2) and n_net, their accumulators (float64 arrays).
    eta None = lr, eta_net None = eta.  dtype=np.float32 runs the sums, the products and the w / V steps in fp32 (the bias, the net and
    its accumulators stay doubles, as on the device).  Returns the smallest |pre-activation| the epoch met (inf without rows)."""
    Tp = np.dtype(dtype).type
    eta = Tp(lr if eta is None else eta)
    eta_net = float(eta) if eta_net is None else float(eta_net)
    F, n_rows = net[0].shape[0] // int(model.k), int(rows.n_rows)
    batch = n_rows if (batch == 0 or batch > n_rows) else int(batch)
    regw, regv = Tp(model.regw), Tp(model.regv)
    closest = np.inf
    for r0 in range(0, n_rows, batch):
        nb = min(batch, n_rows - r0)
        ids, xs, ex, fld, S, D = field_sums(model, groups, rows, r0, nb, F, dtype)
        rest, pre, a, Stot = forward(model, net, ids, xs, ex, S, D, dtype)           # (the kernels read an fp32 copy of the net)
        closest = min(closest, float(np.abs(pre).min()))
        mult = adaptive.bias_steps(model, rest, rows.target[r0:r0 + nb], task, lr, min_target, max_target, batch, w0_chunk, dtype)
        feats, nocc, gw, gv, *gnet = batch_gradients(model, net, mult, ids, xs, ex, fld, S, pre, a, Stot, dtype)
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
        for theta, n, g in zip(net, n_net, gnet):                                   # (fp64, in place)
            g = g + float(reg_net) * theta
            n += g * g
            theta -= eta_net * g / np.sqrt(n)
    return closest
