"""fp64 numpy restatement of the pairwise ranking learner (include/fmx.h, "pairwise ranking"): the loop around the reference's
fm_pairSGD (fm_sgd.h:53-126) and the batch rule of FMX_SGD_MINIBATCH, in the reference's summation order.

Model: an object with w0, w[n], v[k][n] (float64) and k0, k1, reg0, regw, regv -- oracle.Model fits.  Rows: (entries, row_ptr) as
oracle.Data keeps them (entries: structured id / value, values float32 like DATA_FLOAT).  Pairs: two arrays of row indices, row
a[t] preferred to row b[t].
"""
import numpy as np


def _row(data_entries, row_ptr, r):
    a, b = int(row_ptr[r]), int(row_ptr[r + 1])
    e = data_entries[a:b]
    return e["id"].astype(np.int64), e["value"].astype(np.float32).astype(np.float64)


def predict_row(m, ids, xs):
    """fm_model::predict (fm_model.h:105-127) in its order; returns (y, sum[k])"""
    lin = [m.w0] if m.k0 else [0.0]
    if m.k1 and len(ids):
        lin += list(m.w[ids] * xs)
    y = np.cumsum(lin)[-1]                                   # cumsum is sequential: the reference's += order
    k = m.v.shape[0]
    if k == 0:
        return float(y), np.zeros(0)
    if len(ids):
        d = m.v[:, ids] * xs                                 # [k][entries]
        s = np.cumsum(d, axis=1)[:, -1]
        q = np.cumsum(d * d, axis=1)[:, -1]
    else:
        s = np.zeros(k)
        q = np.zeros(k)
    y = np.cumsum(np.concatenate([[y], 0.5 * (s * s - q)]))[-1]
    return float(y), s


def sigmoid(d):
    return 1.0 / (1.0 + np.exp(-d))                          # util.h:52


def pair_gradients(m, ids_a, xs_a, ids_b, xs_b, s_a, s_b):
    """the per-pair gradients of fm_pairSGD for every DISTINCT feature of the pair, in first-occurrence order (x_a then x_b):
    {j: (gw_j, gv_j[k])}, from the parameters as they are now"""
    order = []
    gw, gv = {}, {}
    k = m.v.shape[0]
    for j in list(ids_a) + list(ids_b):
        j = int(j)
        if j not in gw:
            order.append(j)
            gw[j] = 0.0
            gv[j] = np.zeros(k)
    for j, x in zip(ids_a, xs_a):
        gw[int(j)] += x                                       # fm_sgd.h:67-69
    for j, x in zip(ids_b, xs_b):
        gw[int(j)] -= x                                       # :70-72
    for j, x in zip(ids_a, xs_a):
        gv[int(j)] += s_a * x - m.v[:, int(j)] * x * x        # :100-102
    for j, x in zip(ids_b, xs_b):
        gv[int(j)] -= s_b * x - m.v[:, int(j)] * x * x        # :103-105
    return order, gw, gv


def pair_sgd(m, lr, ids_a, xs_a, ids_b, xs_b, mult, s_a, s_b):
    """fm_pairSGD (fm_sgd.h:53-126): w0 decays without learning rate; every distinct feature once, one regularisation term"""
    if m.k0:
        m.w0 -= m.reg0 * m.w0
    order, gw, gv = pair_gradients(m, ids_a, xs_a, ids_b, xs_b, s_a, s_b)   # (all from the start of the pair)
    if m.k1:
        for j in order:
            m.w[j] -= lr * (mult * gw[j] + m.regw * m.w[j])
    for j in order:
        m.v[:, j] -= lr * (mult * gv[j] + m.regv * m.v[:, j])


def pair_epoch_loop(m, entries, row_ptr, pa, pb, lr):
    """one epoch of the learner: the pairs in stored order, each through predict, the BPR multiplier and fm_pairSGD"""
    for a, b in zip(pa, pb):
        ia, xa = _row(entries, row_ptr, int(a))
        ib, xb = _row(entries, row_ptr, int(b))
        ya, sa = predict_row(m, ia, xa)
        yb, sb = predict_row(m, ib, xb)
        mult = -(1.0 - sigmoid(ya - yb))
        pair_sgd(m, lr, ia, xa, ib, xb, mult, sa, sb)


def pair_epoch_batch(m, entries, row_ptr, pa, pb, lr, B):
    """one epoch of the batch rule (FMX_SGD_MINIBATCH): every pair of a batch takes its sums and multiplier from the parameters at
    the start of the batch; each touched feature is updated once with the gradient terms summed in pair order, one
    regularisation term per pair; w0 -= reg0 * w0 once per pair.  B = 1 is the loop."""
    P = len(pa)
    for t0 in range(0, P, B):
        w_start, v_start = m.w.copy(), m.v.copy()
        acc_w, acc_v, order = {}, {}, []
        for t in range(t0, min(t0 + B, P)):
            ia, xa = _row(entries, row_ptr, int(pa[t]))
            ib, xb = _row(entries, row_ptr, int(pb[t]))
            ya, sa = predict_row(m, ia, xa)                  # (m holds the batch-start parameters until the batch ends)
            yb, sb = predict_row(m, ib, xb)
            mult = -(1.0 - sigmoid(ya - yb))
            feats, gw, gv = pair_gradients(m, ia, xa, ib, xb, sa, sb)
            for j in feats:
                if j not in acc_w:
                    order.append(j)
                    acc_w[j] = 0.0
                    acc_v[j] = np.zeros(m.v.shape[0])
                acc_w[j] += mult * gw[j] + m.regw * w_start[j]
                acc_v[j] += mult * gv[j] + m.regv * v_start[:, j]
        for j in order:
            if m.k1:
                m.w[j] = w_start[j] - lr * acc_w[j]
            m.v[:, j] = v_start[:, j] - lr * acc_v[j]
        if m.k0:
            for _ in range(t0, min(t0 + B, P)):
                m.w0 -= m.reg0 * m.w0


def pair_d(m, entries, row_ptr, pa, pb):
    """y_a - y_b per pair (fp64)"""
    out = np.zeros(len(pa))
    for t, (a, b) in enumerate(zip(pa, pb)):
        ia, xa = _row(entries, row_ptr, int(a))
        ib, xb = _row(entries, row_ptr, int(b))
        out[t] = predict_row(m, ia, xa)[0] - predict_row(m, ib, xb)[0]
    return out


def pair_metrics(d):
    """(accuracy = fraction with d > 0, loss = mean of -ln sigmoid(d))"""
    d = np.asarray(d, dtype=np.float64)
    if len(d) == 0:
        return 0.0, 0.0
    loss = np.where(d >= 0, np.log1p(np.exp(-np.abs(d))), -d + np.log1p(np.exp(-np.abs(d))))
    return float(np.mean(d > 0)), float(np.mean(loss))


def predict_rows(m, entries, row_ptr):
    n_rows = len(row_ptr) - 1
    return np.array([predict_row(m, *_row(entries, row_ptr, r))[0] for r in range(n_rows)])
