"""AdaGrad on the minibatch rule, restated in numpy (the CPU reference of fmx_adapt_epoch; include/fmx.h "fmx_adapt_*").

One epoch cuts the rows into batches of `batch` consecutive rows.  Per batch:
  1. from the batch-start parameters, per example e: S_ef = sum_i v_f[id_i] x_i and rest_e = lin_e + 0.5 sum_f (S_ef^2 - Q_ef);
  2. the bias advances in micro-chunks of `w0_chunk` examples with plain SGD at `lr` and reg0; mult_e is the loss multiplier taken
     with its micro-chunk's own bias (steps 1 and 2 are the oracle's fmo_sgd_epoch_minibatch with bias_lag = 0);
  3. for every feature j of the batch, from the batch-start w_j, v_jf, its occurrences (e, x) in row order, nocc their number:
        g_w  = sum_occ mult_e x                       + nocc regw w_j
        g_vf = sum_occ mult_e (S_ef x - v_jf x x)     + nocc regv v_jf
        n += g^2;  theta -= eta g / sqrt(n)           (rule "adagrad"; "sgd": theta -= lr g, the plain batch rule)
An id repeated inside a row counts as separate occurrences.  A feature that no batch touches keeps its parameters and accumulators.
dtype=np.float32 runs every sum and the update in fp32 (the bias stays a double, as on the device)."""
import numpy as np

TASK_REGRESSION, TASK_CLASSIFICATION = 0, 1


class AdaptState:
    """the accumulators: n_w[n], n_v[k][n] (the layout of the model's w and v), every one init_acc at the start"""

    def __init__(self, n, k, init_acc=1.0):
        if not (init_acc > 0.0 and np.isfinite(init_acc)):
            raise ValueError("init_acc must be finite and > 0")
        self.init_acc = float(init_acc)
        self.n_w = np.full(int(n), self.init_acc, dtype=np.float64)
        self.n_v = np.full((int(k), int(n)), self.init_acc, dtype=np.float64)


def _multiplier(task, p, y, min_target, max_target):
    """fm_learn_sgd_element.h:58-65"""
    if task == TASK_REGRESSION:
        return -(y - np.maximum(min_target, np.minimum(max_target, p)))
    return -y * (1.0 - 1.0 / (1.0 + np.exp(-y * p)))


def epoch(model, data, task, lr, min_target, max_target, batch, w0_chunk, state, eta=None, rule="adagrad", dtype=np.float64):
    """one epoch over `data` (oracle.Data layout: entries {id, value}, row_ptr, target), in place on `model` (oracle.Model layout:
    w0, w[n], v[k][n], k0, k1, reg0, regw, regv) and `state`.  eta None = lr.  Returns the largest |change| of a w / v coordinate
    over the epoch's batches."""
    if rule not in ("adagrad", "sgd"):
        raise ValueError("unknown rule %r (adagrad | sgd)" % (rule,))
    T = np.dtype(dtype).type
    eta = T(lr if eta is None else eta)
    ids_all = data.entries["id"].astype(np.int64)
    xs_all = data.entries["value"].astype(dtype)
    row_ptr = data.row_ptr.astype(np.int64)
    n_rows = int(data.n_rows)
    k = int(model.k)
    batch = n_rows if (batch == 0 or batch > n_rows) else int(batch)
    regw, regv = T(model.regw), T(model.regv)
    max_step = 0.0
    for r0 in range(0, n_rows, batch):
        nb = min(batch, n_rows - r0)
        a, b = row_ptr[r0], row_ptr[r0 + nb]
        ids, xs = ids_all[a:b], xs_all[a:b]
        ex = np.repeat(np.arange(nb), np.diff(row_ptr[r0:r0 + nb + 1]))          # example of every entry, row order
        # step 1: sums from the batch-start parameters
        w = model.w.astype(dtype)
        v = model.v.astype(dtype)                                                  # [k][n]
        rest = np.zeros(nb, dtype=dtype)
        if model.k1:
            np.add.at(rest, ex, w[ids] * xs)
        S = np.zeros((nb, k), dtype=dtype)
        if k:
            d = v[:, ids].T * xs[:, None]                                          # [entries][k]
            Q = np.zeros((nb, k), dtype=dtype)
            np.add.at(S, ex, d)
            np.add.at(Q, ex, d * d)
            rest += (T(0.5) * (S * S - Q)).sum(axis=1, dtype=dtype)
        # step 2: the bias in micro-chunks, plain SGD
        y = data.target[r0:r0 + nb].astype(dtype)
        mult = np.zeros(nb, dtype=dtype)
        chunk = nb if (w0_chunk == 0 or w0_chunk > batch) else int(w0_chunk)
        for c0 in range(0, nb, chunk):
            c1 = min(nb, c0 + chunk)
            w0s = T(model.w0) if model.k0 else T(0)
            me = _multiplier(task, w0s + rest[c0:c1], y[c0:c1], T(min_target), T(max_target)).astype(dtype)
            mult[c0:c1] = me
            if model.k0:
                model.w0 -= float(lr) * (float(me.sum(dtype=np.float64)) + (c1 - c0) * float(model.reg0) * float(w0s))
        # step 3: one gradient sum per touched feature, occurrences in row order
        feats, inv = np.unique(ids, return_inverse=True)
        nocc = np.bincount(inv, minlength=len(feats)).astype(dtype)
        me_x = mult[ex] * xs
        if model.k1:
            gw = np.zeros(len(feats), dtype=dtype)
            np.add.at(gw, inv, me_x)
            wj = w[feats]
            gw = gw + nocc * regw * wj
            if rule == "adagrad":
                nw = (state.n_w[feats].astype(dtype) + gw * gw).astype(dtype)
                state.n_w[feats] = nw
                new = (wj - eta * gw / np.sqrt(nw)).astype(dtype)
            else:
                new = (wj - T(lr) * gw).astype(dtype)
            if len(feats):
                max_step = max(max_step, float(np.abs(new.astype(np.float64) - wj.astype(np.float64)).max()))
            model.w[feats] = new
        if k:
            vj = v[:, feats].T                                                     # [feats][k]
            G = np.zeros((len(feats), k), dtype=dtype)
            A = np.zeros(len(feats), dtype=dtype)
            np.add.at(G, inv, me_x[:, None] * S[ex])
            np.add.at(A, inv, me_x * xs)
            gv = G - vj * A[:, None] + nocc[:, None] * regv * vj
            if rule == "adagrad":
                nv = (state.n_v[:, feats].T.astype(dtype) + gv * gv).astype(dtype)
                state.n_v[:, feats] = nv.T
                new = (vj - eta * gv / np.sqrt(nv)).astype(dtype)
            else:
                new = (vj - T(lr) * gv).astype(dtype)
            if len(feats):
                max_step = max(max_step, float(np.abs(new.astype(np.float64) - vj.astype(np.float64)).max()))
            model.v[:, feats] = new.T
    return max_step
