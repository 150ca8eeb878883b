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


def row_weights(weights, n_rows, dtype):
    """the per-row weights of a weighted epoch in the working dtype (None: unweighted): float32 first, as the device stores them"""
    if weights is None:
        return None
    c = np.asarray(weights, dtype=np.float64).reshape(-1)
    if c.shape[0] != int(n_rows):
        raise ValueError("weights: %d values for %d rows" % (c.shape[0], int(n_rows)))
    c = c.astype(np.float32)
    if not (np.isfinite(c).all() and (c >= 0).all()):
        raise ValueError("weights must be finite and >= 0")
    return c.astype(dtype)


def _multiplier(task, p, y, min_target, max_target):
    """fm_learn_sgd_element.h:58-65"""
    if task == TASK_REGRESSION:
        return -(y - np.maximum(min_target, np.minimum(max_target, p)))
    return -y * (1.0 - 1.0 / (1.0 + np.exp(-y * p)))


def epoch(model, data, task, lr, min_target, max_target, batch, w0_chunk, state, eta=None, rule="adagrad", dtype=np.float64,
          weights=None):
    """one epoch over `data` (oracle.Data layout: entries {id, value}, row_ptr, target), in place on `model` (oracle.Model layout:
    w0, w[n], v[k][n], k0, k1, reg0, regw, regv) and `state`.  eta None = lr.  Returns the largest |change| of a w / v coordinate
    over the epoch's batches.  weights: None, or one finite weight >= 0 per row (fmx_set_row_weights): rounded to float32, then
    multiplied into the multiplier in the working dtype -- it scales the loss only, nocc and the bias's reg0 term keep counting rows."""
    if rule not in ("adagrad", "sgd"):
        raise ValueError("unknown rule %r (adagrad | sgd)" % (rule,))
    T = np.dtype(dtype).type
    eta = T(lr if eta is None else eta)
    cw = row_weights(weights, data.n_rows, dtype)
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
            if cw is not None:
                me = (me * cw[r0 + c0:r0 + c1]).astype(dtype)
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


# ---- pairwise ranking (BPR) on the batch rule, stepped per coordinate (the CPU reference of fmx_adapt_pair_epoch) ----------------
# One epoch cuts the pairs (row pa[t] preferred to row pb[t]) into batches of `batch` consecutive pairs.  Per batch, from the
# batch-start parameters: per pair d = y_a - y_b (fm_model::predict on both rows), mult = -(1 - sigmoid(d)) and the gradients of
# fm_pairSGD for every DISTINCT feature of the pair (fm_sgd.h:53-126); per feature j of the batch
#     g = sum over the pairs t of the batch that contain j of (mult_t grad_tj [+ reg theta_j])       (float64, pair order)
# -- the sum the plain batch rule multiplies by its learning rate, one regularisation term per distinct pair -- and then one step of
# the rule per coordinate.  w0 -= reg0 w0 once per pair.  batch = 1 is the per-pair rule.

def _pair_row(entries, row_ptr, r):
    a, b = int(row_ptr[r]), int(row_ptr[r + 1])
    e = entries[a:b]
    return e["id"].astype(np.int64), e["value"].astype(np.float32).astype(np.float64)


def _pair_predict(model, ids, xs):
    """fm_model::predict (fm_model.h:105-127) in its order, without the bias (it cancels in y_a - y_b): (y, sum[k])"""
    y = 0.0
    if model.k1 and len(ids):
        y = float(np.cumsum(model.w[ids] * xs)[-1])
    k = model.v.shape[0]
    if k == 0:
        return y, np.zeros(0)
    if len(ids) == 0:
        return y, np.zeros(k)
    d = model.v[:, ids] * xs                                                        # [k][entries]
    s = np.cumsum(d, axis=1)[:, -1]
    q = np.cumsum(d * d, axis=1)[:, -1]
    return float(np.cumsum(np.concatenate([[y], 0.5 * (s * s - q)]))[-1]), s


def pair_batch_sums(model, entries, row_ptr, pa, pb, t0, t1, reg=True):
    """the gradient sums of the pairs [t0, t1) from the parameters `model` holds now: (feats int64 [m] in first-touch order,
    g_w float64 [m], g_v float64 [m][k]); reg=False leaves the regularisation terms out"""
    k = model.v.shape[0]
    index, gw, gv = {}, [], []
    for t in range(t0, t1):
        ia, xa = _pair_row(entries, row_ptr, int(pa[t]))
        ib, xb = _pair_row(entries, row_ptr, int(pb[t]))
        ya, sa = _pair_predict(model, ia, xa)
        yb, sb = _pair_predict(model, ib, xb)
        mult = -(1.0 - 1.0 / (1.0 + np.exp(-(ya - yb))))                            # util.h:52
        pw, pv, order = {}, {}, []
        for ids, xs, s, sign in ((ia, xa, sa, 1.0), (ib, xb, sb, -1.0)):
            for j, x in zip(ids, xs):
                j = int(j)
                if j not in pw:
                    order.append(j)
                    pw[j] = 0.0
                    pv[j] = np.zeros(k)
                pw[j] += sign * x                                                   # fm_sgd.h:67-72
                pv[j] += sign * (s * x - model.v[:, j] * x * x)                     # :100-105
        for j in order:
            if j not in index:
                index[j] = len(gw)
                gw.append(0.0)
                gv.append(np.zeros(k))
            i = index[j]
            gw[i] += mult * pw[j] + (model.regw * model.w[j] if reg else 0.0)
            gv[i] += mult * pv[j] + (model.regv * model.v[:, j] if reg else 0.0)
    feats = np.fromiter(index.keys(), dtype=np.int64, count=len(index))
    return feats, np.array(gw, dtype=np.float64), (np.array(gv, dtype=np.float64).reshape(len(gw), k))


def pair_decay_w0(model, n_pairs):
    """fm_sgd.h:56 once per pair, without a learning rate"""
    if model.k0:
        for _ in range(n_pairs):
            model.w0 -= model.reg0 * model.w0


def pair_epoch(model, entries, row_ptr, pa, pb, eta, batch, state, rule="adagrad", step_dtype=np.float64):
    """one epoch over the pairs, in place on `model` and `state` (AdaptState).  rule "adagrad": n += g^2, theta -= eta g / sqrt(n);
    "sgd": theta -= eta g, the plain batch rule (the state is not touched).  The sums are float64; the step runs in step_dtype --
    float32 is the device's arithmetic: g32 = float32(g), theta and n in fp32.  Returns the largest |change| of a w / v coordinate
    over the epoch's batches."""
    if rule not in ("adagrad", "sgd"):
        raise ValueError("unknown rule %r (adagrad | sgd)" % (rule,))
    if int(batch) < 1:
        raise ValueError("batch must be >= 1")
    T = np.dtype(step_dtype).type
    P, batch = len(pa), int(batch)
    max_step = 0.0

    def step(theta, n, g):
        if rule == "sgd":
            return theta - eta * g, n
        g, n, theta = g.astype(T), n.astype(T), theta.astype(T)
        n1 = (n + g * g).astype(T)
        return (theta - T(eta) * g / np.sqrt(n1)).astype(T), n1

    for t0 in range(0, P, batch):
        t1 = min(t0 + batch, P)
        feats, gw, gv = pair_batch_sums(model, entries, row_ptr, pa, pb, t0, t1, reg=True)
        if len(feats):
            if model.k1:
                old = model.w[feats]
                new, state.n_w[feats] = step(old, state.n_w[feats], gw)
                max_step = max(max_step, float(np.abs(new.astype(np.float64) - old).max()))
                model.w[feats] = new
            if model.v.shape[0]:
                old = model.v[:, feats].T
                new, n1 = step(old, state.n_v[:, feats].T, gv)
                state.n_v[:, feats] = n1.T
                max_step = max(max_step, float(np.abs(new.astype(np.float64) - old).max()))
                model.v[:, feats] = new.T
        pair_decay_w0(model, t1 - t0)
    return max_step
