"""FTRL-proximal with L1 on the minibatch rule, restated in numpy (the CPU reference of fmx_ftrl_epoch; include/fmx.h "fmx_ftrl_*").

One epoch cuts the rows into batches of `batch` consecutive rows.  Per batch, steps 1 and 2 are AdaGrad's (libfm_amd/adaptive.py):
  1. from the batch-start parameters, per example e: S_ef and rest_e;
  2. the bias advances in micro-chunks of `w0_chunk` examples with plain SGD at `lr` and reg0; mult_e is the loss multiplier taken
     with its micro-chunk's own bias;
  3. for every feature j of the batch, from the batch-start theta (w_j or v_jf) and its occurrences (e, x) in row order:
        g_w  = sum_occ mult_e x                  g_vf = sum_occ mult_e (S_ef x - v_jf x x)      (no regularisation term: L2 is in D)
        n'   = n + g^2        sigma = (sqrt(n') - sqrt(n)) / alpha        z' = z + g - sigma theta
        D'   = (beta + sqrt(n')) / alpha + l2
        theta' = 0 if |z'| <= l1 else -(z' - sgn(z') l1) / D'
The model's regw / regv are not read: l2_w / l2_v are one strength per coordinate, not per occurrence as in the plain rule.
FtrlState derives z from the parameters the model holds when it is made (z0 = -theta0 D0 - sgn(theta0) l1, D0 = (beta +
sqrt(init_acc)) / alpha + l2), so that the closed form returns theta0 and with l1 = 0 every step is theta' = theta - g / D'.
A feature that no batch touches keeps theta, z and n.  dtype=np.float32 runs every sum and the update in fp32 (the bias stays a
double, as on the device)."""
import numpy as np

from .adaptive import _multiplier, row_weights


class FtrlState:
    """z_w[n], z_v[k][n], n_w[n], n_v[k][n] (the layout of the model's w and v) and the rule's constants"""

    def __init__(self, model, alpha, beta=1.0, l1_w=0.0, l1_v=0.0, l2_w=0.0, l2_v=0.0, init_acc=0.0):
        vals = (alpha, beta, l1_w, l1_v, l2_w, l2_v, init_acc)
        if not all(np.isfinite(x) and x >= 0.0 for x in vals):
            raise ValueError("alpha, beta, l1, l2 and init_acc must be finite and >= 0")
        if not alpha > 0.0:
            raise ValueError("alpha must be > 0")
        if beta == 0.0 and init_acc == 0.0:
            raise ValueError("beta = 0 needs init_acc > 0 (D would start at 0)")
        self.alpha, self.beta, self.init_acc = float(alpha), float(beta), float(init_acc)
        self.l1_w, self.l1_v, self.l2_w, self.l2_v = float(l1_w), float(l1_v), float(l2_w), float(l2_v)
        n, k = int(model.n), int(model.k)
        self.n_w = np.full(n, self.init_acc, dtype=np.float64)
        self.n_v = np.full((k, n), self.init_acc, dtype=np.float64)
        base = (self.beta + np.sqrt(self.init_acc)) / self.alpha
        w = np.asarray(model.w, dtype=np.float64)
        v = np.asarray(model.v, dtype=np.float64)
        self.z_w = -w * (base + self.l2_w) - np.sign(w) * self.l1_w
        self.z_v = -v * (base + self.l2_v) - np.sign(v) * self.l1_v


def _step(theta, z, n, g, alpha, beta, l1, l2, dtype):
    """one proximal step of the coordinates given as arrays; returns (theta', z', n')"""
    T = np.dtype(dtype).type
    n1 = (n + g * g).astype(dtype)
    r1 = np.sqrt(n1)
    sigma = ((r1 - np.sqrt(n)) / T(alpha)).astype(dtype)
    z1 = (z + g - sigma * theta).astype(dtype)
    D = ((T(beta) + r1) / T(alpha) + T(l2)).astype(dtype)
    new = np.where(np.abs(z1) <= T(l1), T(0), -(z1 - np.sign(z1) * T(l1)) / D).astype(dtype)
    return new, z1, n1


def epoch(model, data, task, lr, min_target, max_target, batch, w0_chunk, state, dtype=np.float64, weights=None):
    """one epoch over `data` (oracle.Data layout), in place on `model` (oracle.Model layout; regw / regv are not read) and `state`.
    lr is the bias's plain rate.  Returns the largest |change| of a w / v coordinate over the epoch's batches.  weights: as
    adaptive.epoch (one weight per row, float32 first, multiplied into the multiplier)."""
    T = np.dtype(dtype).type
    cw = row_weights(weights, data.n_rows, dtype)
    ids_all = data.entries["id"].astype(np.int64)
    xs_all = data.entries["value"].astype(dtype)
    row_ptr = data.row_ptr.astype(np.int64)
    n_rows = int(data.n_rows)
    k = int(model.k)
    batch = n_rows if (batch == 0 or batch > n_rows) else int(batch)
    st = state
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
        # step 3: one gradient sum and one proximal step per touched feature, occurrences in row order
        feats, inv = np.unique(ids, return_inverse=True)
        me_x = mult[ex] * xs
        if model.k1:
            gw = np.zeros(len(feats), dtype=dtype)
            np.add.at(gw, inv, me_x)
            wj = w[feats]
            new, z1, n1 = _step(wj, st.z_w[feats].astype(dtype), st.n_w[feats].astype(dtype), gw, st.alpha, st.beta, st.l1_w, st.l2_w, dtype)
            st.z_w[feats], st.n_w[feats] = z1, n1
            if len(feats):
                max_step = max(max_step, float(np.abs(new.astype(np.float64) - wj.astype(np.float64)).max()))
            model.w[feats] = new
        if k:
            vj = v[:, feats].T                                                     # [feats][k]
            G = np.zeros((len(feats), k), dtype=dtype)
            A = np.zeros(len(feats), dtype=dtype)
            np.add.at(G, inv, me_x[:, None] * S[ex])
            np.add.at(A, inv, me_x * xs)
            gv = (G - vj * A[:, None]).astype(dtype)
            new, z1, n1 = _step(vj, st.z_v[:, feats].T.astype(dtype), st.n_v[:, feats].T.astype(dtype), gv, st.alpha, st.beta, st.l1_v,
                                st.l2_v, dtype)
            st.z_v[:, feats], st.n_v[:, feats] = z1.T, n1.T
            if len(feats):
                max_step = max(max_step, float(np.abs(new.astype(np.float64) - vj.astype(np.float64)).max()))
            model.v[:, feats] = new.T
    return max_step


def pair_epoch(model, entries, row_ptr, pa, pb, batch, state, step_dtype=np.float64):
    """pairwise ranking (BPR) on the batch rule with the proximal step per coordinate (the CPU reference of fmx_ftrl_pair_epoch): one
    epoch over the pairs (row pa[t] preferred to row pb[t]) in batches of `batch` consecutive pairs, in place on `model` and `state`
    (FtrlState).  Per feature of a batch the gradient sum of adaptive.pair_batch_sums WITHOUT the regularisation terms (float64, pair
    order; regw / regv are not read: L2 lives in D), then _step in step_dtype -- float32 is the device's arithmetic: g32 = float32(g),
    theta, z and n in fp32.  w0 -= reg0 w0 once per pair.  Returns the largest |change| of a w / v coordinate over the epoch's batches."""
    from .adaptive import pair_batch_sums, pair_decay_w0
    if int(batch) < 1:
        raise ValueError("batch must be >= 1")
    T = np.dtype(step_dtype).type
    P, batch, st = len(pa), int(batch), state
    max_step = 0.0
    for t0 in range(0, P, batch):
        t1 = min(t0 + batch, P)
        feats, gw, gv = pair_batch_sums(model, entries, row_ptr, pa, pb, t0, t1, reg=False)
        if len(feats):
            if model.k1:
                old = model.w[feats]
                new, z1, n1 = _step(old.astype(T), st.z_w[feats].astype(T), st.n_w[feats].astype(T), gw.astype(T), st.alpha, st.beta,
                                    st.l1_w, st.l2_w, T)
                st.z_w[feats], st.n_w[feats] = z1, n1
                max_step = max(max_step, float(np.abs(new.astype(np.float64) - old).max()))
                model.w[feats] = new
            if model.v.shape[0]:
                old = model.v[:, feats].T
                new, z1, n1 = _step(old.astype(T), st.z_v[:, feats].T.astype(T), st.n_v[:, feats].T.astype(T), gv.astype(T), st.alpha,
                                    st.beta, st.l1_v, st.l2_v, T)
                st.z_v[:, feats], st.n_v[:, feats] = z1.T, n1.T
                max_step = max(max_step, float(np.abs(new.astype(np.float64) - old).max()))
                model.v[:, feats] = new.T
        pair_decay_w0(model, t1 - t0)
    return max_step
