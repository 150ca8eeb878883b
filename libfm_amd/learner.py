"""Host-side mirror of the reference's learner interface on top of the C-ABI (include/fmx.h).

The names, fields, argument meaning and error behaviour follow the reference so that the parity tests read like
the reference's own driver (there are no reference tests to imitate):

    FMModel      <-> class fm_model            /root/reference/src/fm_core/fm_model.h:36-66
    Data         <-> class Data                /root/reference/src/libfm/src/Data.h:49-73   (rows + target only)
    FMLearnSGD   <-> fm_learn_sgd_element      /root/reference/src/libfm/src/fm_learn_sgd_element.h:34-78
                     (+ fm_learn_sgd.h:34-90, fm_learn.h:31-153)

All arithmetic happens in libfmx.so on the GPU; this file only moves buffers and applies the host-side
clamp / sigmoid of fm_learn_sgd::predict (fm_learn_sgd.h:80-87).  No CPU fallback exists.
"""
import sys

import numpy as np

from . import capi, compact as compact_format, evalmetrics

TASK_REGRESSION = capi.TASK_REGRESSION        # fm_learn.h:46
TASK_CLASSIFICATION = capi.TASK_CLASSIFICATION  # fm_learn.h:47


class Data:
    """Rows in the reference's layout: AoS entries {u32 id; f32 value} + row offsets + float targets."""

    def __init__(self, entries, row_ptr, target):
        self.entries = np.ascontiguousarray(entries, dtype=capi.ENTRY_DTYPE)
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        self.target = np.ascontiguousarray(target, dtype=np.float32)
        self.num_cases = len(self.target)                       # Data.h:60
        self.num_feature = int(self.entries["id"].max()) + 1 if len(self.entries) else 0   # Data.h:59
        self.min_target = float(self.target.min()) if self.num_cases else 0.0   # Data.h:62-63
        self.max_target = float(self.target.max()) if self.num_cases else 0.0
        self.relation = []                                       # Data.h:68: DVector<RelationJoin>
        self.keep_blocks = True        # relations: keep main rows and blocks apart on the device (per-block caches, like the
        #                                reference) instead of materialising the joined rows (FMX_BLOCKS_KEEP / _EXPAND)

    def add_relation(self, rel, data_row_to_relation_row, attr_offset):
        """RelationJoin (relation.h:53-60): `rel` = a data.Relation (the block's own rows), the main-row -> block-row
        mapping of THIS data set (<prefix>.train / <prefix>.test) and the block's first global attribute id
        (RelationData::attr_offset, libfm.cpp:213-216)."""
        m = np.ascontiguousarray(data_row_to_relation_row, dtype=np.uint32)
        if len(m) != self.num_cases:
            raise ValueError("relation mapping has %d rows, the data set %d" % (len(m), self.num_cases))   # relation.h:149
        self.relation.append((rel.entries, rel.row_ptr, m, int(attr_offset)))

    def upload(self, h, slot):
        if self.relation:
            h.upload_block_rows(slot, self.entries, self.row_ptr, self.target, self.relation, keep=self.keep_blocks)
        else:
            h.upload_rows(slot, self.entries, self.row_ptr, self.target)


class FMModel:
    """fm_model: parameters in the reference layout (w0, w[n], v[k][n] fp64) and its hyper-parameters."""

    def __init__(self):
        self.num_attribute = 0
        self.num_factor = 0
        self.k0, self.k1 = True, True
        self.reg0 = self.regw = self.regv = 0.0
        self.init_stdev, self.init_mean = 0.01, 0.0             # fm_model.h:69-78
        self.w0 = 0.0
        self.w = None
        self.v = None

    def init(self, rng=None):
        """fm_model::init (fm_model.h:91-99): w0 = 0, w = 0, v ~ N(init_mean, init_stdev).
        The reference draws from libc rand(); here a numpy Generator is used (pass the reference's own
        initial parameters for trajectory parity, as the tests do)."""
        rng = rng if rng is not None else np.random.default_rng(0)
        self.w0 = 0.0
        self.w = np.zeros(self.num_attribute, dtype=np.float64)
        if self.init_stdev == 0:
            self.v = np.full((self.num_factor, self.num_attribute), self.init_mean, dtype=np.float64)
        else:
            self.v = self.init_mean + self.init_stdev * rng.standard_normal((self.num_factor, self.num_attribute))


    # fm_model::saveModel (fm_model.h:132-154): text, ostream default precision (= printf %g)
    def save_model(self, path):
        with open(path, "w") as f:
            if self.k0:
                f.write("#global bias W0\n%g\n" % self.w0)
            if self.k1:
                f.write("#unary interactions Wj\n")
                f.write("".join("%g\n" % x for x in self.w))
            f.write("#pairwise interactions Vj,f\n")
            for j in range(self.num_attribute):
                f.write(" ".join("%g" % x for x in self.v[:, j]) + "\n")

    # fm_model::loadModel (fm_model.h:160-190); returns False on a malformed file like the reference returns 0.
    # (The reference's splitString yields no token for a line without a blank, so k = 1 models fail to load there,
    #  fm_model.h:195-205; this reader accepts them.)
    def load_model(self, path):
        try:
            lines = open(path).read().splitlines()
            pos = 0
            if self.k0:
                self.w0 = float(lines[pos + 1]); pos += 2
            if self.k1:
                pos += 1
                self.w = np.array([float(x) for x in lines[pos:pos + self.num_attribute]], dtype=np.float64)
                pos += self.num_attribute
            pos += 1
            rows = [[float(x) for x in ln.split(" ") if x != ""] for ln in lines[pos:pos + self.num_attribute]]
            if len(rows) != self.num_attribute or any(len(r) != self.num_factor for r in rows):
                return False
            self.v = np.ascontiguousarray(np.array(rows, dtype=np.float64).reshape(self.num_attribute, self.num_factor).T)
            return True                                          # (-dim 1,1,0: n empty lines, as fm_model.h:160-190 reads them)
        except (OSError, ValueError, IndexError):
            return False


EXTRA_METRICS = ("auc", "logloss")
WEIGHTED_METRIC = "wlogloss"                                    # extra_metrics of a learner with set_weights: fmx_evaluate_weighted's log loss
RANK_MAX_CUTOFFS, RANK_MAX_K = capi.RANK_MAX_CUTOFFS, capi.RANK_MAX_K   # of rank_cutoffs (fmx_evaluate_rank)


def _log_extra_metrics(learner, i, train, test):
    """learner.extra_metrics on a classification task: one stderr line per named metric (where the BPR learner puts its loss
    lines) and <metric>_train / <metric>_test in the iteration's log row.  stdout is not touched."""
    names = tuple(learner.extra_metrics)
    weights = getattr(learner, "_weights", None)                # (only FMLearnSGD and its subclasses carry row weights)
    for m in names:
        if m not in EXTRA_METRICS and not (m == WEIGHTED_METRIC and weights is not None):
            raise ValueError("unknown metric %r (want auc, logloss%s)" % (m, ", wlogloss" if weights is not None else ""))
    if not names or learner.task != TASK_CLASSIFICATION:
        return
    tr, te = learner.evaluate_ex(train), learner.evaluate_ex(test)
    for m in names:
        if m == WEIGHTED_METRIC:                                 # the weighted log loss of the sets that carry weights (set_weights); nan for the others
            a, b = (learner.evaluate_weighted(d).logloss if id(d) in weights else float("nan") for d in (train, test))
        else:
            a, b = getattr(tr, m), getattr(te, m)
        print("#Iter=%3d\t%s: Train=%g\tTest=%g" % (i, m, a, b), file=sys.stderr)
        learner.log[-1][m + "_train"], learner.log[-1][m + "_test"] = a, b


def _log_query_metrics(learner, i, train, test):
    """when a data set of learn() has query ids (set_queries) on a classification task: one more stderr line with the
    impression-weighted per-query AUC (fmx_evaluate_by_query) and gauc_* / auc_within_* in the iteration's log row; a set without
    ids gives nan.  With rank_cutoffs the same scoring pass and sort also give the tie-averaged NDCG, recall and precision at every
    cutoff (fmx_evaluate_rank, whose by_query is fmx_evaluate_by_query's result): one more stderr line per cutoff and ndcg@K_* /
    recall@K_* / precision@K_* in the log row.  stdout is not touched."""
    if learner.task != TASK_CLASSIFICATION or not any(id(d) in learner._queries for d in (train, test)):
        return
    nan = float("nan")
    cutoffs = tuple(learner.rank_cutoffs)
    row, evs = learner.log[-1], {}
    for name, d in (("train", train), ("test", test)):
        ev = rk = None
        if id(d) in learner._queries:
            rk = learner.evaluate_rank(d, cutoffs) if cutoffs else None
            ev = rk.by_query if cutoffs else learner.evaluate_by_query(d)
        evs[name] = rk
        row["gauc_" + name], row["auc_within_" + name] = (ev.gauc, ev.auc_within) if ev is not None else (nan, nan)
    print("#Iter=%3d\tgauc: Train=%g\tTest=%g" % (i, row["gauc_train"], row["gauc_test"]), file=sys.stderr)
    for j, k in enumerate(cutoffs):
        for name, rk in evs.items():
            for m in ("ndcg", "recall", "precision"):
                row["%s@%d_%s" % (m, k, name)] = getattr(rk.at[j], m) if rk is not None else nan
        print("#Iter=%3d\tndcg@%d: Train=%g\tTest=%g" % (i, k, row["ndcg@%d_train" % k], row["ndcg@%d_test" % k]), file=sys.stderr)


def _check_weights(data, weights):
    w = np.asarray(weights, dtype=np.float64).reshape(-1).astype(np.float32)
    if len(w) != data.num_cases:
        raise ValueError("set_weights: %d weights for %d rows" % (len(w), data.num_cases))
    if not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError("set_weights: every weight must be finite and >= 0")
    return w


def _check_queries(data, qid):
    q = np.asarray(qid).reshape(-1)
    if len(q) != data.num_cases:
        raise ValueError("set_queries: %d query ids for %d rows" % (len(q), data.num_cases))
    return q


class CompactView:
    """A frozen bf16 or int8 copy of a learner's model on the device (fmx_compact_*), scored like the learner itself: predict, evaluate,
    evaluate_ex and recommend mirror the learner's methods, link and clamping included, and read the copy, so training the
    learner further does not change what they return.  `info` is the capi.CompactInfo of the copy (bytes, max_abs_err,
    nonfinite).  A handle holds one copy: learner.compact() again replaces it under every earlier view; close() frees it.
    prune ("dead" | "seen"): the copy keeps only the rows that can score (fmx_compact_begin_pruned) -- "dead" drops the features that
    contribute to no prediction, "seen" also those the training rows never name; `prune_info` is its capi.CompactPruneInfo (kept,
    dropped_dead, dropped_unseen, bytes), None for a dense copy."""

    PRUNE = (None, "dead", "seen")

    def __init__(self, learner, format, prune=None):
        if format not in compact_format.FORMATS:
            raise ValueError("unknown serving format %r (%s)" % (format, " | ".join(compact_format.FORMATS)))
        if prune not in self.PRUNE:
            raise ValueError("unknown prune rule %r (None | dead | seen)" % (prune,))
        self._l = learner
        self.format = format
        self.prune = prune
        self.prune_info = None
        if prune is None:
            self.info = learner._h.compact_begin(compact_format.FORMATS[format])
        else:
            self.info, self.prune_info = learner._h.compact_begin_pruned(compact_format.FORMATS[format],
                                                                         learner._compact_train_slot() if prune == "seen" else None)

    def predict_raw(self, data):
        return self._l._h.compact_predict(self._l._compact_slot(data), data.num_cases)

    def predict(self, data):
        return self._l._link(self.predict_raw(data))

    def evaluate(self, data):
        ev = self._l._h.compact_evaluate(self._l._compact_slot(data))
        return ev.rmse if self._l.task == TASK_REGRESSION else ev.accuracy

    def evaluate_ex(self, data):
        return self._l._h.compact_evaluate_ex(self._l._compact_slot(data), self._l.EVAL_LINK)

    def recommend(self, queries, candidates, topk, exclude=None):
        qs, cs = self._l._topk_slots(queries, candidates)
        return self._l._h.compact_topk(qs, cs, topk, 0, queries.num_cases, exclude)

    topk = recommend

    def rows(self, ids):
        """(w[ids], v[:, ids]) as the copy holds them, dequantised; zeros for a feature a pruned copy dropped (fmx_compact_get_rows)"""
        return self._l._h.compact_rows(ids)

    def save(self, path):
        """the copy as a snapshot file, written straight from its device tables (fmx_compact_save): load_snapshot(path) serves from it
        in a process that never holds the model.  Returns the capi.SnapInfo of the file."""
        return self._l._h.compact_save(path)

    def close(self):
        if self._l is not None and self._l._h is not None:
            if getattr(self._l, "owns_handle", False):           # load_snapshot: the view is all there is -- the handle goes with it
                self._l._h.close()
                self._l._h = None
            else:
                self._l._h.compact_end()
        self._l = None


class _SnapshotSource:
    """what a CompactView asks of its learner, over a serve-only handle (load_snapshot): the handle, a slot per data set, and the link
    of fm_learn_sgd::predict under the file's task and target range"""
    EVAL_LINK = capi.LINK_LOGISTIC
    owns_handle = True

    def __init__(self, h):
        self._h = h
        self._slots = {}
        self.task, self.min_target, self.max_target = int(h.snap_info.task), float(h.snap_info.min_target), float(h.snap_info.max_target)

    def _compact_slot(self, data):
        key = id(data)
        if key not in self._slots:
            if len(self._slots) >= capi.MAX_SLOTS:
                raise RuntimeError("too many data sets")
            data.upload(self._h, len(self._slots))
            self._slots[key] = len(self._slots)
        return self._slots[key]

    def _topk_slots(self, queries, candidates):
        return self._compact_slot(queries), self._compact_slot(candidates)

    def _link(self, p):
        if self.task == TASK_REGRESSION:
            return np.maximum(self.min_target, np.minimum(self.max_target, p))
        return 1.0 / (1.0 + np.exp(-p))


def load_snapshot(path, device=-1):
    """a CompactView over a SERVE-ONLY handle made from a snapshot file alone (fmx_serve_open): no model is created or loaded, the
    device holds the snapshot and nothing else.  predict / evaluate / evaluate_ex / recommend (topk) / rows / save work as on a view of a
    learner; predict links as fm_learn_sgd::predict does under the file's task and target range.  close() destroys the handle.
    `info` is the file's capi.SnapInfo."""
    h = capi.serve_open(path, device)
    view = CompactView.__new__(CompactView)
    view._l = _SnapshotSource(h)
    view.info = h.snap_info
    view.format = compact_format.FORMAT_NAMES[int(view.info.format)]
    view.prune = None if not view.info.pruned else ("seen" if view.info.dropped_unseen else "dead")
    view.prune_info = None
    return view


class FMLearnSGD:
    """fm_learn_sgd_element on the GPU.

    Public knobs are plain fields set by the driver, like libfm.cpp:271-309, 387-403 does by direct writes:
    fm, min_target, max_target, task, num_iter, learn_rate.  GPU-only knobs: mode ('sequential' | 'minibatch' |
    'hogwild'), batch, w0_chunk, apply ('default' | 'segmented' | 'atomic' | 'store'), device; optimizer ('sgd': the reference's one
    learn_rate for every coordinate | 'adagrad': a per-coordinate step on the minibatch rule, fmx_adapt_*, with init_acc the start
    value of the accumulators (0 = 1.0) and adapt_learn_rate the eta of w and V (0 = learn_rate; the bias keeps learn_rate) |
    'ftrl': FTRL-proximal with L1 on the minibatch rule, fmx_ftrl_*, which sets coordinates to exactly zero: ftrl_alpha (0 =
    learn_rate; the bias keeps learn_rate), ftrl_beta, l1_w / l1_v, l2_w / l2_v (None = fm.regw / fm.regv).  Under 'ftrl' an l2 is ONE
    strength per coordinate inside the proximal step, not one per occurrence as regw / regv are in the plain rule, and init_acc is the
    start value of n as it is given (0 stays 0).  sparsity() counts the zeros of the model under any optimizer.
    `devices` (None: one handle on `device`) lists device ordinals as on FMLearnALS: with more than one entry the model is split into
    one feature shard per entry (hashed ownership; "[0, 0]" = two shards on one device) and optimizer 'adagrad' / 'ftrl' train over
    the shards (capi.Group, fmx_group_adapt_* / fmx_group_ftrl_*): learn, predict, evaluate, evaluate_ex, extra_metrics, set_queries
    and sparsity() run through the group.  Optimizer 'sgd' has no sharded form here, nor have compact(), recommend(), checkpoints and
    row weights: each raises NotImplementedError before any device is touched.  Checkpoints of a sharded model exist one layer down:
    capi.Group.checkpoint_save / checkpoint_load (fmx_group_checkpoint_*) write and read the unsharded handle's file in global
    feature order, so the route from shards to this learner is the file itself -- load_checkpoint of an unsharded FMLearnSGD
    continues from a file a group wrote."""

    OPTIMIZERS = ("sgd", "adagrad", "ftrl")
    SHARDED_OPTIMIZERS = ("adagrad", "ftrl")                    # what `devices` with more than one entry is honoured for
    MODES = {"sequential": capi.SGD_SEQUENTIAL, "minibatch": capi.SGD_MINIBATCH, "hogwild": capi.SGD_HOGWILD}
    APPLY = {"default": capi.APPLY_DEFAULT, "atomic": capi.APPLY_ATOMIC, "store": capi.APPLY_STORE,
             "segmented": capi.APPLY_SEGMENTED, "fused": capi.APPLY_FUSED}

    def __init__(self):
        self.fm = None
        self.min_target = 0.0
        self.max_target = 0.0
        self.task = TASK_REGRESSION
        self.num_iter = 100                                     # libfm.cpp:274 default
        self.learn_rate = None                                  # no default in the reference (libfm.cpp:391-392)
        self.mode = "minibatch"
        self.batch = 0                                          # 0: the library's choice (262144 cut to the rows' stability bound)
        self.w0_chunk = 0
        self.apply = "fused"                                    # the batch rule in one pass (hogwild: "default")
        self.bias_lag = 2
        self.reject_unstable = True                             # an explicit batch the rule diverges at raises instead of training
        self.optimizer = "sgd"
        self.init_acc = 0.0
        self.adapt_learn_rate = 0.0
        self.ftrl_alpha = 0.0
        self.ftrl_beta = 1.0
        self.l1_w, self.l1_v = 0.0, 0.0
        self.l2_w, self.l2_v = None, None
        self.device = -1
        self.devices = None                                     # device ordinals of the feature shards (more than one: a capi.Group)
        self.log = []                                           # one dict per iteration (rlog fields)
        self.extra_metrics = ()                                 # classification: "auc" and / or "logloss" per iteration, on stderr and in log
        self.out = sys.stdout
        self._h = None                                          # a capi.Handle, or the capi.Group of the shards
        self._shards = []
        self._slots = {}
        self._queries = {}                                      # id(data) -> (qid, n_queries) of set_queries
        self._weights = {}                                      # id(data) -> float32 weights of set_weights
        self.rank_cutoffs = ()                                  # with query ids: ndcg / recall / precision at these K per iteration
        self._adapt_open = False
        self._ftrl_open = False
        self._checkpoint = None                                 # load_checkpoint before init(): the file init() starts from

    def _check_optimizer(self):
        if self.optimizer not in self.OPTIMIZERS:
            raise ValueError("unknown optimizer for %s: %s (%s)" % (type(self).__name__, self.optimizer, " | ".join(self.OPTIMIZERS)))
        if self.optimizer == "adagrad" and self.mode != "minibatch":
            raise ValueError("optimizer adagrad runs on the minibatch rule: mode %s is not supported" % self.mode)
        if self.optimizer == "ftrl" and self.mode != "minibatch":
            raise ValueError("optimizer ftrl runs on the minibatch rule: mode %s is not supported" % self.mode)

    def _sharded(self):
        """`devices` asks for feature shards (more than one entry); decided from the field alone, so that it holds before init()"""
        return self.devices is not None and len(self.devices) > 1

    def _not_on_shards(self, what):
        if self._sharded():
            raise NotImplementedError("%s is not supported on feature shards (devices lists %d GPUs)" % (what, len(self.devices)))

    def _check_devices(self):
        if not self._sharded():
            return
        if type(self) is not FMLearnSGD:
            raise NotImplementedError("%s has no form on feature shards (devices lists %d GPUs): FMLearnSGD with optimizer %s has"
                                      % (type(self).__name__, len(self.devices), " | ".join(self.SHARDED_OPTIMIZERS)))
        if self.optimizer not in self.SHARDED_OPTIMIZERS:
            raise NotImplementedError("optimizer %s is not supported on feature shards (devices lists %d GPUs): use %s"
                                      % (self.optimizer, len(self.devices), " | ".join(self.SHARDED_OPTIMIZERS)))
        if self._checkpoint is not None:
            self._not_on_shards("load_checkpoint")
        if self._weights:
            self._not_on_shards("set_weights")

    # fm_learn::init (fm_learn.h:73-91): here it creates the device context and uploads the parameters
    def init(self):
        if self.task not in (TASK_REGRESSION, TASK_CLASSIFICATION):
            raise ValueError("unknown task")                    # fm_learn.h:81
        if self.learn_rate is None:
            raise ValueError("learn_rate must be set")          # the reference asserts (libfm.cpp:391-392)
        self._check_optimizer()
        self._check_devices()
        fm = self.fm
        if self._sharded():
            devs = [int(d) for d in self.devices]
            self._shards = [capi.Handle(fm.num_attribute, fm.num_factor, fm.k0, fm.k1, self.task, fm.reg0, fm.regw, fm.regv,
                                        self.learn_rate, self.min_target, self.max_target, device=d, shard_rank=r,
                                        shard_world=len(devs), shard_hash=1) for r, d in enumerate(devs)]
            self._h = capi.Group(self._shards)
            self._h.set_params(fm.w0, fm.w, fm.v)
            self._begin_session()
            return
        if self.devices is not None and len(self.devices) == 1:
            self.device = int(self.devices[0])
        self._h = capi.Handle(fm.num_attribute, fm.num_factor, fm.k0, fm.k1, self.task, fm.reg0, fm.regw, fm.regv,
                              self.learn_rate, self.min_target, self.max_target, device=self.device)
        if self._checkpoint is not None:                        # the file's parameters and session, not fm's and a fresh one
            self._load_checkpoint_now(self._checkpoint)
        else:
            self._h.set_params(fm.w0, fm.w, fm.v)
        self._begin_session()

    def _begin_session(self):
        """open the optimizer's session unless it is open already (a checkpoint brought it)"""
        fm = self.fm
        if self.optimizer == "adagrad" and not self._adapt_open:
            self._h.adapt_begin("adagrad", self.init_acc, self.adapt_learn_rate)
            self._adapt_open = True
        if self.optimizer == "ftrl" and not self._ftrl_open:
            self._h.ftrl_begin(self.ftrl_alpha, self.ftrl_beta, self.l1_w, self.l1_v, fm.regw if self.l2_w is None else self.l2_w,
                               fm.regv if self.l2_v is None else self.l2_v, self.init_acc)
            self._ftrl_open = True

    def save_checkpoint(self, path, dense=False):
        """the exact binary checkpoint of the model on the device and of the open adagrad / ftrl session (fmx_checkpoint_save;
        libfm_amd/checkpoint.py reads the file).  dense: every feature's state rows, not only those that differ from the start
        state.  Returns capi.CkptInfo."""
        self._not_on_shards("save_checkpoint")
        if self._h is None:
            raise ValueError("save_checkpoint before init()")
        return self._h.checkpoint_save(path, dense=dense)

    def load_checkpoint(self, path):
        """continue from a file of save_checkpoint: the parameters are the file's bit for bit, and if it holds a session the
        learner's optimizer and its constants become the file's (an optimizer other than 'sgd' set by the caller that is not the
        file's raises ValueError; a file without a session leaves the optimizer alone, and a fresh session starts from the loaded
        parameters).  Before init() the file is only looked at and init() loads it in place of fm's parameters; after init() it
        is loaded at once.  Neither init() nor learn() begins the session again."""
        self._not_on_shards("load_checkpoint")
        from . import checkpoint
        with open(path, "rb") as f:
            head = checkpoint.read_header(f.read(checkpoint.HEADER_BYTES))
        kind = checkpoint.SESSION_NAMES[head["session"]]
        if kind != "none" and self.optimizer not in ("sgd", kind):
            raise ValueError("load_checkpoint: optimizer is %s but the file's session is %s" % (self.optimizer, kind))
        if kind != "none" and kind not in self.OPTIMIZERS:
            raise ValueError("load_checkpoint: the file's session is %s but %s knows %s" % (kind, type(self).__name__, " | ".join(self.OPTIMIZERS)))
        if self._h is None:
            self._checkpoint = path
            if kind != "none":
                self.optimizer = kind
            return None
        return self._load_checkpoint_now(path)

    def _load_checkpoint_now(self, path):
        from . import checkpoint
        info = self._h.checkpoint_load(path)
        self._checkpoint = None
        if info.session != checkpoint.SESSION_NONE:
            with open(path, "rb") as f:
                c = checkpoint.consts_dict(checkpoint.read_header(f.read(checkpoint.HEADER_BYTES)))
            self.optimizer = checkpoint.SESSION_NAMES[info.session]
            self._adapt_open, self._ftrl_open = self.optimizer == "adagrad", self.optimizer == "ftrl"
            self.init_acc = c["init_acc"]
            if self._adapt_open:
                self.adapt_learn_rate = c["eta"]
            else:                                               # (alpha is informational: the session keeps the fp32 reciprocal it was saved with)
                self.ftrl_alpha, self.ftrl_beta = 1.0 / c["inv_alpha"], c["beta"]
                self.l1_w, self.l1_v, self.l2_w, self.l2_v = c["l1_w"], c["l1_v"], c["l2_w"], c["l2_v"]
        else:
            self._begin_session()
        self.sync_model()
        return info

    def sparsity(self):
        """how many coordinates of the model on the device are exactly zero (capi.Sparsity, fmx_param_sparsity)"""
        return self._h.param_sparsity()

    def _slot(self, data):
        key = id(data)
        if key not in self._slots:
            slot = len(self._slots)
            if slot >= capi.MAX_SLOTS:
                raise RuntimeError("too many data sets")
            data.upload(self._h, slot)
            self._slots[key] = slot
            if key in self._queries:
                self._h.set_row_queries(slot, *self._queries[key])
            if key in self._weights:
                self._h.set_row_weights(slot, self._weights[key])
        return self._slots[key]

    def set_queries(self, data, qid, n_queries=None):
        """one query id (user, session) per row of `data`: learn() then reports the per-query AUC of the set, and
        evaluate_by_query(data) works (fmx_set_row_queries).  n_queries None = max id + 1."""
        self._queries[id(data)] = (_check_queries(data, qid), n_queries)
        if id(data) in self._slots:
            self._h.set_row_queries(self._slots[id(data)], *self._queries[id(data)])

    def set_weights(self, data, weights):
        """one weight >= 0 per row of `data` (fmx_set_row_weights; None drops them): as the train set, optimizer 'adagrad' / 'ftrl'
        scale every row's loss by its weight (the other trainers have no weighted form and learn() refuses); on any set,
        evaluate_weighted(data) and extra_metrics 'wlogloss' report the weighted log loss.  The weights are stored and attached
        when the set is uploaded, like set_queries' ids."""
        if weights is not None:
            self._not_on_shards("set_weights")
        if weights is None:
            self._weights.pop(id(data), None)
        else:
            self._weights[id(data)] = _check_weights(data, weights)
        if id(data) in self._slots:
            self._h.set_row_weights(self._slots[id(data)], self._weights.get(id(data)))

    def evaluate_weighted(self, data):
        """weighted log loss / accuracy (classification) or RMSE / MAE (regression) of `data` under the current parameters
        (capi.EvalWeighted), reduced on the device (fmx_evaluate_weighted)"""
        if id(data) not in self._weights:
            raise ValueError("evaluate_weighted: the data set has no weights (set_weights)")
        return self._h.evaluate_weighted(self._slot(data), self.EVAL_LINK)

    def evaluate_by_query(self, data):
        """exact AUC inside every query of `data` under the current parameters: gauc, auc_macro, auc_within, the counts and the
        pooled metrics (capi.EvalQuery), reduced on the device (fmx_evaluate_by_query)"""
        if id(data) not in self._queries:
            raise ValueError("evaluate_by_query: the data set has no query ids (set_queries)")
        return self._h.evaluate_by_query(self._slot(data), self.EVAL_LINK)

    def evaluate_rank(self, data, cutoffs):
        """exact tie-averaged NDCG, recall and precision at the cutoffs (at most four, ascending) inside every query of `data` under
        the current parameters (capi.EvalRank: at[j].ndcg / .recall / .precision / .hits / .tied_queries, by_query), reduced on the
        device (fmx_evaluate_rank)"""
        if id(data) not in self._queries:
            raise ValueError("evaluate_rank: the data set has no query ids (set_queries)")
        return self._h.evaluate_rank(self._slot(data), cutoffs, self.EVAL_LINK)

    # fm_learn_sgd_element::learn (fm_learn_sgd_element.h:48-78)
    def learn(self, train, test):
        self._check_optimizer()
        self._check_devices()
        if (self.optimizer == "adagrad") != self._adapt_open or (self.optimizer == "ftrl") != self._ftrl_open:
            raise ValueError("optimizer was changed after init()")
        if id(train) in self._weights and self.optimizer == "sgd":
            raise ValueError("the train set has weights (set_weights): optimizer sgd has no weighted form, use adagrad or ftrl")
        print("learnrate=%g" % self.learn_rate, file=self.out)   # fm_learn_sgd.h:57-59
        print("#iterations=%d" % self.num_iter, file=self.out)
        print("SGD: DON'T FORGET TO SHUFFLE THE ROWS IN TRAINING DATA TO GET THE BEST RESULTS.", file=self.out)
        st = self._slot(train)
        self._train = train                                          # (compact(prune="seen") asks which features these rows name)
        for i in range(self.num_iter):
            apply_ = self.APPLY[self.apply]
            if self.mode != "minibatch" and apply_ == capi.APPLY_FUSED:
                apply_ = capi.APPLY_DEFAULT
            flags = capi.FLAG_REJECT_UNSTABLE if (self.reject_unstable and self.mode == "minibatch") else 0
            flags |= capi.FLAG_KEEP_WSIDE                # the train set is evaluated after every epoch (fm_learn_sgd_element.h:69-70)
            if self._adapt_open:
                stats = self._h.adapt_epoch(st, self.batch, self.w0_chunk)
            elif self._ftrl_open:
                stats = self._h.ftrl_epoch(st, self.batch, self.w0_chunk)
            else:
                stats = self._h.sgd_epoch(st, self.MODES[self.mode], apply_, self.batch, self.w0_chunk, flags,
                                          self.bias_lag if apply_ == capi.APPLY_FUSED else 0)
            if i == 0 and self.mode == "minibatch" and (stats.status & capi.STAT_BATCH_CUT):
                print("libfmx: batch %d (collision mass of the rows %.4g, gain %.3g)" % (stats.batch_used, stats.collision_mass,
                                                                                        stats.batch_gain), file=sys.stderr)
            rmse_train = self.evaluate(train)
            rmse_test = self.evaluate(test)
            print("#Iter=%3d\tTrain=%g\tTest=%g" % (i, rmse_train, rmse_test), file=self.out)   # :71
            self.log.append({"rmse_train": rmse_train, "time_learn": stats.device_seconds})
            _log_extra_metrics(self, i, train, test)
            _log_query_metrics(self, i, train, test)
        self.sync_model()

    def sync_model(self):
        """after learn() the host fm_model holds the learned parameters (main reads it, libfm.cpp:431-434)."""
        self.fm.w0, self.fm.w, self.fm.v = self._h.get_params(self.fm.w, self.fm.v)

    # fm_learn::evaluate (fm_learn.h:93-153): rmse for regression, accuracy for classification
    def evaluate(self, data):
        ev = self._h.evaluate(self._slot(data))
        return ev.rmse if self.task == TASK_REGRESSION else ev.accuracy

    EVAL_LINK = capi.LINK_LOGISTIC       # fm_learn_sgd::predict maps a classification score through the sigmoid (fm_learn_sgd.h:80-87)

    def evaluate_ex(self, data):
        """exact AUC, log loss and the counts behind them under the current parameters, reduced on the device (fmx_evaluate_ex)"""
        return self._h.evaluate_ex(self._slot(data), self.EVAL_LINK)

    def predict_raw(self, data):
        """fm_learn::predict_case over the data set (fm_learn.h:63-65)."""
        return self._h.predict(self._slot(data), data.num_cases)

    def recommend(self, queries, candidates, topk, exclude=None):
        """the topk best candidate rows for every query row under the current parameters (fmx_topk): score(q, c) is the raw
        prediction of the joined row queries[q] ++ candidates[c], without ever writing it out.  Returns (idx uint32
        [queries, topk], score float64 [queries, topk]), padded with (capi.TOPK_NONE, -inf).  exclude: per query, the candidate
        rows it must not get back (a list of iterables, or a CSR (ptr, idx))."""
        self._not_on_shards("recommend: top-K retrieval")
        return self._h.topk(*self._topk_slots(queries, candidates), topk, 0, queries.num_cases, exclude)

    def _topk_slots(self, queries, candidates):
        return self._slot(queries), self._slot(candidates)

    _compact_slot = _slot

    def _compact_train_slot(self):
        """the slot whose entries say which features training has seen (compact(prune="seen"))"""
        if getattr(self, "_train", None) is None:
            raise ValueError("compact(prune='seen'): no single training set (learn() has not run, or learn_implicit() trained on "
                             "query x candidate slots): use prune='dead'")
        return self._compact_slot(self._train)

    def compact(self, format="bf16", prune=None):
        """a CompactView: a frozen reduced-precision copy of the model as it stands, to score from (fmx_compact_begin); with
        prune = "dead" | "seen" one that keeps only the rows that can score (fmx_compact_begin_pruned).  Not on feature shards."""
        self._not_on_shards("compact: the serving snapshot")
        return CompactView(self, format, prune)

    # fm_learn_sgd::predict (fm_learn_sgd.h:76-90)
    def predict(self, data):
        return self._link(self.predict_raw(data))

    def _link(self, p):
        if self.task == TASK_REGRESSION:
            p = np.minimum(self.max_target, p)
            p = np.maximum(self.min_target, p)
        elif self.task == TASK_CLASSIFICATION:
            p = 1.0 / (1.0 + np.exp(-p))
        else:
            raise ValueError("task not supported")              # fm_learn_sgd.h:85
        return p

    def close(self):
        if self._h is not None:
            if self._adapt_open:
                self._h.adapt_end()
                self._adapt_open = False
            if self._ftrl_open:
                self._h.ftrl_end()
                self._ftrl_open = False
            self._h.close()
            self._h = None
        for s in self._shards:
            s.close()
        self._shards = []


cdf_gaussian = evalmetrics.ref_cdf_gaussian       # random.h:65-67 with the reference's erf polynomial (:45-59)


class FMLearnALS:
    """fm_learn_mcmc_simultaneous with do_sample = 0, do_multilevel = 0 -- what `-method als` runs
    (libfm.cpp:135-139, 283-290) -- on the GPU.  Fields follow fm_learn_mcmc (fm_learn_mcmc.h:60-88):
    fm, min_target, max_target, task, num_iter; w_lambda / v_lambda are set from -regular like libfm.cpp:326-365.
    `groups` (attribute -> group id, the `-meta` file; fm_learn.h:40, Data.h:39-46) makes them per group:
    w_lambda [G], v_lambda [G] or [G][k] (libfm.cpp:353-363).
    `device_average` = True keeps the test predictions and their running sums on the device (fmx_post_begin / fmx_post_accumulate):
    the `#Iter=` line then carries the reference's Test(ll) column on classification, the log rows its rmse_mcmc_* / acc_mcmc_* /
    ll_mcmc_* fields, and extra_metrics / evaluate_ex(test) score the averaged prediction.
    `devices` (None: one handle on `device`) lists device ordinals; with more than one entry the model is split into one feature
    shard per entry (hashed ownership, like the libFM adapter's gpu_devices; "[0, 0]" = two shards on one device) and the sweeps
    run over the shards (capi.Group) -- block-structured data keeps its blocks apart there too (Data.keep_blocks)."""

    def __init__(self):
        self.fm = None
        self.min_target = self.max_target = 0.0
        self.task = TASK_REGRESSION
        self.num_iter = 100
        self.w_lambda = 0.0
        self.v_lambda = 0.0
        self.do_sample = False
        self.seed = 0
        self.device = -1
        self.devices = None            # device ordinals of the feature shards (more than one: a capi.Group)
        self.groups = None             # DataMetaInfo::attr_group (None = one group)
        self.out = sys.stdout
        self.pred_this = None          # fm_learn_mcmc.h:116
        self.pred_sum_all = None       # fm_learn_mcmc.h:114
        self.log = []
        self.extra_metrics = ()        # classification: "auc" and / or "logloss" per iteration, on stderr and in log
        self.device_average = False    # keep pred_this / pred_sum_all on the device (fmx_post_*) instead of predicting to the host
        self._h = None                 # a capi.Handle, or the capi.Group of the shards
        self._shards = []
        self._train = self._test = None   # the data sets of learn(): slots 0 and 1
        self._queries = {}             # id(data) -> (qid, n_queries) of set_queries
        self.rank_cutoffs = ()         # with query ids: ndcg / recall / precision at these K per iteration

    def init(self):
        fm = self.fm
        devs = [] if self.devices is None else [int(d) for d in self.devices]
        if len(devs) > 1:
            self._shards = [capi.Handle(fm.num_attribute, fm.num_factor, fm.k0, fm.k1, self.task, fm.reg0, fm.regw, fm.regv,
                                        0.0, self.min_target, self.max_target, device=d, shard_rank=r, shard_world=len(devs),
                                        shard_hash=1) for r, d in enumerate(devs)]
            for s in self._shards:
                s.set_groups(self.groups)
            self._h = capi.Group(self._shards)
            self._h.set_params(fm.w0, fm.w, fm.v)
            return
        self._h = capi.Handle(fm.num_attribute, fm.num_factor, fm.k0, fm.k1, self.task, fm.reg0, fm.regw, fm.regv,
                              0.0, self.min_target, self.max_target, device=devs[0] if devs else self.device)
        self._h.set_params(fm.w0, fm.w, fm.v)
        self._h.set_groups(self.groups)

    def _v_table(self, x):
        """v_lambda-like value -> [G][k].  Scalar, the full [G][k] table, or a 1-D vector that ALWAYS means one value per
        attribute group (what `-regular 'r0,w_1..w_G,v_1..v_G'` supplies, libfm.cpp:353-363) -- never per factor."""
        G, k = self._h.G, max(self.fm.num_factor, 1)
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1 and x.shape[0] != 1:
            if x.shape[0] != G:
                raise ValueError("a 1-D v_lambda holds one value per attribute group (%d), got %d" % (G, x.shape[0]))
            x = x[:, None]
        return np.ascontiguousarray(np.broadcast_to(x, (G, k)))

    # fm_learn_mcmc::learn + _learn (fm_learn_mcmc.h:1160-1201, fm_learn_mcmc_simultaneous.h:56-270)
    def learn(self, train, test):
        h = self._h
        if self._queries and self.device_average:
            raise NotImplementedError("set_queries: the per-query AUC scores one parameter set, device_average reports the mean over the draws")
        train.upload(h, 0)
        test.upload(h, 1)
        self._train, self._test = train, test
        for slot, d in ((0, train), (1, test)):
            if id(d) in self._queries:
                h.set_row_queries(slot, *self._queries[id(d)])
        self.pred_sum_all = np.zeros(test.num_cases)
        if self.device_average:
            h.post_begin(1)
        h.als_begin(0)
        for i in range(self.num_iter):
            st = h.als_sweep(self.w_lambda, self._v_table(self.v_lambda), 1.0, 0.0, 0.0, self.do_sample, self.seed)
            row = {"train": st.train_metric, "time_learn": st.device_seconds, "levels": st.levels}
            if self.device_average:
                row.update(self._post_iteration(i, st)[1])
                self.log.append(row)
                self._log_post_metrics(i)
                continue
            p = h.predict(1, test.num_cases)
            if self.task == TASK_REGRESSION:                  # :127-138
                self.pred_this = p
                self.pred_sum_all += np.maximum(self.min_target, np.minimum(self.max_target, p))
                rmse_test = float(np.sqrt(np.mean((self.pred_sum_all / (i + 1) - test.target) ** 2)))
                print("#Iter=%3d\tTrain=%g\tTest=%g" % (i, st.train_metric, rmse_test), file=self.out)
            else:                                             # :151-161
                self.pred_this = cdf_gaussian(p)
                self.pred_sum_all += self.pred_this
                acc = float(np.mean(((self.pred_sum_all / (i + 1)) >= 0.5) == (test.target >= 0)))
                print("#Iter=%3d\tTrain=%g\tTest=%g" % (i, st.train_metric, acc), file=self.out)
            self.log.append(row)
            _log_extra_metrics(self, i, train, test)
            _log_query_metrics(self, i, train, test)
        if self.device_average:
            self._post_download(test)
        h.als_end()
        self.fm.w0, self.fm.w, self.fm.v = h.get_params(self.fm.w, self.fm.v)

    # device_average: the test predictions of fm_learn_mcmc_simultaneous.h:127-161, 213-264 without leaving the device
    def _post_iteration(self, i, st):
        """add the sweep's draw to the accumulator of slot 1 and print the reference's `#Iter=` line from the mean over all draws.
        Returns (the line's test metric, the reference's rlog fields of the three vectors)."""
        ps = self._h.post_accumulate(1)
        m, row = ps.m[capi.POST_ALL], {}
        names = (("this", capi.POST_THIS), ("all", capi.POST_ALL), ("all_but5", capi.POST_LATE))
        if self.task == TASK_REGRESSION:                      # :213-226
            metric = m.rmse
            print("#Iter=%3d\tTrain=%g\tTest=%g" % (i, st.train_metric, metric), file=self.out)
            for name, q in names:
                row["rmse_mcmc_" + name] = ps.m[q].rmse
        else:                                                 # :237-253
            metric = m.accuracy
            print("#Iter=%3d\tTrain=%g\tTest=%g\tTest(ll)=%g" % (i, st.train_metric, metric, m.ll_ref), file=self.out)
            for name, q in names:
                row["acc_mcmc_" + name], row["ll_mcmc_" + name] = ps.m[q].accuracy, ps.m[q].ll_ref
        return metric, row

    def _log_post_metrics(self, i):
        """extra_metrics of the averaged test prediction: one stderr line per named metric, <metric>_test in the log row"""
        names = tuple(self.extra_metrics)
        for m in names:
            if m not in EXTRA_METRICS:
                raise ValueError("unknown metric %r (want auc, logloss)" % (m,))
        if not names or self.task != TASK_CLASSIFICATION:
            return
        te = self._h.post_evaluate_ex(1, capi.POST_ALL)
        for m in names:
            print("#Iter=%3d\t%s: Test=%g" % (i, m, getattr(te, m)), file=sys.stderr)
            self.log[-1][m + "_test"] = getattr(te, m)

    def _post_download(self, test):
        """pred_sum_all / pred_this of the finished run, once"""
        self.pred_sum_all, _ = self._h.post_get(1, capi.POST_ALL, test.num_cases)
        self.pred_this, _ = self._h.post_get(1, capi.POST_THIS, test.num_cases)

    def evaluate_ex(self, data):
        """exact AUC and log loss (probit link: this learner's probability is cdf_gaussian(y-hat)) of the train or test set of the
        running learn() under the parameters of the last sweep (fmx_evaluate_ex / fmx_group_evaluate_ex); with device_average,
        of the test set's mean over the draws (fmx_post_evaluate_ex)"""
        if data is not self._train and data is not self._test:
            raise ValueError("evaluate_ex: the data set is neither the train nor the test set of learn()")
        if self.device_average:
            if data is not self._test:
                raise NotImplementedError("evaluate_ex: device_average averages the test predictions only, like the reference")
            return self._h.post_evaluate_ex(1, capi.POST_ALL)
        return self._h.evaluate_ex(0 if data is self._train else 1, capi.LINK_PROBIT)

    def set_queries(self, data, qid, n_queries=None):
        """one query id (user, session) per row of the train or test set, before learn(): the iterations then report the
        per-query AUC of the set under the parameters of the sweep (fmx_set_row_queries)"""
        self._queries[id(data)] = (_check_queries(data, qid), n_queries)
        if data is self._train or data is self._test:
            self._h.set_row_queries(0 if data is self._train else 1, *self._queries[id(data)])

    def evaluate_by_query(self, data):
        """exact AUC inside every query of the train or test set of learn() under the parameters of the last sweep
        (fmx_evaluate_by_query / fmx_group_evaluate_by_query; probit link for the pooled log loss)"""
        if data is not self._train and data is not self._test:
            raise ValueError("evaluate_by_query: the data set is neither the train nor the test set of learn()")
        if id(data) not in self._queries:
            raise ValueError("evaluate_by_query: the data set has no query ids (set_queries)")
        return self._h.evaluate_by_query(0 if data is self._train else 1, capi.LINK_PROBIT)

    def evaluate_rank(self, data, cutoffs):
        """exact tie-averaged NDCG, recall and precision at the cutoffs inside every query of the train or test set of learn() under
        the parameters of the last sweep (fmx_evaluate_rank / fmx_group_evaluate_rank)"""
        if data is not self._train and data is not self._test:
            raise ValueError("evaluate_rank: the data set is neither the train nor the test set of learn()")
        if id(data) not in self._queries:
            raise ValueError("evaluate_rank: the data set has no query ids (set_queries)")
        return self._h.evaluate_rank(0 if data is self._train else 1, cutoffs, capi.LINK_PROBIT)

    TOPK_SLOTS = (2, 3)             # learn() keeps train and test in slots 0 and 1

    def recommend(self, queries, candidates, topk, exclude=None):
        """as FMLearnSGD.recommend, with the parameters of the last sweep; queries and candidates go into slots 2 and 3"""
        if len(self._shards) > 1:
            raise NotImplementedError("recommend: top-K retrieval is not supported on feature shards (devices lists %d GPUs)"
                                      % len(self._shards))
        return self._h.topk(*self._topk_slots(queries, candidates), topk, 0, queries.num_cases, exclude)

    def _topk_slots(self, queries, candidates):
        qs, cs = self.TOPK_SLOTS
        queries.upload(self._h, qs)
        if candidates is queries:
            cs = qs
        else:
            candidates.upload(self._h, cs)
        return qs, cs

    EVAL_LINK = capi.LINK_PROBIT    # this learner's probability is cdf_gaussian(y-hat)

    def evaluate(self, data):
        """rmse (regression) or accuracy of the train or test set of learn() under the parameters of the last sweep (fmx_evaluate)"""
        ev = self._h.evaluate(self._compact_slot(data))
        return ev.rmse if self.task == TASK_REGRESSION else ev.accuracy

    def _compact_slot(self, data):
        if data is not self._train and data is not self._test:
            raise ValueError("compact: the data set is neither the train nor the test set of learn()")
        return 0 if data is self._train else 1

    def _link(self, p):
        """one parameter set's prediction as fm_learn_mcmc::predict clamps it (fm_learn_mcmc.h:380-404)"""
        if self.task == TASK_REGRESSION:
            return np.maximum(self.min_target, np.minimum(self.max_target, p))
        return np.maximum(0.0, np.minimum(1.0, cdf_gaussian(p)))

    def _compact_train_slot(self):
        return 0

    def compact(self, format="bf16", prune=None):
        """a CompactView of the parameters of the last sweep (fmx_compact_begin, or fmx_compact_begin_pruned with prune = "dead" |
        "seen"); its data sets are the train and test set of learn().  Not on feature shards."""
        if len(self._shards) > 1:
            raise NotImplementedError("compact: the serving snapshot is not supported on feature shards (devices lists %d GPUs)"
                                      % len(self._shards))
        return CompactView(self, format, prune)

    # fm_learn_mcmc::predict (fm_learn_mcmc.h:380-404)
    def predict(self, data):
        out = self.pred_sum_all / self.num_iter if self.do_sample else self.pred_this.copy()
        if self.task == TASK_REGRESSION:
            return np.maximum(self.min_target, np.minimum(self.max_target, out))
        return np.maximum(0.0, np.minimum(1.0, out))

    def close(self):
        if self._h is not None:
            self._h.close()
            self._h = None
        for s in self._shards:
            s.close()
        self._shards = []


class FMLearnMCMC(FMLearnALS):
    """fm_learn_mcmc_simultaneous with do_sample = 1, do_multilevel = 1 -- `-method mcmc` (libfm.cpp:283-290).

    The coordinate draws run on the GPU (fmx_als_sweep with do_sample = 1); the hyper-prior draws are scalar work
    and stay on the host, in the reference's order (draw_all, fm_learn_mcmc.h:430-527): alpha (:911-939), w_lambda
    (:985-1017), w_mu (:941-983), v_lambda (:1061-1097), v_mu (:1019-1059), from statistics reduced on the device
    (fmx_als_moments).  Hyper-priors alpha_0 = gamma_0 = beta_0 = 1, mu_0 = 0 (:1106-1109).  Random numbers come
    from numpy / a counter hash, not libc rand(): parity with the reference is statistical."""

    def recommend(self, queries, candidates, topk, exclude=None):
        raise NotImplementedError("recommend: the MCMC prediction is the average over the draws (pred_sum_all / num_iter); "
                                  "no single parameter set scores it")

    def compact(self, format="bf16", prune=None):
        raise NotImplementedError("compact: the MCMC prediction is the average over the draws (pred_sum_all / num_iter); "
                                  "a snapshot of one parameter set does not score it")

    def __init__(self):
        super().__init__()
        self.do_sample = True
        self.do_multilevel = True
        self.alpha_0 = self.gamma_0 = self.beta_0 = 1.0
        self.mu_0 = 0.0

    def set_queries(self, data, qid, n_queries=None):
        raise NotImplementedError("set_queries: the MCMC prediction is the average over the draws (pred_sum_all / num_iter); "
                                  "no single parameter set scores it")

    def evaluate_by_query(self, data):
        raise NotImplementedError("evaluate_by_query: the MCMC prediction is the average over the draws (pred_sum_all / num_iter); "
                                  "no single device pass scores it")

    def evaluate_rank(self, data, cutoffs):
        raise NotImplementedError("evaluate_rank: the MCMC prediction is the average over the draws (pred_sum_all / num_iter); "
                                  "no single device pass scores it")

    def evaluate_ex(self, data):
        if self.device_average:
            return super().evaluate_ex(data)
        raise NotImplementedError("evaluate_ex: the MCMC prediction is the average over the draws (pred_sum_all / num_iter); "
                                  "no single device pass scores it")

    def learn(self, train, test):
        if tuple(self.extra_metrics) and not self.device_average:
            raise NotImplementedError("extra_metrics: the MCMC prediction is the average over the draws (pred_sum_all / num_iter); "
                                      "no single device pass scores it")
        h = self._h
        rng = np.random.default_rng(self.seed)
        k, n, G = self.fm.num_factor, self.fm.num_attribute, h.G
        train.upload(h, 0)
        test.upload(h, 1)
        self._train, self._test = train, test
        self.pred_sum_all = np.zeros(test.num_cases)
        if self.device_average:
            h.post_begin(1)
        N = train.num_cases
        # meta->num_attr_per_group (Data.h:93-95)
        n_g = np.array([float(n)]) if self.groups is None else np.bincount(np.asarray(self.groups), minlength=G).astype(np.float64)
        alpha = 1.0
        w_mu, w_lambda = np.zeros(G), np.broadcast_to(np.asarray(self.w_lambda, dtype=np.float64), (G,)).copy()
        v_mu, v_lambda = np.zeros((G, max(k, 1))), self._v_table(self.v_lambda).copy()
        a0, g0, b0, m0 = self.alpha_0, self.gamma_0, self.beta_0, self.mu_0
        h.als_begin(0)
        for i in range(self.num_iter):
            if self.do_multilevel:
                sum_e2, _, mom = h.als_moments()               # mom[1 + k][G][{sum, sum of squares}]
                alpha = rng.gamma((a0 + N) / 2.0) / ((g0 + sum_e2) / 2.0)                        # draw_alpha :911-922
                if self.fm.k1:
                    sw, sw2 = mom[0, :, 0], mom[0, :, 1]
                    gam = b0 * (w_mu - m0) ** 2 + g0 + (sw2 - 2 * w_mu * sw + n_g * w_mu * w_mu)   # draw_w_lambda :985-997
                    w_lambda = _keep_finite(rng.gamma((a0 + n_g + 1) / 2.0) / (gam / 2.0), w_lambda)
                    mean = (sw + b0 * m0) / (n_g + b0)                                            # draw_w_mu :946-959
                    w_mu = _keep_finite(mean + rng.standard_normal(G) * np.sqrt(1.0 / ((n_g + b0) * w_lambda)), w_mu)
                if k > 0:
                    sv, sv2 = mom[1:, :, 0].T, mom[1:, :, 1].T                                    # [G][k]
                    ng = n_g[:, None]
                    gam = b0 * (v_mu - m0) ** 2 + g0 + (sv2 - 2 * v_mu * sv + ng * v_mu ** 2)     # draw_v_lambda :1061-1075
                    v_lambda = _keep_finite(rng.gamma(np.broadcast_to((a0 + ng + 1) / 2.0, gam.shape)) / (gam / 2.0), v_lambda)
                    mean = (sv + b0 * m0) / (ng + b0)                                             # draw_v_mu :1019-1037
                    v_mu = _keep_finite(mean + rng.standard_normal(mean.shape) * np.sqrt(1.0 / ((ng + b0) * v_lambda)), v_mu)
            st = h.als_sweep(w_lambda, v_lambda, alpha, w_mu, v_mu, self.do_sample, self.seed * 7919 + 13)
            post_row = {}
            if self.device_average:
                metric, post_row = self._post_iteration(i, st)
            else:
                p = h.predict(1, test.num_cases)
                if self.task == TASK_REGRESSION:
                    self.pred_this = p
                    self.pred_sum_all += np.maximum(self.min_target, np.minimum(self.max_target, p))
                    metric = float(np.sqrt(np.mean((self.pred_sum_all / (i + 1) - test.target) ** 2)))
                else:
                    self.pred_this = cdf_gaussian(p)
                    self.pred_sum_all += self.pred_this
                    metric = float(np.mean(((self.pred_sum_all / (i + 1)) >= 0.5) == (test.target >= 0)))
                print("#Iter=%3d\tTrain=%g\tTest=%g" % (i, st.train_metric, metric), file=self.out)
            row = {"train": st.train_metric, "test": metric, "alpha": alpha, "time_learn": st.device_seconds}
            row.update(post_row)
            for g in range(G):                                                                    # rlog fields :1145-1157
                row["wmu[%d]" % g], row["wlambda[%d]" % g] = float(w_mu[g]), float(w_lambda[g])
            row["w_lambda"] = float(w_lambda[0])
            self.log.append(row)
            if self.device_average:
                self._log_post_metrics(i)
        if self.device_average:
            self._post_download(test)
        self.w_mu, self.w_lambda_last, self.v_mu, self.v_lambda_last = w_mu, w_lambda, v_mu, v_lambda
        h.als_end()
        self.fm.w0, self.fm.w, self.fm.v = h.get_params(self.fm.w, self.fm.v)


def _keep_finite(new, old):
    """the reference keeps the old value of a hyper-parameter whose draw is NaN / Inf (fm_learn_mcmc.h:961-975 etc.)"""
    new = np.asarray(new, dtype=np.float64)
    return np.where(np.isfinite(new), new, old)


class FMLearnPairSGD(FMLearnSGD):
    """Pairwise ranking (BPR) around the reference's fm_pairSGD (fm_sgd.h:53-126) on the GPU.  The reference has the update but
    no learner that calls it; the loop is include/fmx.h's: per pair (a, b), "row a preferred to row b", mult = -(1 - sigmoid(y_a - y_b))
    and one fm_pairSGD step.  Fields: num_iter, learn_rate, mode ('sequential': the pairs in order, 'minibatch': the batch rule),
    batch (minibatch: pairs per batch, 0 = the library's default).  Pairs are (row_a, row_b) arrays of 0-based rows of their data."""

    MODES = {"sequential": capi.SGD_SEQUENTIAL, "minibatch": capi.SGD_MINIBATCH}
    OPTIMIZERS = ("sgd",)

    def __init__(self):
        super().__init__()
        self.mode = "sequential"
        self._pairs = {}

    def _pair_slot(self, data, pairs):
        slot = self._slot(data)
        a, b = (np.ascontiguousarray(p, dtype=np.uint32) for p in pairs)
        key = (a.tobytes(), b.tobytes())
        if self._pairs.get(slot) != key:                        # (new or resampled pairs replace the old ones)
            self._h.upload_pairs(slot, a, b)
            self._pairs[slot] = key
        return slot

    def evaluate_pairs(self, data, pairs=None):
        """pair accuracy (fraction of pairs with y_a > y_b) over the pairs last uploaded for `data` (or these)"""
        slot = self._pair_slot(data, pairs) if pairs is not None else self._slot(data)
        return self._h.pair_evaluate(slot).accuracy

    # the epoch calls of learn() and learn_implicit(): what a subclass with another update rule overrides
    def _pair_epoch(self, slot):
        return self._h.pair_epoch(slot, self.MODES[self.mode], self.batch)

    def _pair_epoch_sampled(self, query_slot, n_neg, seed, epoch, neg_draws):
        return self._h.pair_epoch_sampled(query_slot, self.MODES[self.mode], self.batch, n_neg, seed, epoch, draws=neg_draws)

    def learn(self, train, train_pairs, test, test_pairs):
        self._check_optimizer()
        if self.mode not in self.MODES:
            raise ValueError("unknown mode for pairwise SGD: %s (sequential | minibatch)" % self.mode)
        print("learnrate=%g" % self.learn_rate, file=self.out)
        print("#iterations=%d" % self.num_iter, file=self.out)
        st = self._pair_slot(train, train_pairs)
        se = self._pair_slot(test, test_pairs)
        self._train = train
        for i in range(self.num_iter):
            stats = self._pair_epoch(st)
            tr, te = self._h.pair_evaluate(st), self._h.pair_evaluate(se)
            print("#Iter=%3d\tTrain=%g\tTest=%g" % (i, tr.accuracy, te.accuracy), file=self.out)
            print("#Iter=%3d\tloss: Train=%g\tTest=%g" % (i, tr.loss, te.loss), file=sys.stderr)
            self.log.append({"accuracy_train": tr.accuracy, "accuracy_test": te.accuracy, "loss_train": tr.loss,
                             "loss_test": te.loss, "time_learn": stats.device_seconds})
        self.sync_model()

    # implicit feedback: interactions over query rows x candidate rows, negatives drawn on the device ----------------------
    EVAL_EPOCH = 1 << 32          # the ONE sampler epoch both evaluations use (no training epoch reaches it)

    @staticmethod
    def _interactions(x, what):
        if isinstance(x, tuple) and len(x) == 2:
            q, c = x
        else:
            x = np.asarray(x)
            if x.ndim != 2 or x.shape[1] != 2:
                raise ValueError("%s: want (q_row, c_row) or an [n, 2] array" % what)
            q, c = x[:, 0], x[:, 1]
        q, c = np.ascontiguousarray(q, dtype=np.uint32), np.ascontiguousarray(c, dtype=np.uint32)
        if q.shape != c.shape or q.ndim != 1:
            raise ValueError("%s: q_row and c_row must be 1-d arrays of one length" % what)
        return q, c

    @staticmethod
    def _positives_csr(n_query, *inter):
        """per query row, the candidate rows of its interactions: the CSR (ptr [n_query + 1], idx)"""
        q = np.concatenate([i[0] for i in inter]).astype(np.int64)
        c = np.concatenate([i[1] for i in inter]).astype(np.uint32)
        if len(q) and int(q.max()) >= n_query:
            raise ValueError("an interaction names query row %d of %d" % (int(q.max()), n_query))
        ptr = np.zeros(n_query + 1, dtype=np.uint64)
        ptr[1:] = np.cumsum(np.bincount(q, minlength=n_query))
        return ptr, c[np.argsort(q, kind="stable")]

    def evaluate_implicit(self):
        """(train, test) pair metrics (capi.PairEval: accuracy, loss) of the interactions of the last learn_implicit under the
        current parameters, on the fixed evaluation epoch; test is None without test interactions"""
        sq, se, n_neg, seed = self._implicit
        h = self._h
        return (h.pair_evaluate_sampled(sq, n_neg, seed, self.EVAL_EPOCH),
                h.pair_evaluate_sampled(se, n_neg, seed, self.EVAL_EPOCH) if se is not None else None)

    def learn_implicit(self, queries, candidates, interactions, test_interactions=None, n_neg=1, seed=0, exclude="positives",
                       test_queries=None, neg_draws=1):
        """BPR on observed (query row, candidate row) interactions (fmx_pair_epoch_sampled): every interaction is paired with
        n_neg candidate rows drawn on the device, epoch i with the negatives of (seed, i); the joined rows queries[q] ++
        candidates[c] are never written.  interactions / test_interactions: (q_row, c_row) or an [n, 2] array; the test
        interactions name rows of test_queries (default: of queries).  exclude: what a query never gets as a negative --
        "positives" (its own interactions; for the test pairs the train and test interactions together, when both name rows of
        queries), None, a CSR (ptr, idx) over the query rows or a list of iterables.  neg_draws = M > 1: every training negative
        is the hardest of M accepted draws under the parameters at the start of its epoch (FMX_NEG_HARDEST).  The #Iter= lines
        come from fmx_pair_evaluate_sampled on one fixed epoch number and on UNIFORM negatives whatever neg_draws is, so the curves
        of different samplers measure the same thing; recommend() works on the trained model."""
        self._train = None                                           # (two slots, not one training set: compact(prune="seen") refuses)
        neg_draws = int(neg_draws)
        if not 1 <= neg_draws <= capi.NEG_ATTEMPTS:
            raise ValueError("neg_draws must be in 1 .. %d" % capi.NEG_ATTEMPTS)
        if self.mode not in self.MODES:
            raise ValueError("unknown mode for pairwise SGD: %s (sequential | minibatch)" % self.mode)
        print("learnrate=%g" % self.learn_rate, file=self.out)
        print("#iterations=%d" % self.num_iter, file=self.out)
        h = self._h
        tr = self._interactions(interactions, "interactions")
        te = None if test_interactions is None else self._interactions(test_interactions, "test_interactions")
        sq, sc = self._slot(queries), self._slot(candidates)
        ex_tr = self._positives_csr(queries.num_cases, tr) if isinstance(exclude, str) and exclude == "positives" else exclude
        h.upload_interactions(sq, sc, tr[0], tr[1], ex_tr)
        se = None
        if te is not None:
            if test_queries is None or test_queries is queries:   # a slot holds ONE set of interactions: the test set's live on a copy of the rows
                if not hasattr(self, "_query_copy") or self._query_copy[0] is not queries:
                    self._query_copy = (queries, Data(queries.entries, queries.row_ptr, queries.target))
                tq, both = self._query_copy[1], (tr, te)
            else:
                tq, both = test_queries, (te,)
            se = self._slot(tq)
            ex_te = self._positives_csr(tq.num_cases, *both) if isinstance(exclude, str) and exclude == "positives" else exclude
            if isinstance(ex_te, tuple) and len(ex_te) == 2 and len(ex_te[0]) != tq.num_cases + 1:
                raise ValueError("learn_implicit: the exclusion CSR covers %d query rows, test_queries has %d (pass queries of one "
                                 "row count, or exclude='positives')" % (len(ex_te[0]) - 1, tq.num_cases))
            h.upload_interactions(se, sc, te[0], te[1], ex_te)
        self._implicit = (sq, se, n_neg, seed)
        for i in range(self.num_iter):
            stats, forced = self._pair_epoch_sampled(sq, n_neg, seed, i, neg_draws)
            e_tr, e_te = self.evaluate_implicit()
            acc_te, loss_te = (e_te.accuracy, e_te.loss) if e_te is not None else (float("nan"), float("nan"))
            print("#Iter=%3d\tTrain=%g\tTest=%g" % (i, e_tr.accuracy, acc_te), file=self.out)
            print("#Iter=%3d\tloss: Train=%g\tTest=%g" % (i, e_tr.loss, loss_te), file=sys.stderr)
            self.log.append({"accuracy_train": e_tr.accuracy, "accuracy_test": acc_te, "loss_train": e_tr.loss, "loss_test": loss_te,
                             "time_learn": stats.device_seconds, "time_setup": stats.setup_seconds, "forced": forced,
                             "neg_draws": neg_draws})
        self.sync_model()


class FMLearnPairAdaptive(FMLearnPairSGD):
    """FMLearnPairSGD with a per-coordinate step on the pairwise batch rule: optimizer 'adagrad' (fmx_adapt_pair_epoch*: the step of a
    coordinate stays below eta per batch whatever a popular item's segment sums) or 'ftrl' (fmx_ftrl_pair_epoch*: FTRL-proximal with
    L1, exact zeros), with FMLearnSGD's fields for them (init_acc, adapt_learn_rate, ftrl_alpha, ftrl_beta, l1_w / l1_v, l2_w / l2_v);
    'sgd' is FMLearnPairSGD's plain rule.  init() opens the session; both rules run on mode 'minibatch' only (batch = 1 is the
    per-pair rule).  Everything else -- learn(), learn_implicit(), sparsity(), recommend(), compact() -- is inherited."""

    OPTIMIZERS = FMLearnSGD.OPTIMIZERS

    def __init__(self):
        super().__init__()
        self.mode = "minibatch"

    def _pair_epoch(self, slot):
        if self._adapt_open:
            return self._h.adapt_pair_epoch(slot, self.batch)
        if self._ftrl_open:
            return self._h.ftrl_pair_epoch(slot, self.batch)
        return super()._pair_epoch(slot)

    def _pair_epoch_sampled(self, query_slot, n_neg, seed, epoch, neg_draws):
        if self._adapt_open:
            return self._h.adapt_pair_epoch_sampled(query_slot, self.batch, n_neg, seed, epoch, neg_draws)
        if self._ftrl_open:
            return self._h.ftrl_pair_epoch_sampled(query_slot, self.batch, n_neg, seed, epoch, neg_draws)
        return super()._pair_epoch_sampled(query_slot, n_neg, seed, epoch, neg_draws)

    def _check_session(self):
        self._check_optimizer()
        if (self.optimizer == "adagrad") != self._adapt_open or (self.optimizer == "ftrl") != self._ftrl_open:
            raise ValueError("optimizer was changed after init()")

    def learn(self, train, train_pairs, test, test_pairs):
        self._check_session()
        super().learn(train, train_pairs, test, test_pairs)

    def learn_implicit(self, *args, **kw):
        self._check_session()
        super().learn_implicit(*args, **kw)


class FMLearnSGDA(FMLearnSGD):
    """fm_learn_sgd_element_adapt_reg (`-method sgda`, fm_learn_sgd_element_adapt_reg.h:44-93) on the GPU: theta steps
    on the train rows alternate with lambda steps on `validation` (libfm.cpp:276-279).  gpu_batch = 0: the reference's
    strictly online order (one wavefront, parity); > 0: the batch form (fmx_sgda_epoch_minibatch)."""

    OPTIMIZERS = ("sgd",)

    def __init__(self):
        super().__init__()
        self.gpu_batch, self.gpu_w0_chunk = 0, 0
        self.validation = None
        self.groups = None               # DataMetaInfo::attr_group (None = one group)
        self.reg_w = 0.0                 # one group: scalar / [k]; with groups: [G] / [G][k]  (:84-85)
        self.reg_v = None

    def learn(self, train, test):
        if self.validation is None:
            raise ValueError("sgda needs a validation set")              # the reference asserts (libfm.cpp:277)
        self._check_optimizer()
        print("Training using self-adaptive-regularization SGD.", file=self.out)
        h = self._h
        st, sv = self._slot(train), self._slot(self.validation)
        self._train = train
        self.fm.reg0 = self.fm.regw = self.fm.regv = 0.0                  # :257-259
        h.set_groups(self.groups)
        h.sgda_begin()
        for i in range(self.num_iter):
            stats = (h.sgda_epoch_minibatch(st, sv, i > 0, self.gpu_batch, self.gpu_w0_chunk) if self.gpu_batch > 0
                     else h.sgda_epoch(st, sv, i > 0))
            rmse_val = self.evaluate(self.validation)
            rmse_train = self.evaluate(train)
            rmse_test = self.evaluate(test)
            print("#Iter=%3d\tTrain=%g\tTest=%g" % (i, rmse_train, rmse_test), file=self.out)
            reg = h.sgda_get_reg()                                           # [G][1 + k]
            if h.G == 1:
                self.reg_w, self.reg_v = float(reg[0, 0]), reg[0, 1:].copy()
            else:
                self.reg_w, self.reg_v = reg[:, 0].copy(), reg[:, 1:].copy()
            row = {"rmse_train": rmse_train, "rmse_val": rmse_val, "time_learn": stats.device_seconds}
            for g in range(h.G):                                             # rlog fields :119-132
                row["regw[%d]" % g] = float(reg[g, 0])
                for f in range(self.fm.num_factor):
                    row["regv[%d,%d]" % (g, f)] = float(reg[g, 1 + f])
            self.log.append(row)
            _log_extra_metrics(self, i, train, test)
            _log_query_metrics(self, i, train, test)
        h.sgda_end()
        self.sync_model()
