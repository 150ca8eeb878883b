"""Command line with libFM's flags on top of the GPU learners (host side only; all arithmetic is in libfmx.so).

    python -m libfm_amd.cli -task r -train tr.libfm -test te.libfm -dim 1,1,8 -iter 20 -method sgd \
           -learn_rate 0.01 -regular 0,0,0.01 -init_stdev 0.1 -seed 42 -out pred.txt -save_model model.txt

Mirrors the driver of the reference (src/libfm/libfm.cpp:62-441): same flag names and defaults (:76-121), the flag
syntax of CMDLine (`-x value`, lists separated by ',' or ';', src/util/cmdline.h:80-105), binary-or-text data
auto-detection (Data.h:113-125), `-seed` reproducing the reference's initial model bit for bit (refrand.py),
targets rewritten to +-1 for `-task c` (:298-306), regularisation / learning-rate parsing (:326-404), the
`#Iter=...` progress lines, `-out` (:423-428), `-save_model` / `-load_model` (:262-268, :431-434), and the
reference's error convention: "ERROR: ..." on stderr and exit status 0 (:436-441).
`-meta` (attribute groups, :199-242 / Data.h:85-97) is honoured by als / mcmc / sgda, incl. `-regular 'r0,w_1..w_G,v_1..v_G'`
(:353-363).  `-relation a,b` (block structure, :172-196; als / mcmc only like the reference's learners) loads <a>.x or
<a>.xt, <a>.train, <a>.test and optional <a>.groups; the joined rows are expanded on the device.  `-cache_size` is
accepted and ignored (everything is resident).
GPU-only additions: -gpu_mode sequential|minibatch|hogwild (default minibatch), -batch, -w0_chunk, -device.
Top-K retrieval after training (every method but mcmc): -topk K -candidates F [-queries F] [-exclude F] [-topk_out F] ranks the
candidate rows for every query row (default: the test rows) by the raw prediction of the joined row (fmx_topk).
Implicit feedback: -method bpr -train Q -test Qtest -candidates C -interactions F [-test_interactions F] [-neg N] trains on the
observed (query row of -train, candidate row) interactions of F with N negatives per interaction drawn on the device
(fmx_pair_epoch_sampled); the test interactions name rows of -test.  -train_pairs / -test_pairs are not needed then.
-neg_draws M (1 .. 16, default 1) trains every negative as the hardest of M accepted draws under the parameters at the start of
the epoch; the #Iter= lines stay on uniform negatives.
-metrics auc,logloss (-task c with sgd, sgda, als): after every iteration the exact AUC and / or the log loss of the train and
test rows, reduced on the device (fmx_evaluate_ex), as "#Iter=  i\tauc: Train=..\tTest=.." lines on stderr and auc_train /
auc_test / logloss_train / logloss_test columns of -rlog; stdout stays byte for byte what it is without the flag.
-test_queries F [-train_queries F] (-task c with sgd, sgda, als): one non-negative integer per row of -test / -train, the row's
query (user, session).  After every iteration the impression-weighted exact AUC inside the queries (GAUC), reduced on the device
(fmx_evaluate_by_query), as one "#Iter=  i\tgauc: Train=..\tTest=.." line on stderr (nan for a set without ids) and gauc_* /
auc_within_* columns of -rlog; stdout stays byte for byte what it is without the flags.
-rank_at K1,K2,... (needs -test_queries; at most 4 ascending integers in 1 .. 65536): after every iteration the exact tie-averaged
NDCG at each K inside the queries, reduced on the device (fmx_evaluate_rank: rows of equal score share their ranks in expectation,
so the figure does not depend on a sort's tie order), as one "#Iter=  i\tndcg@K: Train=..\tTest=.." line per K on stderr and
ndcg@K_* / recall@K_* / precision@K_* columns of -rlog; stdout stays byte for byte what it is without the flag.
-device_average 1 (als, mcmc): the test predictions and their running sums stay on the device (fmx_post_accumulate); the #Iter=
lines gain the reference's Test(ll) column on -task c, -rlog its rmse_mcmc_* / acc_mcmc_* / ll_mcmc_* columns, and -metrics then
scores the averaged test prediction ("#Iter=  i\tauc: Test=.." on stderr, auc_test / logloss_test) -- with -method mcmc too.
-optimizer sgd|adagrad [-init_acc X] (-method sgd, -gpu_mode minibatch): adagrad trains w and V with a per-coordinate step size on
the minibatch rule (fmx_adapt_epoch; -learn_rate is its eta and the bias's plain rate, X the start value of the accumulators,
default 1); the printed lines are those of sgd.  Without the option nothing changes.
-optimizer ftrl [-ftrl_alpha A] [-ftrl_beta B] [-l1 W,V] (-method sgd, -gpu_mode minibatch): FTRL-proximal with L1 on the minibatch
rule (fmx_ftrl_epoch): A the per-coordinate rate (default -learn_rate, which stays the bias's plain rate), B default 1, W and V the L1
strengths of the linear weights and the factors (default 0,0); the L2 strengths are -regular's regw and regv, one per coordinate.
After training one line on stderr gives the zero counts of the model (fmx_param_sparsity).
-method bpr -optimizer adagrad|ftrl (with the same options): the pairwise batch rule with that per-coordinate step
(fmx_adapt_pair_epoch* / fmx_ftrl_pair_epoch*, learner.FMLearnPairAdaptive), on -train_pairs and on -interactions; -gpu_mode then
defaults to minibatch (batch 1 is the per-pair rule) and sequential is refused.
-train_weights F [-test_weights F] (-method sgd with -optimizer adagrad | ftrl): one non-negative float per row of -train / -test,
the row's weight (fmx_set_row_weights): the epochs scale every train row's loss by its weight -- the way to train on subsampled
negatives, each kept one weighing 1 / rate.  -metrics then also knows wlogloss, the weighted log loss of the sets that have weights
(fmx_evaluate_weighted; nan for a set without), as "#Iter=  i\twlogloss: Train=..\tTest=.." on stderr and wlogloss_* in -rlog.
Any other method or optimizer refuses the flags: it has no weighted form.
-save_checkpoint F [-checkpoint_dense 1] / -load_checkpoint F (-method sgd and -method bpr, any -optimizer): the exact binary
checkpoint of the model and of the adagrad / ftrl session (fmx_checkpoint_save / _load; libfm_amd/checkpoint.py reads the file).
-load_checkpoint takes the place of the random initialisation and of -load_model (giving both is an error) and, when the file holds
a session, of the -optimizer options: training continues bit for bit where the saving run stopped.  -save_checkpoint writes the
file after training (-checkpoint_dense 1: every feature's state rows, not only those that differ from the start state).  Each
prints one "checkpoint" line on stderr: session, state rows, bytes, seconds.  Any other method refuses the flags.
-serve bf16 (sgd, sgda, bpr, als): after training a frozen bf16 copy of the model is taken on the device (fmx_compact_begin) and the
-out predictions and the -topk lists come from it.  One "compact" line on stderr carries the copy's bytes next to the fp32 tables',
max_abs_err and nonfinite of the rounding, and the test metric -- with -metrics each named metric too -- from fp32 and from bf16 side
by side.  -serve int8 takes the row-wise 8-bit copy instead (codes, scale and linear weight of a feature in one block; the line says
format=int8 and names its metrics (int8)).  Without the option stdout and stderr are byte for byte what they are.
-serve_prune dead|seen (with -serve): the copy keeps only the rows that can score (fmx_compact_begin_pruned) -- dead drops the features
that contribute to no prediction, seen also those no -train row names (not with -interactions, whose training rows are two files).
The "compact" line gains kept, dropped_dead, dropped_unseen, bytes_directory and bytes_rows; bytes is their sum.
-save_snapshot F (with -serve): the frozen copy is written to F after it is taken (fmx_compact_save; libfm_amd/compact.py reads the
file); one "snapshot" line on stderr: format, pruned, rows, bytes, seconds.
-method serve -load_snapshot F -test T [-out P] [-metrics ...] [-topk K -candidates C [-queries Q] [-exclude E] [-topk_out O]]: scores
from a snapshot file and creates NO model (fmx_serve_open: the device holds the snapshot alone).  -train and -dim are not needed -- the
geometry, the task and the target range are the file's -- and every training option is refused by name.  -out is written as the
training run's -out with -serve is (the link of -method sgd); one "serve" line on stderr carries the test metric, with -metrics each
named metric too.
-devices D0,D1[,...] (-method sgd with -optimizer adagrad | ftrl): the model is split into one feature shard per listed device
ordinal ("0,0" = two shards on device 0) and the epochs run over the shards (fmx_group_adapt_epoch / fmx_group_ftrl_epoch,
learner.FMLearnSGD.devices); the printed lines are those of one device.  Any other method or optimizer refuses the flag, and so do
-serve, -topk, -save_checkpoint, -load_checkpoint, -save_snapshot, -load_snapshot and -train_weights, which have no sharded form.
Without the flag nothing changes.
"""
import os
import sys
import time

import numpy as np

from . import compact as C
from . import data as D
from . import learner as L
from . import refrand as R

FLAGS = {"task": "r=regression, c=binary classification [MANDATORY]", "meta": "filename for meta information about data set", "train": "filename for training data [MANDATORY]",
         "test": "filename for test data [MANDATORY]", "validation": "", "out": "filename for output",
         "dim": "'k0,k1,k2': k0=use bias, k1=use 1-way interactions, k2=dim of 2-way interactions; default=1,1,8",
         "regular": "'r0,r1,r2' for SGD and ALS", "init_stdev": "stdev for initialization of 2-way factors; default=0.1",
         "iter": "number of iterations; default=100", "learn_rate": "learn_rate for SGD",
         "method": "sgd, sgda, als, mcmc, bpr; default=mcmc.  serve: score from -load_snapshot, no model, no training",
         "verbosity": "", "rlog": "write measurements within iterations to a file", "seed": "integer value", "help": "",
         "relation": "BS: filenames for the relations, default=''", "cache_size": "", "save_model": "filename for writing the FM model",
         "load_model": "filename for reading the FM model",
         "gpu_mode": "sequential | minibatch | hogwild (default minibatch; bpr: sequential | minibatch, default sequential)", "batch": "",
         "w0_chunk": "", "device": "",
         "train_pairs": "bpr: pairs of the train rows, one per line 'row_a row_b' (0-based rows; row_a is preferred) [MANDATORY for bpr]",
         "test_pairs": "bpr: pairs of the test rows, same format [MANDATORY for bpr]",
         "candidates": "top-K retrieval after training, bpr with -interactions: filename of the candidate rows (libFM text or binary)",
         "interactions": "bpr: observed interactions, one per line 'query_row cand_row' (0-based rows of -train and -candidates)",
         "test_interactions": "bpr with -interactions: held-out interactions, same format (rows of -test and -candidates)",
         "neg": "bpr with -interactions: negatives drawn per interaction; default=1",
         "neg_draws": "bpr with -interactions: train each negative as the best-scoring of M accepted draws (1 .. 16); default=1 (uniform)",
         "topk": "results per query row (1 .. 1024); needs -candidates; not with -method mcmc",
         "topk_out": "filename for the top-K lists: one line per query, 'cand:score cand:score ...'",
         "queries": "filename of the query rows; default: the test rows",
         "exclude": "filename of excluded pairs, one per line 'query_row cand_row'",
         "metrics": "'auc,logloss': exact AUC / log loss of train and test per iteration on stderr; -task c with sgd, sgda, als"
                    " (mcmc: of the averaged test prediction, with -device_average 1)",
         "test_queries": "filename with one query id (non-negative integer) per test row: per-query AUC (GAUC) per iteration on"
                         " stderr; -task c with sgd, sgda, als",
         "train_queries": "the same for the train rows; needs -test_queries",
         "rank_at": "'K1,K2,...' (at most 4, ascending, 1 .. 65536): tie-averaged NDCG / recall / precision at K inside the queries per"
                    " iteration on stderr and in -rlog; needs -test_queries",
         "device_average": "als, mcmc: 1 = keep the test predictions and their running mean on the device; default=0",
         "optimizer": "sgd, bpr: sgd | adagrad (a per-coordinate step size on the minibatch rule) | ftrl (FTRL-proximal with L1 on the same"
                      " rule: exact zeros); default=sgd.  bpr with adagrad | ftrl: -gpu_mode defaults to minibatch",
         "init_acc": "-optimizer adagrad: start value of every accumulator (> 0); default=1",
         "ftrl_alpha": "-optimizer ftrl: per-coordinate rate of w and V (> 0); default=-learn_rate",
         "ftrl_beta": "-optimizer ftrl: beta (> 0); default=1",
         "l1": "-optimizer ftrl: 'w,v' = L1 strength of the linear weights and of the factors (>= 0); default=0,0",
         "train_weights": "filename with one weight (float >= 0) per train row: -method sgd with -optimizer adagrad | ftrl scales every"
                          " row's loss by it; -metrics then knows wlogloss",
         "test_weights": "the same for the test rows (read by -metrics wlogloss only); needs -train_weights",
         "save_checkpoint": "sgd, bpr: filename for the exact binary checkpoint (model + adagrad / ftrl session) written after training",
         "checkpoint_dense": "with -save_checkpoint: 1 = write every feature's state rows; default=0 (only rows that differ from the start state)",
         "load_checkpoint": "sgd, bpr: filename of a checkpoint to continue from (instead of the random initialisation; not with -load_model)",
         "serve": "bf16 | int8: score -out, -metrics and -topk after training from a frozen bf16 or row-wise int8 copy of the model; sgd, sgda, bpr, als",
         "serve_prune": "dead | seen (with -serve): keep only the rows that can score -- dead: drop features that contribute to no prediction; seen: also those no -train row names",
         "save_snapshot": "with -serve: filename for the snapshot file of the frozen copy, written after it is taken",
         "load_snapshot": "-method serve: filename of the snapshot file to score from (no model is created; -train and -dim are not needed)",
         "devices": "'D0,D1,...': -method sgd with -optimizer adagrad | ftrl over one feature shard per listed device ordinal ('0,0': two shards on device 0)"}


def checkpoint_line(what, info):
    """the one stderr line of -save_checkpoint / -load_checkpoint (capi.CkptInfo)"""
    return "checkpoint\t%s\tsession=%s\tstate_rows=%d\tbytes=%d\tseconds=%.3g" % (
        what, L.capi.CKPT_SESSIONS[info.session], info.state_rows, info.bytes, info.seconds)


def snapshot_line(what, info):
    """the one stderr line of -save_snapshot / -load_snapshot (capi.SnapInfo)"""
    return "snapshot\t%s\tformat=%s\tpruned=%d\trows=%d\tbytes=%d\tseconds=%.3g" % (
        what, C.FORMAT_NAMES.get(int(info.format), "?"), info.pruned, info.rows, info.bytes, info.seconds)


# what -method serve takes; every other flag is a training option and is refused by name
SERVE_FLAGS = ("method", "load_snapshot", "test", "out", "metrics", "topk", "topk_out", "candidates", "queries", "exclude", "device", "task",
               "verbosity")


def _serve_main(a):
    """-method serve: score -test (and -topk lists) from the snapshot file -load_snapshot names, through a handle that holds no model"""
    for f in a:
        if f not in SERVE_FLAGS:
            raise ValueError("-%s is not supported with -method serve: it creates no model and trains nothing (it takes %s)"
                             % (f, ", ".join("-" + x for x in SERVE_FLAGS[1:])))
    if not a.get("load_snapshot"):
        raise ValueError("-method serve needs -load_snapshot with a filename")
    if not a.get("test"):
        raise ValueError("-test is mandatory")
    want_topk = any(f in a for f in ("topk", "topk_out", "candidates", "queries", "exclude"))
    if want_topk and ("topk" not in a or "candidates" not in a):
        raise ValueError("top-K retrieval needs -topk and -candidates")
    head = C.snapshot_header(a["load_snapshot"])                 # (refused from the header alone, before any device)
    task = "c" if head["task"] == L.TASK_CLASSIFICATION else "r"
    if a.get("task", task) != task:
        raise ValueError("-task %s but the snapshot was taken for -task %s" % (a["task"], task))
    metrics = tuple(split_list(a.get("metrics", "")))
    for m in metrics:
        if m not in L.EXTRA_METRICS:
            raise ValueError("-metrics knows auc and logloss, not '%s'" % m)
    if metrics and task != "c":
        raise ValueError("-metrics needs a snapshot of -task c: AUC and log loss are classification metrics")
    print("Loading test... \t")
    test = L.Data(*D.load(a["test"]))
    print("num_rows=%d\tnum_values=%d\tnum_features=%d\tmin_target=%g\tmax_target=%g" %
          (test.num_cases, len(test.entries), test.num_feature, test.min_target, test.max_target))
    if test.num_feature > head["num_attribute"]:
        raise ValueError("-test names feature %d, the snapshot holds %d features" % (test.num_feature - 1, head["num_attribute"]))
    if task == "c":                                                                  # libfm.cpp:302-306
        test.target[:] = np.where(test.target <= 0.0, -1.0, 1.0)
    view = L.load_snapshot(a["load_snapshot"], int(a.get("device", "-1")))
    try:
        print(snapshot_line("load", view.info), file=sys.stderr)
        line = "serve\tformat=%s\tbytes=%d\tTest(%s)=%g" % (view.format, view.info.bytes_compact, view.format, view.evaluate(test))
        if metrics:
            ex = view.evaluate_ex(test)
            line += "".join("\t%s(%s)=%g" % (m, view.format, getattr(ex, m)) for m in metrics)
        print(line, file=sys.stderr)
        if a.get("out"):
            with open(a["out"], "w") as f:                                               # DVector::save, matrix.h:332-342
                f.write("".join("%g\n" % p for p in view.predict(test)))
        if want_topk:
            topk = int(a["topk"])
            cand = L.Data(*D.load(a["candidates"]))
            queries = L.Data(*D.load(a["queries"])) if a.get("queries") else test
            for d, name in ((cand, "-candidates"), (queries, "-queries")):
                if d.num_feature > head["num_attribute"]:
                    raise ValueError("%s names feature %d, the snapshot holds %d features" % (name, d.num_feature - 1, head["num_attribute"]))
            exclude = read_exclude(a["exclude"], queries.num_cases, cand.num_cases) if a.get("exclude") else None
            idx, score = view.recommend(queries, cand, topk, exclude)
            print("Top-K\tqueries=%d\tcandidates=%d\tK=%d" % (queries.num_cases, cand.num_cases, topk))
            if a.get("topk_out"):
                write_topk(a["topk_out"], idx, score)
    finally:
        view.close()
    return 0


def read_pairs(path, n_rows):
    """a pairs file of -method bpr: one pair per line, 'row_a row_b', 0-based row numbers of the matching data file (row_a is
    preferred to row_b); blank lines and lines starting with '#' are skipped"""
    a, b = [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            if len(t) != 2:
                raise ValueError("cannot parse line %d of %s: want 'row_a row_b'" % (no, path))
            ra, rb = int(t[0]), int(t[1])
            if not (0 <= ra < n_rows and 0 <= rb < n_rows):
                raise ValueError("line %d of %s: row outside the data set (%d rows)" % (no, path, n_rows))
            a.append(ra)
            b.append(rb)
    return np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32)


def read_queries(path, n_rows):
    """a -test_queries / -train_queries file: one non-negative integer per line, the query id of the row with that line number;
    the line count must equal the rows of the data file"""
    ids = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            t = line.split()
            if len(t) != 1:
                raise ValueError("cannot parse line %d of %s: want one query id" % (no, path))
            q = int(t[0])
            if not 0 <= q < 2 ** 31 - 1:
                raise ValueError("line %d of %s: a query id is an integer in 0 .. 2^31 - 2 (got %d)" % (no, path, q))
            ids.append(q)
    if len(ids) != n_rows:
        raise ValueError("%s has %d lines, the data set has %d rows" % (path, len(ids), n_rows))
    return np.array(ids, dtype=np.uint32)


def read_weights(path, n_rows):
    """a -train_weights / -test_weights file: one finite float >= 0 per line, the weight of the row with that line number; the line
    count must equal the rows of the data file"""
    ws = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            t = line.split()
            if len(t) != 1:
                raise ValueError("cannot parse line %d of %s: want one weight" % (no, path))
            w = float(t[0])
            if not 0.0 <= w < float("inf"):
                raise ValueError("line %d of %s: a weight is a finite number >= 0 (got %s)" % (no, path, t[0]))
            ws.append(w)
    if len(ws) != n_rows:
        raise ValueError("%s has %d lines, the data set has %d rows" % (path, len(ws), n_rows))
    return np.array(ws, dtype=np.float32)


def read_exclude(path, n_query, n_cand):
    """an -exclude file: one pair per line, 'query_row cand_row' (0-based); returns the CSR (ptr [n_query + 1], idx)"""
    q, c = [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            if len(t) != 2:
                raise ValueError("cannot parse line %d of %s: want 'query_row cand_row'" % (no, path))
            qr, cr = int(t[0]), int(t[1])
            if not (0 <= qr < n_query and 0 <= cr < n_cand):
                raise ValueError("line %d of %s: row outside the query (%d) or candidate (%d) rows" % (no, path, n_query, n_cand))
            q.append(qr)
            c.append(cr)
    q = np.array(q, dtype=np.int64)
    order = np.argsort(q, kind="stable")
    ptr = np.zeros(n_query + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(np.bincount(q, minlength=n_query))
    return ptr, np.array(c, dtype=np.uint32)[order]


def read_interactions(path, n_query, n_cand):
    """an -interactions file: one interaction per line, 'query_row cand_row' (0-based; the format of -exclude), in file order;
    returns (q_row, c_row)"""
    q, c = [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            if len(t) != 2:
                raise ValueError("cannot parse line %d of %s: want 'query_row cand_row'" % (no, path))
            qr, cr = int(t[0]), int(t[1])
            if not (0 <= qr < n_query and 0 <= cr < n_cand):
                raise ValueError("line %d of %s: row outside the query (%d) or candidate (%d) rows" % (no, path, n_query, n_cand))
            q.append(qr)
            c.append(cr)
    return np.array(q, dtype=np.uint32), np.array(c, dtype=np.uint32)


def write_topk(path, idx, score):
    """one line per query: 'cand:score ...' with %g scores, padding entries left out"""
    none = np.uint32(0xFFFFFFFF)
    with open(path, "w") as f:
        for i, s in zip(idx, score):
            f.write(" ".join("%d:%g" % (int(c), float(v)) for c, v in zip(i, s) if c != none) + "\n")


def parse(argv):
    """CMDLine (cmdline.h:80-105): a flag is '-name' or '--name'; its value is the next token unless that starts with '-'."""
    vals, i = {}, 0
    while i < len(argv):
        a = argv[i]
        if not a.startswith("-"):
            raise ValueError("cannot parse parameter \"%s\"" % a)
        name = a.lstrip("-")
        if i + 1 < len(argv) and not argv[i + 1].startswith("-"):
            vals[name] = argv[i + 1]
            i += 2
        else:
            vals[name] = ""
            i += 1
    for k in vals:
        if k not in FLAGS:
            raise ValueError("the parameter " + k + " does not exist")      # cmdline.h:150-157
    return vals


def split_list(s):
    return [t for t in s.replace(";", ",").split(",") if t != ""]


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    try:
        return _main(argv)
    except (ValueError, OSError, RuntimeError) as e:
        print("\nERROR: %s" % e, file=sys.stderr)
        return 0                                                     # the reference exits 0 on errors (libfm.cpp:436-441)


def _main(argv):
    print("----------------------------------------------------------------------------")
    print("libfm_amd: MI355X-native FM learners behind libFM's command line")
    print("----------------------------------------------------------------------------")
    if not argv or "-help" in argv or "--help" in argv:
        for k, v in FLAGS.items():
            print("-%-14s %s" % (k, v))
        return 0
    a = parse(argv)
    seed = int(a["seed"]) if "seed" in a else int(time.time())
    method = a.get("method", "mcmc")
    if method == "serve":
        return _serve_main(a)
    if "load_snapshot" in a:
        raise ValueError("-load_snapshot belongs to -method serve")
    init_stdev = float(a.get("init_stdev", "0.1"))
    dim = [int(x) for x in split_list(a.get("dim", "1,1,8"))]
    if len(dim) != 3:
        raise ValueError("-dim needs k0,k1,k2")
    if method == "mcmc" and ("save_model" in a or "load_model" in a):
        print("WARNING: -save_model / -load_model enabled only for SGD and ALS.")      # libfm.cpp:123-133
        return 0
    if method not in ("sgd", "sgda", "als", "mcmc", "bpr"):
        raise ValueError("unknown method")
    implicit = method == "bpr" and "interactions" in a
    if not implicit and any(f in a for f in ("interactions", "test_interactions", "neg", "neg_draws")):
        raise ValueError("-interactions, -test_interactions, -neg and -neg_draws belong to -method bpr with -interactions")
    want_topk = any(f in a for f in ("topk", "topk_out", "queries", "exclude")) or ("candidates" in a and not implicit)
    if implicit and "candidates" not in a:
        raise ValueError("-interactions needs -candidates")
    if want_topk:
        if method == "mcmc":
            raise ValueError("-topk is not supported with -method mcmc: its prediction averages the draws, no single model scores it")
        if "topk" not in a or "candidates" not in a:
            raise ValueError("top-K retrieval needs -topk and -candidates")
    if method == "bpr":                      # pairwise ranking: the targets are not used, so -task is optional
        a.setdefault("task", "r")
        for need in ("train_pairs", "test_pairs"):
            if need not in a and not implicit:
                raise ValueError("-%s is mandatory for -method bpr" % need)
    for need in ("task", "train", "test"):
        if need not in a:
            raise ValueError("-%s is mandatory" % need)
    dev_avg = a.get("device_average", "0")
    if dev_avg not in ("0", "1"):
        raise ValueError("-device_average takes 0 or 1")
    dev_avg = dev_avg == "1"
    if dev_avg and method not in ("als", "mcmc"):
        raise ValueError("-device_average belongs to -method als and mcmc")
    optimizer = a.get("optimizer", "sgd")
    ftrl_flags = [f for f in ("ftrl_alpha", "ftrl_beta", "l1") if f in a]
    ftrl_l1 = (0.0, 0.0)
    if "optimizer" in a or "init_acc" in a or ftrl_flags:
        if optimizer not in L.FMLearnSGD.OPTIMIZERS:
            raise ValueError("-optimizer knows sgd and adagrad, not '%s' (ftrl is the third it knows)" % optimizer)
        if method not in ("sgd", "bpr"):                     # (bpr: the pairwise batch rule with the same two rules, FMLearnPairAdaptive)
            raise ValueError("-optimizer / -init_acc belong to -method sgd, not -method %s" % method)
        if optimizer == "ftrl" and a.get("gpu_mode", "minibatch") != "minibatch":
            raise ValueError("-optimizer ftrl runs on the minibatch rule: -gpu_mode %s is not supported" % a["gpu_mode"])
        if ftrl_flags:
            if optimizer != "ftrl":
                raise ValueError("-%s belongs to -optimizer ftrl" % ftrl_flags[0])
            for f in ("ftrl_alpha", "ftrl_beta"):
                if f in a and not (0.0 < float(a[f]) < float("inf")):
                    raise ValueError("-%s needs a finite value > 0" % f)
            if "l1" in a:
                ftrl_l1 = tuple(float(x) for x in split_list(a["l1"]))
                if len(ftrl_l1) != 2 or not all(0.0 <= x < float("inf") for x in ftrl_l1):
                    raise ValueError("-l1 needs 2 finite values >= 0: 'w,v'")
        if optimizer == "adagrad" and a.get("gpu_mode", "minibatch") != "minibatch":
            raise ValueError("-optimizer adagrad runs on the minibatch rule: -gpu_mode %s is not supported" % a["gpu_mode"])
        if "init_acc" in a:
            if optimizer != "adagrad":
                raise ValueError("-init_acc belongs to -optimizer adagrad")
            if not (0.0 < float(a["init_acc"]) < float("inf")):
                raise ValueError("-init_acc needs a finite value > 0")
    devices = None
    if "devices" in a:
        if method != "sgd" or optimizer not in L.FMLearnSGD.SHARDED_OPTIMIZERS:
            raise ValueError("-devices belongs to -method sgd with -optimizer adagrad or ftrl: -method %s%s has no form on feature shards"
                             % (method, " -optimizer " + optimizer if method in ("sgd", "bpr") else ""))
        for f in ("serve", "topk", "save_checkpoint", "load_checkpoint", "save_snapshot", "load_snapshot", "train_weights"):
            if f in a:
                raise ValueError("-%s is not supported with -devices: it has no form on feature shards" % f)
        try:
            devices = [int(x) for x in split_list(a["devices"])]
        except ValueError:
            devices = []
        if not devices or any(d < 0 for d in devices) or len(devices) > 16:
            raise ValueError("-devices needs 1 .. 16 device ordinals >= 0: 'D0,D1,...'")
    serve = a.get("serve")
    if "serve" in a:
        if serve not in C.FORMATS:
            raise ValueError("-serve knows bf16, not '%s' (also: %s)" % (serve, ", ".join(f for f in C.FORMATS if f != "bf16")))
        if method == "mcmc":
            raise ValueError("-serve is not supported with -method mcmc: its prediction averages the draws, no single model scores it")
        if a.get("relation"):
            raise ValueError("-serve is not supported with -relation: the snapshot does not score kept blocks")
    serve_prune = a.get("serve_prune")
    if "serve_prune" in a:
        if "serve" not in a:
            raise ValueError("-serve_prune needs -serve (bf16 | int8)")
        if serve_prune not in ("dead", "seen"):
            raise ValueError("-serve_prune knows dead and seen, not '%s'" % serve_prune)
        if serve_prune == "seen" and implicit:
            raise ValueError("-serve_prune seen is not supported with -interactions: the training rows are two files (use dead)")
    if "save_snapshot" in a:
        if "serve" not in a:
            raise ValueError("-save_snapshot needs -serve (bf16 | int8): it writes the frozen copy")
        if not a["save_snapshot"]:
            raise ValueError("-save_snapshot needs a filename")
    if "train_weights" in a or "test_weights" in a:
        if method != "sgd" or optimizer not in ("adagrad", "ftrl"):
            raise ValueError("-train_weights / -test_weights belong to -method sgd with -optimizer adagrad or ftrl: -method %s%s has no "
                             "weighted form" % (method, " -optimizer " + optimizer if method in ("sgd", "bpr") else ""))
        if not a.get("train_weights"):
            raise ValueError("-test_weights needs -train_weights" if "train_weights" not in a else "-train_weights needs a filename")
        if "test_weights" in a and not a["test_weights"]:
            raise ValueError("-test_weights needs a filename")
    if any(f in a for f in ("save_checkpoint", "load_checkpoint", "checkpoint_dense")):
        if method not in ("sgd", "bpr"):
            raise ValueError("-save_checkpoint / -load_checkpoint belong to -method sgd and -method bpr: -method %s has no checkpoint" % method)
        for f in ("save_checkpoint", "load_checkpoint"):
            if f in a and not a[f]:
                raise ValueError("-%s needs a filename" % f)
        if "load_checkpoint" in a and "load_model" in a:
            raise ValueError("-load_checkpoint replaces -load_model: give one of them")
        if a.get("checkpoint_dense", "0") not in ("0", "1"):
            raise ValueError("-checkpoint_dense takes 0 or 1")
        if "checkpoint_dense" in a and "save_checkpoint" not in a:
            raise ValueError("-checkpoint_dense needs -save_checkpoint")
    metrics = tuple(split_list(a.get("metrics", "")))
    if "metrics" in a:
        for m in metrics:
            if m == L.WEIGHTED_METRIC:
                if not a.get("train_weights"):
                    raise ValueError("-metrics wlogloss needs -train_weights")
            elif m not in L.EXTRA_METRICS:
                raise ValueError("-metrics knows auc and logloss, not '%s'" % m)
        if method == "bpr" or (method == "mcmc" and not dev_avg):
            raise ValueError("-metrics is not supported with -method %s" % method +
                             (": its prediction averages the draws, no single model scores it" if method == "mcmc" else
                              ": the pairwise learner reports its own accuracy and loss"))
        if a["task"] != "c":
            raise ValueError("-metrics needs -task c: AUC and log loss are classification metrics")
    if "test_queries" in a or "train_queries" in a:
        if method in ("mcmc", "bpr"):
            raise ValueError("-test_queries / -train_queries are not supported with -method %s" % method +
                             (": its prediction averages the draws, no single model scores it" if method == "mcmc" else
                              ": the pairwise learner reports its own accuracy and loss"))
        if a["task"] != "c":
            raise ValueError("-test_queries / -train_queries need -task c: the per-query AUC is a classification metric")
        if dev_avg:
            raise ValueError("-test_queries / -train_queries are not supported with -device_average 1")
        if not a.get("test_queries"):
            raise ValueError("-train_queries needs -test_queries" if "test_queries" not in a else "-test_queries needs a filename")
        if "train_queries" in a and not a["train_queries"]:
            raise ValueError("-train_queries needs a filename")
    rank_at = ()
    if "rank_at" in a:
        if method in ("mcmc", "bpr"):
            raise ValueError("-rank_at is not supported with -method %s" % method +
                             (": its prediction averages the draws, no single model scores it" if method == "mcmc" else
                              ": the pairwise learner reports its own accuracy and loss"))
        if a["task"] != "c":
            raise ValueError("-rank_at needs -task c: a row is relevant by the sign of its classification target")
        if not a.get("test_queries"):
            raise ValueError("-rank_at needs -test_queries")
        try:
            rank_at = tuple(int(x) for x in split_list(a["rank_at"]))
        except ValueError:
            raise ValueError("-rank_at needs integers: 'K1,K2,...' (got '%s')" % a["rank_at"])
        if not 1 <= len(rank_at) <= L.RANK_MAX_CUTOFFS:
            raise ValueError("-rank_at takes 1 .. %d cutoffs (got %d)" % (L.RANK_MAX_CUTOFFS, len(rank_at)))
        if any(not 1 <= k <= L.RANK_MAX_K for k in rank_at):
            raise ValueError("-rank_at: a cutoff is an integer in 1 .. %d" % L.RANK_MAX_K)
        if any(y <= x for x, y in zip(rank_at, rank_at[1:])):
            raise ValueError("-rank_at: the cutoffs must be strictly ascending")

    print("Loading train...\t")
    train = L.Data(*D.load(a["train"]))
    print("num_rows=%d\tnum_values=%d\tnum_features=%d\tmin_target=%g\tmax_target=%g" %
          (train.num_cases, len(train.entries), train.num_feature, train.min_target, train.max_target))
    print("Loading test... \t")
    test = L.Data(*D.load(a["test"]))
    print("num_rows=%d\tnum_values=%d\tnum_features=%d\tmin_target=%g\tmax_target=%g" %
          (test.num_cases, len(test.entries), test.num_feature, test.min_target, test.max_target))

    test_queries = read_queries(a["test_queries"], test.num_cases) if a.get("test_queries") else None
    train_queries = read_queries(a["train_queries"], train.num_cases) if a.get("train_queries") else None
    train_weights = read_weights(a["train_weights"], train.num_cases) if a.get("train_weights") else None
    test_weights = read_weights(a["test_weights"], test.num_cases) if a.get("test_weights") else None

    validation = None
    if method == "sgda":                                                             # libfm.cpp:173-194
        if "validation" not in a:
            raise ValueError("sgda needs -validation")
        print("Loading validation set...\t")
        validation = L.Data(*D.load(a["validation"]))

    cand = None
    if implicit:                             # the candidate rows are training data here: their features are model features
        print("Loading candidates...\t")
        cand = L.Data(*D.load(a["candidates"]))
        print("num_rows=%d\tnum_values=%d\tnum_features=%d" % (cand.num_cases, len(cand.entries), cand.num_feature))

    fm = L.FMModel()
    fm.num_attribute = max(train.num_feature, test.num_feature)                      # libfm.cpp:203-206
    if cand is not None:
        fm.num_attribute = max(fm.num_attribute, cand.num_feature)
    if validation is not None:
        fm.num_attribute = max(fm.num_attribute, validation.num_feature)
    # (1.2) relations (libfm.cpp:172-196): block attributes follow the main attributes (:213-216)
    relations = []
    if a.get("relation"):
        if method not in ("als", "mcmc"):
            raise ValueError("relations are not supported with SGD")            # fm_learn_sgd.h:61-63
        rel_names = split_list(a["relation"])
        print("#relations: %d" % len(rel_names))
        for name in rel_names:
            r = D.read_relation(name)
            print("num_cases=%d\tnum_values=%d\tnum_features=%d" % (r.num_cases, len(r.entries), r.num_feature))
            train.add_relation(r, D.read_row_mapping(name + ".train", train.num_cases), fm.num_attribute)
            test.add_relation(r, D.read_row_mapping(name + ".test", test.num_cases), fm.num_attribute)
            relations.append(r)
            fm.num_attribute += r.num_feature
    num_main_attribute = fm.num_attribute - sum(r.num_feature for r in relations)

    fm.k0, fm.k1, fm.num_factor = dim[0] != 0, dim[1] != 0, dim[2]
    fm.init_stdev = init_stdev
    R.srand(seed)                                                                     # libfm.cpp:115-116
    fm.w0 = 0.0
    fm.w = np.zeros(fm.num_attribute)
    fm.v = R.init_v(fm.num_factor, fm.num_attribute, fm.init_mean, fm.init_stdev)    # fm_model.h:96
    if "load_model" in a:
        print("Reading FM model... \t")
        if not fm.load_model(a["load_model"]):
            print("WARNING: malformed model file. Nothing will be loaded.")
            fm.w0, fm.w[:] = 0.0, 0.0

    # (1.3) meta data: attribute -> group, one id per line (DataMetaInfo::loadGroupsFromFile, Data.h:85-97;
    # DVector::load reads num_attribute values, missing ones stay 0, matrix.h:360-371)
    groups, num_groups = None, 1
    if a.get("meta") or any(r.groups is not None for r in relations):
        print("Loading meta data...\t")
        groups = np.zeros(fm.num_attribute, dtype=np.uint32)
        if a.get("meta"):
            with open(a["meta"]) as f:
                vals = f.read().split()[:num_main_attribute]
            groups[:len(vals)] = [int(x) for x in vals]
        num_groups = int(groups[:num_main_attribute].max()) + 1 if num_main_attribute else 1
        at = num_main_attribute
        for r in relations:                                                          # the joined table, :217-240
            rg = r.groups if r.groups is not None else np.zeros(r.num_feature, dtype=np.uint32)
            groups[at:at + r.num_feature] = num_groups + rg
            num_groups += int(rg.max()) + 1 if r.num_feature else 1
            at += r.num_feature
        print("#attr=%d\t#groups=%d" % (fm.num_attribute, num_groups))

    task = a["task"]
    if task not in ("r", "c"):
        raise ValueError("unknown task")
    min_t, max_t = train.min_target, train.max_target                                # libfm.cpp:295-296
    if task == "c":                                                                  # libfm.cpp:302-306
        train.target[:] = np.where(train.target <= 0.0, -1.0, 1.0)
        test.target[:] = np.where(test.target <= 0.0, -1.0, 1.0)
    reg = [float(x) for x in split_list(a.get("regular", ""))]
    if len(reg) == 0:
        reg = [0.0, 0.0, 0.0]
    elif len(reg) == 1:
        reg = [reg[0]] * 3
    group_reg = None
    if len(reg) == 1 + 2 * num_groups and len(reg) != 3 and method in ("als", "mcmc"):      # libfm.cpp:353-363
        group_reg = (np.array(reg[1:1 + num_groups]), np.array(reg[1 + num_groups:]))
        reg = [reg[0], 0.0, 0.0]
    elif len(reg) != 3:
        raise ValueError("-regular needs 0, 1, 3 or 1+2*#groups values")
    fm.reg0, fm.regw, fm.regv = reg
    num_iter = int(a.get("iter", "100"))

    if method == "bpr":
        l = L.FMLearnPairSGD() if optimizer == "sgd" else L.FMLearnPairAdaptive()
        lrs = [float(x) for x in split_list(a.get("learn_rate", ""))]
        if len(lrs) != 1:
            raise ValueError("-learn_rate needs 1 value for bpr")
        l.learn_rate = lrs[0]
        l.mode = a.get("gpu_mode", "sequential" if optimizer == "sgd" else "minibatch")
        l.batch = int(a.get("batch", "0"))
        if optimizer != "sgd":
            l.optimizer = optimizer
            l.init_acc = float(a.get("init_acc", "0"))
            if optimizer == "ftrl":
                l.ftrl_alpha, l.ftrl_beta = float(a.get("ftrl_alpha", "0")), float(a.get("ftrl_beta", "1"))
                l.l1_w, l.l1_v = ftrl_l1
    elif method in ("sgd", "sgda"):
        l = L.FMLearnSGD() if method == "sgd" else L.FMLearnSGDA()
        if method == "sgda":
            l.validation = validation
            l.groups = groups
            if task == "c":
                l.validation.target[:] = np.where(l.validation.target <= 0.0, -1.0, 1.0)
        lrs = [float(x) for x in split_list(a.get("learn_rate", ""))]
        if len(lrs) not in (1, 3):
            raise ValueError("-learn_rate needs 1 or 3 values")                     # the reference asserts (libfm.cpp:391-392)
        l.learn_rate = lrs[0] if len(lrs) == 1 else 0.0                              # 3 values: scalar rate 0 (libfm.cpp:396-401)
        l.mode = a.get("gpu_mode", "minibatch")
        l.batch = int(a.get("batch", "0"))
        l.w0_chunk = int(a.get("w0_chunk", "0"))
        if optimizer != "sgd":
            l.optimizer = optimizer
            l.init_acc = float(a.get("init_acc", "0"))
            if optimizer == "ftrl":
                l.ftrl_alpha, l.ftrl_beta = float(a.get("ftrl_alpha", "0")), float(a.get("ftrl_beta", "1"))
                l.l1_w, l.l1_v = ftrl_l1
    else:
        if method == "als":
            l = L.FMLearnALS()
        else:
            l = L.FMLearnMCMC()
            l.seed = seed
        fm.w = R.init_w_normal(fm.num_attribute, fm.init_mean, fm.init_stdev)        # libfm.cpp:283
        l.w_lambda, l.v_lambda = fm.regw, fm.regv
        l.groups = groups
        if group_reg is not None:
            l.w_lambda, l.v_lambda = group_reg
    l.fm, l.num_iter, l.task = fm, num_iter, (0 if task == "r" else 1)
    l.min_target, l.max_target = min_t, max_t
    l.device = int(a.get("device", "-1"))
    if devices is not None:
        l.devices = devices
    if metrics:
        l.extra_metrics = metrics
    if dev_avg:
        l.device_average = True
    if "load_checkpoint" in a:
        l.load_checkpoint(a["load_checkpoint"])
    l.init()
    if "load_checkpoint" in a:
        optimizer = l.optimizer                                 # (a file with a session names it)
        print(checkpoint_line("load", L.capi.checkpoint_info(a["load_checkpoint"])), file=sys.stderr)
    if test_queries is not None:
        l.set_queries(test, test_queries)
    if train_queries is not None:
        l.set_queries(train, train_queries)
    if rank_at:
        l.rank_cutoffs = rank_at
    if train_weights is not None:
        l.set_weights(train, train_weights)
    if test_weights is not None:
        l.set_weights(test, test_weights)
    if implicit:
        print("Loading interactions...\t")
        inter = read_interactions(a["interactions"], train.num_cases, cand.num_cases)
        test_inter = read_interactions(a["test_interactions"], test.num_cases, cand.num_cases) if a.get("test_interactions") else None
        n_neg = int(a.get("neg", "1"))
        if n_neg < 1:
            raise ValueError("-neg needs at least 1")
        neg_draws = int(a.get("neg_draws", "1"))
        if not 1 <= neg_draws <= 16:
            raise ValueError("-neg_draws needs 1 .. 16")
        print("interactions=%d\ttest_interactions=%d\tneg=%d\tneg_draws=%d" %
              (len(inter[0]), 0 if test_inter is None else len(test_inter[0]), n_neg, neg_draws))
        # -train and -test naming one file are the same query rows: a query's train interactions are then excluded from the test
        # pairs' negatives too (learn_implicit keeps the test interactions on a copy of the rows)
        same_rows = os.path.realpath(a["train"]) == os.path.realpath(a["test"])
        l.learn_implicit(train, cand, inter, test_inter, n_neg=n_neg, seed=seed, test_queries=None if same_rows else test,
                         neg_draws=neg_draws)
    elif method == "bpr":
        print("Loading pairs...\t")
        train_pairs = read_pairs(a["train_pairs"], train.num_cases)
        test_pairs = read_pairs(a["test_pairs"], test.num_cases)
        print("train_pairs=%d\ttest_pairs=%d" % (len(train_pairs[0]), len(test_pairs[0])))
        l.learn(train, train_pairs, test, test_pairs)
    else:
        l.learn(train, test)
    if implicit:
        e_tr, e_te = l.evaluate_implicit()
        print("Final\tTrain=%g\tTest=%g" % (e_tr.accuracy, e_te.accuracy if e_te is not None else float("nan")))
    elif method == "bpr":
        print("Final\tTrain=%g\tTest=%g" % (l.evaluate_pairs(train), l.evaluate_pairs(test)))
    if method in ("sgd", "sgda"):
        print("Final\tTrain=%g\tTest=%g" % (l.evaluate(train), l.evaluate(test)))   # libfm.cpp:418-420
    if optimizer == "ftrl":
        sp = l.sparsity()
        print("sparsity\tfeatures=%d\tw_zero=%d\tv_coords=%d\tv_zero=%d\tv_zero_rows=%d\tdead_features=%d" %
              (sp.features, sp.w_zero, sp.v_coords, sp.v_zero, sp.v_zero_rows, sp.dead_features), file=sys.stderr)
    scorer = l                               # what -out and -topk read: the learner, or with -serve the frozen copy
    if serve:
        scorer = l.compact(serve, prune=serve_prune) if serve_prune else l.compact(serve)
        ci = scorer.info
        line = "compact\tformat=%s\tbytes=%d\tbytes_fp32=%d\tmax_abs_err=%g\tnonfinite=%d\tTest(fp32)=%g\tTest(%s)=%g" % (
            serve, ci.bytes_compact, ci.bytes_params, ci.max_abs_err, ci.nonfinite, l.evaluate(test), serve, scorer.evaluate(test))
        if serve_prune:
            pi = scorer.prune_info
            line += "\tprune=%s\tkept=%d\tdropped_dead=%d\tdropped_unseen=%d\tbytes_directory=%d\tbytes_rows=%d" % (
                serve_prune, pi.kept, pi.dropped_dead, pi.dropped_unseen, pi.bytes_directory, pi.bytes_rows)
        if metrics and not dev_avg:
            ex32, ex16 = l.evaluate_ex(test), scorer.evaluate_ex(test)
            line += "".join("\t%s(fp32)=%g\t%s(%s)=%g" % (m, getattr(ex32, m), m, serve, getattr(ex16, m)) for m in metrics if m in L.EXTRA_METRICS)
        print(line, file=sys.stderr)
        if "save_snapshot" in a:
            print(snapshot_line("save", scorer.save(a["save_snapshot"])), file=sys.stderr)
    if "rlog" in a and a["rlog"]:
        with open(a["rlog"], "w") as f:                                              # rlog.h:60-103: TSV with a header
            keys = sorted(l.log[0].keys()) if l.log else []
            f.write("\t".join(keys) + "\n")
            for row in l.log:
                f.write("\t".join("%g" % row[k] for k in keys) + "\n")
    if "out" in a and a["out"]:
        pred = scorer.predict_raw(test) if method == "bpr" else scorer.predict(test)      # bpr: raw y per test row (a score)
        with open(a["out"], "w") as f:                                               # DVector::save, matrix.h:332-342
            f.write("".join("%g\n" % p for p in pred))
    if "save_model" in a and a["save_model"]:
        print("Writing FM model to " + a["save_model"])
        fm.save_model(a["save_model"])
    if "save_checkpoint" in a:
        print(checkpoint_line("save", l.save_checkpoint(a["save_checkpoint"], dense=a.get("checkpoint_dense", "0") == "1")), file=sys.stderr)
    if want_topk:
        topk = int(a["topk"])
        if cand is None:
            cand = L.Data(*D.load(a["candidates"]))
        queries = L.Data(*D.load(a["queries"])) if a.get("queries") else test
        exclude = read_exclude(a["exclude"], queries.num_cases, cand.num_cases) if a.get("exclude") else None
        idx, score = scorer.recommend(queries, cand, topk, exclude)
        print("Top-K\tqueries=%d\tcandidates=%d\tK=%d" % (queries.num_cases, cand.num_cases, topk))
        if a.get("topk_out"):
            write_topk(a["topk_out"], idx, score)
    if scorer is not l:
        scorer.close()
    l.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
