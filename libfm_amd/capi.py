"""ctypes binding of the C-ABI in include/fmx.h (libfm_amd/libfmx.so).

This is the only way Python reaches the HIP kernels; there is no Python/CPU fallback: if the shared library is
missing or no HIP device is present, the calls raise."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMX_LIB", os.path.join(HERE, "libfmx.so"))   # FMX_LIB: experiment builds only

FMX_OK = 0
TASK_REGRESSION, TASK_CLASSIFICATION = 0, 1
SGD_SEQUENTIAL, SGD_MINIBATCH, SGD_HOGWILD = 0, 1, 2
APPLY_DEFAULT, APPLY_ATOMIC, APPLY_STORE, APPLY_SEGMENTED, APPLY_FUSED = 0, 1, 2, 3, 4
FLAG_TIME_MAIN_KERNEL = 1
FLAG_BIAS_LAG = 2
FLAG_PIPELINE = 4
FLAG_REJECT_UNSTABLE = 8
FLAG_EVENT_SYNC = 16
FLAG_KEEP_WSIDE = 32
EVAL_WSIDE = 1
LINK_LOGISTIC, LINK_PROBIT = 0, 1   # FMX_LINK_*: fmx_eval_opts::link
STAT_BATCH_CUT, STAT_UNSTABLE = 1, 2
STAT_WARN = 3   # FMX_STAT_WARN_MASK: the two bits that say something about the RULE; the bits above are how the epoch ran (include/fmx.h, ABI 7, 9)
STAT_SCAN_PIT, STAT_SCAN_SERIAL, STAT_SCAN_FALLBACK, STAT_EVENT_SYNC, STAT_HANDOFF_TIMEOUT, STAT_SEQ_RUNS, STAT_SMALL_ONE = 4, 8, 16, 32, 64, 256, 512
# FMX_SGD_SEQUENTIAL: which kernels the epoch ran (ABI 9)
STAT_SEQ_ENTRIES, STAT_SEQ_WG, STAT_SEQ_ROWS, STAT_RUN_ONE, STAT_RUN_TWO, STAT_RUN_THREE = 1024, 2048, 4096, 8192, 16384, 32768
STAT_WEIGHTED = 65536   # FMX_STAT_WEIGHTED: an fmx_adapt / fmx_ftrl epoch on a slot with row weights (set_row_weights)
STAT_WSTREAM = 131072   # FMX_STAT_WSTREAM: a one-pass minibatch epoch read the once-only features' linear weights from the slot's packed stream
SYNTH_UNIFORM, SYNTH_CRITEO = 0, 1
BLOCKS_EXPAND, BLOCKS_KEEP = 0, 1
COMM_ID_BYTES = 128
MAX_SLOTS = 8

ENTRY_DTYPE = np.dtype([("id", np.uint32), ("value", np.float32)])   # sparse_entry<float>, fmatrix.h:34-37


class FmxError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("libfmx error %d: %s" % (code, text))
        self.code = code
        self.text = text


class Config(C.Structure):
    _fields_ = [("num_attribute", C.c_uint64), ("num_factor", C.c_int32), ("k0", C.c_int32), ("k1", C.c_int32),
                ("task", C.c_int32), ("reg0", C.c_double), ("regw", C.c_double), ("regv", C.c_double),
                ("learn_rate", C.c_double), ("min_target", C.c_double), ("max_target", C.c_double),
                ("device", C.c_int32), ("shard_rank", C.c_int32), ("shard_world", C.c_int32), ("shard_hash", C.c_int32),
                ("place_candidates", C.c_int32), ("als_split_min", C.c_uint32), ("exchange_runs", C.c_uint32), ("exchange_algo", C.c_uint32)]


ALS_SPLIT_NEVER = 0xFFFFFFFF
ALS_SPLIT_MIN = 0           # default of Handle(als_split_min=None): 0 = the library's choice (tests set 1 / ALS_SPLIT_NEVER to force a form)


class SgdOpts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("apply", C.c_int32), ("batch", C.c_uint32), ("w0_chunk", C.c_uint32),
                ("flags", C.c_uint32), ("bias_lag", C.c_uint32)]


class EpochStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("batches", C.c_uint64), ("device_seconds", C.c_double),
                ("main_kernel_seconds", C.c_double), ("main_kernel_launches", C.c_uint64),
                ("max_feature_count", C.c_uint32), ("batch_used", C.c_uint32), ("deferred_features", C.c_uint64),
                ("collision_mass", C.c_double), ("batch_gain", C.c_double), ("status", C.c_uint32), ("w0_chunk_used", C.c_uint32),
                ("setup_seconds", C.c_double), ("phase_seconds", C.c_double * 4)]


ADAPT_ADAGRAD = 1   # FMX_ADAPT_ADAGRAD: fmx_adapt_opts::rule


class AdaptOpts(C.Structure):
    _fields_ = [("rule", C.c_uint32), ("flags", C.c_uint32), ("init_acc", C.c_double), ("learn_rate", C.c_double)]


class FtrlOpts(C.Structure):                       # fmx_ftrl_opts
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32), ("alpha", C.c_double), ("beta", C.c_double),
                ("l1_w", C.c_double), ("l1_v", C.c_double), ("l2_w", C.c_double), ("l2_v", C.c_double), ("init_acc", C.c_double)]


class Sparsity(C.Structure):                       # fmx_sparsity
    _fields_ = [("features", C.c_uint64), ("w_zero", C.c_uint64), ("v_coords", C.c_uint64), ("v_zero", C.c_uint64),
                ("v_zero_rows", C.c_uint64), ("dead_features", C.c_uint64)]


COMPACT_BF16 = 1    # FMX_COMPACT_BF16: fmx_compact_opts::format
COMPACT_INT8 = 3    # FMX_COMPACT_INT8 (2 is not assigned)


class CompactOpts(C.Structure):                    # fmx_compact_opts
    _fields_ = [("format", C.c_uint32), ("flags", C.c_uint32)]


class CompactInfo(C.Structure):                    # fmx_compact_info
    _fields_ = [("features", C.c_uint64), ("bytes_compact", C.c_uint64), ("bytes_params", C.c_uint64), ("nonfinite", C.c_uint64),
                ("max_abs_err", C.c_double), ("sum_sq_err", C.c_double)]


PRUNE_DEAD, PRUNE_SEEN = 1, 2   # FMX_PRUNE_*: fmx_compact_prune_opts::flags
SLOT_NONE = 0xFFFFFFFF          # fmx_compact_slot_of: a dropped id


class CompactPruneOpts(C.Structure):               # fmx_compact_prune_opts
    _fields_ = [("format", C.c_uint32), ("flags", C.c_uint32), ("keep_slot", C.c_int32), ("reserved", C.c_uint32)]


class CompactPruneInfo(C.Structure):               # fmx_compact_prune_info
    _fields_ = [("features", C.c_uint64), ("kept", C.c_uint64), ("dropped_dead", C.c_uint64), ("dropped_unseen", C.c_uint64),
                ("bytes_directory", C.c_uint64), ("bytes_rows", C.c_uint64)]


CKPT_DENSE_STATE, CKPT_MODEL_ONLY = 1, 2   # FMX_CKPT_*: fmx_ckpt_opts::flags
CKPT_SESSIONS = ("none", "adagrad", "ftrl")   # fmx_ckpt_info::session


class CkptOpts(C.Structure):                       # fmx_ckpt_opts
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32)]


class CkptInfo(C.Structure):                       # fmx_ckpt_info
    _fields_ = [("version", C.c_uint32), ("session", C.c_uint32), ("num_attribute", C.c_uint64), ("num_factor", C.c_uint32),
                ("k0", C.c_uint32), ("k1", C.c_uint32), ("flags", C.c_uint32), ("state_rows", C.c_uint64), ("bytes", C.c_uint64),
                ("seconds", C.c_double), ("device_seconds", C.c_double)]


class SnapInfo(C.Structure):                       # fmx_snap_info
    _fields_ = [("version", C.c_uint32), ("format", C.c_uint32), ("num_attribute", C.c_uint64), ("num_factor", C.c_uint32),
                ("k0", C.c_uint32), ("k1", C.c_uint32), ("task", C.c_int32), ("min_target", C.c_double), ("max_target", C.c_double),
                ("pruned", C.c_uint32), ("row_bytes", C.c_uint32), ("kept", C.c_uint64), ("rows", C.c_uint64),
                ("nonfinite", C.c_uint64), ("max_abs_err", C.c_double), ("sum_sq_err", C.c_double),
                ("dropped_dead", C.c_uint64), ("dropped_unseen", C.c_uint64), ("bytes", C.c_uint64), ("bytes_compact", C.c_uint64),
                ("seconds", C.c_double), ("device_seconds", C.c_double)]


class BatchInfo(C.Structure):
    _fields_ = [("collision_mass", C.c_double), ("batch_gain", C.c_double), ("batch", C.c_uint32), ("status", C.c_uint32)]


class PlaceInfo(C.Structure):
    _fields_ = [("method", C.c_int32), ("chunks", C.c_uint32), ("per_class", C.c_uint32 * 2), ("pool", C.c_uint32),
                ("classes_seen", C.c_uint32), ("seconds", C.c_double)]


class Eval(C.Structure):
    _fields_ = [("rmse", C.c_double), ("mae", C.c_double), ("accuracy", C.c_double),
                ("device_seconds", C.c_double), ("rows", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class EvalOpts(C.Structure):
    _fields_ = [("link", C.c_uint32), ("flags", C.c_uint32)]


class EvalEx(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("nan_rows", C.c_uint64), ("pos", C.c_uint64), ("neg", C.c_uint64), ("correct", C.c_uint64),
                ("auc_num2", C.c_uint64), ("auc", C.c_double), ("logloss", C.c_double), ("rmse", C.c_double), ("mae", C.c_double),
                ("accuracy", C.c_double), ("device_seconds", C.c_double), ("rank_seconds", C.c_double),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class EvalWeighted(C.Structure):                   # fmx_eval_weighted
    _fields_ = [("rows", C.c_uint64), ("nan_rows", C.c_uint64), ("weight_sum", C.c_double), ("pos_weight", C.c_double),
                ("neg_weight", C.c_double), ("correct_weight", C.c_double), ("loss_sum", C.c_double), ("sq_sum", C.c_double),
                ("abs_sum", C.c_double), ("logloss", C.c_double), ("rmse", C.c_double), ("mae", C.c_double), ("accuracy", C.c_double),
                ("device_seconds", C.c_double)]


class EvalQuery(C.Structure):
    _fields_ = [("pooled", EvalEx), ("queries", C.c_uint64), ("valid_queries", C.c_uint64), ("one_class_queries", C.c_uint64),
                ("empty_queries", C.c_uint64), ("valid_rows", C.c_uint64), ("num2_within", C.c_uint64), ("den2_within", C.c_uint64),
                ("auc_within", C.c_double), ("gauc", C.c_double), ("auc_macro", C.c_double),
                ("device_seconds", C.c_double), ("rank_seconds", C.c_double)]


RANK_MAX_CUTOFFS, RANK_MAX_K = 4, 65536             # FMX_RANK_MAX_CUTOFFS, FMX_RANK_MAX_K


class RankOpts(C.Structure):                       # fmx_rank_opts
    _fields_ = [("link", C.c_uint32), ("flags", C.c_uint32), ("n_cutoffs", C.c_uint32), ("k", C.c_uint32 * RANK_MAX_CUTOFFS),
                ("reserved", C.c_uint32)]


class RankAt(C.Structure):                         # fmx_rank_at
    _fields_ = [("k", C.c_uint32), ("reserved", C.c_uint32), ("tied_queries", C.c_uint64), ("hits", C.c_double), ("ndcg", C.c_double),
                ("recall", C.c_double), ("precision", C.c_double)]


class EvalRank(C.Structure):                       # fmx_eval_rank
    _fields_ = [("by_query", EvalQuery), ("relevant_queries", C.c_uint64), ("n_cutoffs", C.c_uint32), ("reserved", C.c_uint32),
                ("at", RankAt * RANK_MAX_CUTOFFS), ("device_seconds", C.c_double), ("topk_seconds", C.c_double)]


POST_THIS, POST_ALL, POST_LATE = 0, 1, 2   # FMX_POST_*: the last draw, the mean over all draws, the mean over the draws from burn_in on


class PostOpts(C.Structure):
    _fields_ = [("burn_in", C.c_uint32), ("eval_rows", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class PostMetric(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("nan_rows", C.c_uint64), ("correct", C.c_uint64), ("rmse", C.c_double), ("mae", C.c_double),
                ("accuracy", C.c_double), ("ll_ref", C.c_double)]


class PostStats(C.Structure):
    _fields_ = [("draws", C.c_uint64), ("late_draws", C.c_uint64), ("m", PostMetric * 3), ("device_seconds", C.c_double)]


class PairOpts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("batch", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class PairEval(C.Structure):
    _fields_ = [("accuracy", C.c_double), ("loss", C.c_double), ("device_seconds", C.c_double), ("pairs", C.c_uint64)]


PAIR_DEFAULT_BATCH = 1024   # FMX_PAIR_DEFAULT_BATCH: fmx_pair_opts::batch = 0


class PairNegOpts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("batch", C.c_uint32), ("n_neg", C.c_uint32), ("flags", C.c_uint32),
                ("seed", C.c_uint64), ("epoch", C.c_uint64)]


NEG_ATTEMPTS = 16           # FMX_NEG_ATTEMPTS: draws per negative before one is forced
NEG_HARDEST = 2             # FMX_NEG_HARDEST: the best-scoring of the first M accepted draws (FMX_NEG_DRAWS(M) = M << 8)


def neg_flags(draws):
    """fmx_pairneg_opts::flags of `draws` accepted draws per negative: 1 = the uniform sampler (0), M > 1 = hardest of M"""
    draws = int(draws)
    return 0 if draws == 1 else NEG_HARDEST | (draws << 8)


class TopkOpts(C.Structure):
    _fields_ = [("topk", C.c_uint32), ("flags", C.c_uint32), ("query_row0", C.c_uint64), ("n_query", C.c_uint32),
                ("reserved", C.c_uint32), ("exclude_ptr", C.c_void_p), ("exclude_idx", C.c_void_p)]


class TopkStats(C.Structure):
    _fields_ = [("device_seconds", C.c_double), ("score_seconds", C.c_double), ("scores", C.c_uint64), ("splits", C.c_uint32),
                ("reserved", C.c_uint32)]


TOPK_MAX = 1024             # FMX_TOPK_MAX: results per query, at most
TOPK_NONE = 0xFFFFFFFF      # index of a padding entry (its score is -inf)


class Relation(C.Structure):
    _fields_ = [("entries", C.c_void_p), ("row_ptr", C.c_void_p), ("n_rows", C.c_uint32), ("reserved", C.c_uint32),
                ("nnz", C.c_uint64), ("data_row_to_relation_row", C.c_void_p), ("attr_offset", C.c_uint64)]


class HostRows(C.Structure):
    _fields_ = [("entries", C.c_void_p), ("row_ptr", C.c_void_p), ("target", C.c_void_p), ("n_rows", C.c_uint32),
                ("num_feature", C.c_uint32), ("nnz", C.c_uint64), ("min_target", C.c_float), ("max_target", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class AlsOpts(C.Structure):
    _fields_ = [("alpha", C.c_double), ("w_mu", C.c_double), ("w_lambda", C.c_double), ("v_mu", C.c_double),
                ("v_lambda", C.c_double), ("do_sample", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64),
                ("v_mu_f", C.c_void_p), ("v_lambda_f", C.c_void_p),
                ("num_groups", C.c_uint32), ("reserved2", C.c_uint32), ("w_mu_g", C.c_void_p), ("w_lambda_g", C.c_void_p),
                ("v_mu_gf", C.c_void_p), ("v_lambda_gf", C.c_void_p)]


class AlsStats(C.Structure):
    _fields_ = [("train_metric", C.c_double), ("device_seconds", C.c_double), ("levels", C.c_uint32),
                ("reserved", C.c_uint32), ("sum_e_sqr", C.c_double)]


class Info(C.Structure):
    _fields_ = [("n_local", C.c_uint64), ("k_padded", C.c_int32), ("device", C.c_int32),
                ("bytes_params", C.c_uint64), ("device_name", C.c_char * 64), ("arch", C.c_char * 32)]


# every symbol include/fmx.h declares: (name, restype, argtypes)
H = C.c_void_p
SYMBOLS = [
    ("fmx_create", C.c_int, [C.POINTER(Config), C.POINTER(H)]),
    ("fmx_destroy", C.c_int, [H]),
    ("fmx_last_error", C.c_char_p, [H]),
    ("fmx_abi_version", C.c_int, []),
    ("fmx_default_w0_chunk", C.c_uint32, [C.c_double, C.c_int]),
    ("fmx_release_cached_memory", C.c_int, []),
    ("fmx_device_count", C.c_int, []),
    ("fmx_set_params", C.c_int, [H, C.c_double, C.c_void_p, C.c_void_p]),
    ("fmx_get_params", C.c_int, [H, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    ("fmx_init_params", C.c_int, [H, C.c_double, C.c_double, C.c_uint64]),
    ("fmx_get_param_rows", C.c_int, [H, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("fmx_get_w0", C.c_int, [H, C.POINTER(C.c_double)]),
    ("fmx_save_model", C.c_int, [H, C.c_char_p]),
    ("fmx_load_model", C.c_int, [H, C.c_char_p]),
    ("fmx_set_groups", C.c_int, [H, C.c_void_p, C.c_uint32]),
    ("fmx_upload_rows", C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64]),
    ("fmx_upload_block_rows", C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                        C.POINTER(Relation), C.c_uint32]),
    ("fmx_upload_block_rows_ex", C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                           C.POINTER(Relation), C.c_uint32, C.c_uint32]),
    ("fmx_read_libsvm", C.c_int, [C.c_char_p, C.POINTER(HostRows), C.c_char_p, C.c_size_t]),
    ("fmx_read_binary", C.c_int, [C.c_char_p, C.POINTER(HostRows), C.c_char_p, C.c_size_t]),
    ("fmx_free_host_rows", None, [C.POINTER(HostRows)]),
    ("fmx_synth_rows", C.c_int, [H, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]),
    ("fmx_synth_rows_ex", C.c_int, [H, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("fmx_free_rows", C.c_int, [H, C.c_int]),
    ("fmx_rows_info", C.c_int, [H, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("fmx_download_rows", C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("fmx_wtrain_info", C.c_int, [H, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    ("fmx_predict", C.c_int, [H, C.c_int, C.c_void_p]),
    ("fmx_evaluate", C.c_int, [H, C.c_int, C.POINTER(Eval)]),
    ("fmx_evaluate_ex", C.c_int, [H, C.c_int, C.POINTER(EvalOpts), C.POINTER(EvalEx)]),
    ("fmx_set_row_queries", C.c_int, [H, C.c_int, C.c_void_p, C.c_uint32]),
    ("fmx_set_row_weights", C.c_int, [H, C.c_int, C.c_void_p]),
    ("fmx_get_row_weights", C.c_int, [H, C.c_int, C.c_void_p]),
    ("fmx_evaluate_weighted", C.c_int, [H, C.c_int, C.POINTER(EvalOpts), C.POINTER(EvalWeighted)]),
    ("fmx_evaluate_by_query", C.c_int, [H, C.c_int, C.POINTER(EvalOpts), C.POINTER(EvalQuery), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("fmx_rank_discounts", C.c_int, [C.c_uint32, C.c_void_p]),
    ("fmx_evaluate_rank", C.c_int, [H, C.c_int, C.POINTER(RankOpts), C.POINTER(EvalRank), C.c_void_p, C.c_void_p]),
    ("fmx_post_begin", C.c_int, [H, C.c_int, C.POINTER(PostOpts)]),
    ("fmx_post_accumulate", C.c_int, [H, C.c_int, C.POINTER(PostStats)]),
    ("fmx_post_evaluate_ex", C.c_int, [H, C.c_int, C.c_uint32, C.POINTER(EvalEx)]),
    ("fmx_post_get", C.c_int, [H, C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    ("fmx_post_end", C.c_int, [H, C.c_int]),
    ("fmx_sgd_epoch", C.c_int, [H, C.c_int, C.POINTER(SgdOpts), C.POINTER(EpochStats)]),
    ("fmx_sgd_batch_info", C.c_int, [H, C.c_int, C.POINTER(SgdOpts), C.POINTER(BatchInfo)]),
    ("fmx_get_place_info", C.c_int, [H, C.POINTER(PlaceInfo)]),
    ("fmx_batch_rule", C.c_int, [C.c_int32, C.c_double, C.c_double, C.c_uint32, C.POINTER(BatchInfo)]),
    ("fmx_place_layout", C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("fmx_partial_floats", C.c_int, [H, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("fmx_sgd_partial", C.c_int, [H, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("fmx_sgd_finish", C.c_int, [H, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(SgdOpts), C.c_void_p]),
    ("fmx_predict_finish", C.c_int, [H, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("fmx_shard_place", C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("fmx_shard_global", C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]),
    ("fmx_comm_unique_id", C.c_int, [C.c_void_p]),
    ("fmx_comm_init_rank", C.c_int, [H, C.c_void_p, C.c_int, C.c_int]),
    ("fmx_comm_destroy", C.c_int, [H]),
    ("fmx_group_create", C.c_int, [C.POINTER(H), C.c_int, C.POINTER(H)]),
    ("fmx_group_destroy", C.c_int, [H]),
    ("fmx_group_last_error", C.c_char_p, [H]),
    ("fmx_group_set_params", C.c_int, [H, C.c_double, C.c_void_p, C.c_void_p]),
    ("fmx_group_upload_rows", C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64]),
    ("fmx_group_upload_block_rows_ex", C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                                 C.POINTER(Relation), C.c_uint32, C.c_uint32]),
    ("fmx_group_sgd_epoch", C.c_int, [H, C.c_int, C.POINTER(SgdOpts), C.POINTER(EpochStats)]),
    ("fmx_group_predict", C.c_int, [H, C.c_int, C.c_void_p]),
    ("fmx_group_evaluate", C.c_int, [H, C.c_int, C.POINTER(Eval)]),
    ("fmx_group_evaluate_ex", C.c_int, [H, C.c_int, C.POINTER(EvalOpts), C.POINTER(EvalEx)]),
    ("fmx_group_set_row_queries", C.c_int, [H, C.c_int, C.c_void_p, C.c_uint32]),
    ("fmx_group_evaluate_by_query", C.c_int, [H, C.c_int, C.POINTER(EvalOpts), C.POINTER(EvalQuery), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("fmx_group_evaluate_rank", C.c_int, [H, C.c_int, C.POINTER(RankOpts), C.POINTER(EvalRank), C.c_void_p, C.c_void_p]),
    ("fmx_group_post_begin", C.c_int, [H, C.c_int, C.POINTER(PostOpts)]),
    ("fmx_group_post_accumulate", C.c_int, [H, C.c_int, C.POINTER(PostStats)]),
    ("fmx_group_post_evaluate_ex", C.c_int, [H, C.c_int, C.c_uint32, C.POINTER(EvalEx)]),
    ("fmx_group_post_get", C.c_int, [H, C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    ("fmx_group_post_end", C.c_int, [H, C.c_int]),
    ("fmx_group_als_begin", C.c_int, [H, C.c_int]),
    ("fmx_group_als_moments", C.c_int, [H, C.c_void_p]),
    ("fmx_group_als_sweep", C.c_int, [H, C.POINTER(AlsOpts), C.POINTER(AlsStats)]),
    ("fmx_group_als_end", C.c_int, [H]),
    ("fmx_sgda_begin", C.c_int, [H]),
    ("fmx_sgda_epoch", C.c_int, [H, C.c_int, C.c_int, C.c_int, C.POINTER(EpochStats)]),
    ("fmx_sgda_epoch_minibatch", C.c_int, [H, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(EpochStats)]),
    ("fmx_sgda_get_reg", C.c_int, [H, C.c_void_p]),
    ("fmx_sgda_end", C.c_int, [H]),
    ("fmx_adapt_begin", C.c_int, [H, C.POINTER(AdaptOpts)]),
    ("fmx_adapt_epoch", C.c_int, [H, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(EpochStats)]),
    ("fmx_adapt_get_state_rows", C.c_int, [H, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("fmx_adapt_end", C.c_int, [H]),
    ("fmx_ftrl_begin", C.c_int, [H, C.POINTER(FtrlOpts)]),
    ("fmx_ftrl_epoch", C.c_int, [H, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(EpochStats)]),
    ("fmx_ftrl_get_state_rows", C.c_int, [H, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("fmx_ftrl_end", C.c_int, [H]),
    ("fmx_param_sparsity", C.c_int, [H, C.POINTER(Sparsity)]),
    ("fmx_group_adapt_begin", C.c_int, [H, C.POINTER(AdaptOpts)]),
    ("fmx_group_adapt_epoch", C.c_int, [H, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(EpochStats)]),
    ("fmx_group_adapt_get_state_rows", C.c_int, [H, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("fmx_group_adapt_end", C.c_int, [H]),
    ("fmx_group_ftrl_begin", C.c_int, [H, C.POINTER(FtrlOpts)]),
    ("fmx_group_ftrl_epoch", C.c_int, [H, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(EpochStats)]),
    ("fmx_group_ftrl_get_state_rows", C.c_int, [H, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("fmx_group_ftrl_end", C.c_int, [H]),
    ("fmx_group_param_sparsity", C.c_int, [H, C.POINTER(Sparsity)]),
    ("fmx_compact_begin", C.c_int, [H, C.POINTER(CompactOpts), C.POINTER(CompactInfo)]),
    ("fmx_compact_predict", C.c_int, [H, C.c_int, C.c_void_p]),
    ("fmx_compact_evaluate", C.c_int, [H, C.c_int, C.POINTER(Eval)]),
    ("fmx_compact_evaluate_ex", C.c_int, [H, C.c_int, C.POINTER(EvalOpts), C.POINTER(EvalEx)]),
    ("fmx_compact_topk", C.c_int, [H, C.c_int, C.c_int, C.POINTER(TopkOpts), C.c_void_p, C.c_void_p, C.POINTER(TopkStats)]),
    ("fmx_compact_get_rows", C.c_int, [H, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("fmx_compact_end", C.c_int, [H]),
    ("fmx_compact_row_bytes", C.c_uint32, [C.c_uint32, C.c_int]),
    ("fmx_compact_begin_pruned", C.c_int, [H, C.POINTER(CompactPruneOpts), C.POINTER(CompactInfo), C.POINTER(CompactPruneInfo)]),
    ("fmx_compact_slot_of", C.c_int, [H, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("fmx_checkpoint_save", C.c_int, [H, C.c_char_p, C.POINTER(CkptOpts), C.POINTER(CkptInfo)]),
    ("fmx_checkpoint_load", C.c_int, [H, C.c_char_p, C.POINTER(CkptOpts), C.POINTER(CkptInfo)]),
    ("fmx_checkpoint_info", C.c_int, [C.c_char_p, C.POINTER(CkptInfo), C.c_char_p, C.c_size_t]),
    ("fmx_group_checkpoint_save", C.c_int, [H, C.c_char_p, C.POINTER(CkptOpts), C.POINTER(CkptInfo)]),
    ("fmx_group_checkpoint_load", C.c_int, [H, C.c_char_p, C.POINTER(CkptOpts), C.POINTER(CkptInfo)]),
    ("fmx_als_begin", C.c_int, [H, C.c_int]),
    ("fmx_als_moments", C.c_int, [H, C.c_void_p]),
    ("fmx_als_sweep", C.c_int, [H, C.POINTER(AlsOpts), C.POINTER(AlsStats)]),
    ("fmx_als_end", C.c_int, [H]),
    ("fmx_upload_pairs", C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]),
    ("fmx_pair_epoch", C.c_int, [H, C.c_int, C.POINTER(PairOpts), C.POINTER(EpochStats)]),
    ("fmx_pair_evaluate", C.c_int, [H, C.c_int, C.POINTER(PairEval)]),
    ("fmx_topk", C.c_int, [H, C.c_int, C.c_int, C.POINTER(TopkOpts), C.c_void_p, C.c_void_p, C.POINTER(TopkStats)]),
    ("fmx_upload_interactions", C.c_int, [H, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("fmx_interactions_info", C.c_int, [H, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    ("fmx_pair_sample", C.c_int, [H, C.c_int, C.POINTER(PairNegOpts), C.c_void_p, C.POINTER(C.c_uint64)]),
    ("fmx_pair_epoch_sampled", C.c_int, [H, C.c_int, C.POINTER(PairNegOpts), C.POINTER(EpochStats), C.POINTER(C.c_uint64)]),
    ("fmx_pair_evaluate_sampled", C.c_int, [H, C.c_int, C.POINTER(PairNegOpts), C.POINTER(PairEval)]),
    ("fmx_adapt_pair_epoch", C.c_int, [H, C.c_int, C.POINTER(PairOpts), C.POINTER(EpochStats)]),
    ("fmx_adapt_pair_epoch_sampled", C.c_int, [H, C.c_int, C.POINTER(PairNegOpts), C.POINTER(EpochStats), C.POINTER(C.c_uint64)]),
    ("fmx_ftrl_pair_epoch", C.c_int, [H, C.c_int, C.POINTER(PairOpts), C.POINTER(EpochStats)]),
    ("fmx_ftrl_pair_epoch_sampled", C.c_int, [H, C.c_int, C.POINTER(PairNegOpts), C.POINTER(EpochStats), C.POINTER(C.c_uint64)]),
    ("fmx_compact_save", C.c_int, [H, C.c_char_p, C.POINTER(SnapInfo)]),
    ("fmx_compact_load", C.c_int, [H, C.c_char_p, C.POINTER(SnapInfo)]),
    ("fmx_snapshot_info", C.c_int, [C.c_char_p, C.POINTER(SnapInfo), C.c_char_p, C.c_size_t]),
    ("fmx_serve_open", C.c_int, [C.c_char_p, C.c_int, C.POINTER(H), C.POINTER(SnapInfo)]),
    ("fmx_get_info", C.c_int, [H, C.POINTER(Info)]),
    ("fmx_synchronize", C.c_int, [H]),
]

_lib = None


def load():
    """dlopen libfmx.so and bind every declared symbol.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        try:                       # torch bundles its own HIP runtime: when both live in one process torch's
            import torch  # noqa: F401   # must be loaded first, or torch.cuda finds no device afterwards
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise ImportError("libfm_amd/libfmx.so is not built: run `python -m libfm_amd.build` "
                              "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)          # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _block_args(entries, row_ptr, target, relations, keep):
    """the arguments of fmx_upload_block_rows_ex after the slot, and the arrays they point into (alive while the call runs)"""
    entries = np.ascontiguousarray(entries, dtype=ENTRY_DTYPE)
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
    target = None if target is None else np.ascontiguousarray(target, dtype=np.float32)
    n_rows = len(row_ptr) - 1
    alive, arr = [entries, row_ptr, target], (Relation * max(len(relations), 1))()
    for i, (re, rp, mp, off) in enumerate(relations):
        re = np.ascontiguousarray(re, dtype=ENTRY_DTYPE)
        rp = np.ascontiguousarray(rp, dtype=np.uint64)
        mp = np.ascontiguousarray(mp, dtype=np.uint32)
        if len(mp) != n_rows:
            raise ValueError("relation %d: the row mapping has %d entries for %d data rows" % (i, len(mp), n_rows))
        alive += [re, rp, mp]
        arr[i] = Relation(_ptr(re) if len(re) else None, _ptr(rp), len(rp) - 1, 0, len(re), _ptr(mp), int(off))
    alive.append(arr)
    return ((_ptr(entries) if len(entries) else None, _ptr(row_ptr), _ptr(target), n_rows, len(entries), arr, len(relations),
             1 if keep else 0), alive)


def default_w0_chunk(learn_rate, task):
    """what fmx_sgd_opts::w0_chunk = 0 resolves to (host arithmetic inside libfmx.so; no device needed)"""
    return int(load().fmx_default_w0_chunk(float(learn_rate), int(task)))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _set_row_queries(obj, fn, handle, slot, qid, n_queries):
    """the body of Handle / Group.set_row_queries; returns n_queries (None after qid=None)"""
    if qid is None:
        obj._chk(fn(handle, slot, None, 0))
        return None
    q = np.asarray(qid)
    if q.size and (q.dtype.kind not in "iu" or int(q.min()) < 0 or int(q.max()) > 0xFFFFFFFF):
        raise ValueError("set_row_queries: query ids are non-negative integers below 2^32")
    q = np.ascontiguousarray(q, dtype=np.uint32).reshape(-1)
    if n_queries is None:
        n_queries = int(q.max()) + 1 if q.size else 1
    if not 0 <= int(n_queries) <= 0xFFFFFFFF:
        raise ValueError("set_row_queries: n_queries out of range")
    obj._chk(fn(handle, slot, _ptr(q) if q.size else _ptr(np.zeros(1, dtype=np.uint32)), int(n_queries)))
    return int(n_queries)


def _evaluate_by_query(obj, fn, handle, slot, link, per_query, n_queries):
    """the body of Handle / Group.evaluate_by_query"""
    opts, ev = EvalOpts(link, 0), EvalQuery()
    if not per_query:
        obj._chk(fn(handle, slot, C.byref(opts), C.byref(ev), None, None, None))
        return ev
    if n_queries is None:                            # no ids were set through this object: the library says so
        obj._chk(fn(handle, slot, C.byref(opts), C.byref(ev), None, None, None))
        raise RuntimeError("evaluate_by_query(per_query=True): the query ids of slot %d were not set through this object" % slot)
    num2 = np.zeros(n_queries, dtype=np.uint64)
    pos, neg = np.zeros(n_queries, dtype=np.uint32), np.zeros(n_queries, dtype=np.uint32)
    obj._chk(fn(handle, slot, C.byref(opts), C.byref(ev), _ptr(num2), _ptr(pos), _ptr(neg)))
    return ev, num2, pos, neg


def _rank_opts(cutoffs, link):
    """fmx_rank_opts of a sequence of cutoffs; what the struct cannot hold is left for the library to refuse"""
    ks = [int(k) for k in cutoffs]
    if any(not 0 <= k <= 0xFFFFFFFF for k in ks):
        raise ValueError("evaluate_rank: cutoffs are non-negative integers below 2^32")
    opts = RankOpts(link, 0, len(ks))
    for j, k in enumerate(ks[:RANK_MAX_CUTOFFS]):
        opts.k[j] = k
    return opts


def _evaluate_rank(obj, fn, handle, slot, cutoffs, link, per_query, n_queries):
    """the body of Handle / Group.evaluate_rank"""
    opts, ev = _rank_opts(cutoffs, link), EvalRank()
    if not per_query:
        obj._chk(fn(handle, slot, C.byref(opts), C.byref(ev), None, None))
        return ev
    if n_queries is None:                            # no ids were set through this object: the library says so
        obj._chk(fn(handle, slot, C.byref(opts), C.byref(ev), None, None))
        raise RuntimeError("evaluate_rank(per_query=True): the query ids of slot %d were not set through this object" % slot)
    shape = (n_queries, min(max(opts.n_cutoffs, 1), RANK_MAX_CUTOFFS))
    dcg, hits = np.zeros(shape, dtype=np.float64), np.zeros(shape, dtype=np.float64)
    obj._chk(fn(handle, slot, C.byref(opts), C.byref(ev), _ptr(dcg), _ptr(hits)))
    return ev, dcg, hits


def rank_discounts(k_max):
    """D[0 .. k_max] of fmx_evaluate_rank: D[r + 1] = D[r] + 1 / log2(r + 2) (fmx_rank_discounts; host arithmetic, no device)"""
    if not 0 <= int(k_max) <= 0xFFFFFFFF:
        raise ValueError("rank_discounts: k_max out of range")
    out = np.zeros(min(int(k_max), RANK_MAX_K) + 1, dtype=np.float64)
    lib = load()
    rc = lib.fmx_rank_discounts(int(k_max), _ptr(out))
    if rc:
        raise FmxError(rc, (lib.fmx_last_error(None) or b"").decode())
    return out


class Handle:
    """Thin OO wrapper over an fmx_handle; every method is one C-ABI call."""

    def __init__(self, num_attribute, num_factor, k0=True, k1=True, task=TASK_REGRESSION, reg0=0.0, regw=0.0, regv=0.0,
                 learn_rate=0.0, min_target=0.0, max_target=0.0, device=-1, shard_rank=0, shard_world=1, shard_hash=0,
                 place_candidates=0, als_split_min=None, exchange_runs=0, exchange_algo=0):
        self.lib = load()
        self.cfg = Config(int(num_attribute), int(num_factor), int(bool(k0)), int(bool(k1)), int(task),
                          float(reg0), float(regw), float(regv), float(learn_rate), float(min_target),
                          float(max_target), int(device), int(shard_rank), int(shard_world), int(shard_hash),
                          int(place_candidates), int(ALS_SPLIT_MIN if als_split_min is None else als_split_min), int(exchange_runs), int(exchange_algo))
        self.h = H()
        rc = self.lib.fmx_create(C.byref(self.cfg), C.byref(self.h))
        if rc != FMX_OK:
            raise FmxError(rc, self.lib.fmx_last_error(None).decode())
        self._opened()

    def _opened(self):
        """what every way of making a Handle sets once self.lib, self.cfg and self.h stand (__init__, serve_open)"""
        self.n, self.k = int(self.cfg.num_attribute), int(self.cfg.num_factor)
        self._nq = {}                                # slot -> n_queries of the last set_row_queries (sizes the per-query arrays)
        self.G = 1                                   # attribute groups (set_groups)
        self.n_local = int(self.info().n_local)
        self.serve_only = False                      # serve_open: the handle holds a snapshot and no model
        self.snap_info = None                        # ... and this is its file's SnapInfo

    def _chk(self, rc):
        if rc != FMX_OK:
            raise FmxError(rc, self.lib.fmx_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.lib.fmx_destroy(self.h)
            self.h = H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # parameters ------------------------------------------------------------------------------
    def set_params(self, w0, w, v):
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        v = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        if w is not None:
            assert w.shape == (self.n,)
        if v is not None:
            assert v.shape == (self.k, self.n)
        self._chk(self.lib.fmx_set_params(self.h, float(w0), _ptr(w), _ptr(v)))

    def get_params(self, w=None, v=None):
        w0 = C.c_double(0)
        if w is None:
            w = np.zeros(self.n, dtype=np.float64)
        if v is None:
            v = np.zeros((self.k, self.n), dtype=np.float64)
        self._chk(self.lib.fmx_get_params(self.h, C.byref(w0), _ptr(w), _ptr(v) if self.k > 0 else None))
        return w0.value, w, v

    def init_params(self, mean, stdev, seed):
        self._chk(self.lib.fmx_init_params(self.h, float(mean), float(stdev), int(seed)))

    def get_param_rows(self, ids):
        """(w[ids], v[:, ids]) for spot checks when the full model does not fit the host."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        w = np.zeros(len(ids), dtype=np.float64)
        v = np.zeros((len(ids), max(self.k, 1)), dtype=np.float64)
        self._chk(self.lib.fmx_get_param_rows(self.h, _ptr(ids), len(ids), _ptr(w), _ptr(v) if self.k > 0 else None))
        return w, v[:, :self.k].T.copy()

    def save_model(self, path):
        """fm_model::saveModel (fm_model.h:132-154) straight from the device table"""
        self._chk(self.lib.fmx_save_model(self.h, os.fsencode(path)))

    def load_model(self, path):
        """fm_model::loadModel (fm_model.h:160-190); raises FmxError "malformed model file" where the reference returns 0"""
        self._chk(self.lib.fmx_load_model(self.h, os.fsencode(path)))

    def checkpoint_save(self, path, dense=False, model_only=False):
        """the exact binary checkpoint of the model and the open AdaGrad / FTRL session (fmx_checkpoint_save); returns CkptInfo"""
        opts, info = CkptOpts((CKPT_DENSE_STATE if dense else 0) | (CKPT_MODEL_ONLY if model_only else 0), 0), CkptInfo()
        self._chk(self.lib.fmx_checkpoint_save(self.h, os.fsencode(path), C.byref(opts), C.byref(info)))
        return info

    def checkpoint_load(self, path, model_only=False):
        """replace the parameters, and unless model_only the session, by a checkpoint's (fmx_checkpoint_load); returns CkptInfo"""
        opts, info = CkptOpts(CKPT_MODEL_ONLY if model_only else 0, 0), CkptInfo()
        self._chk(self.lib.fmx_checkpoint_load(self.h, os.fsencode(path), C.byref(opts), C.byref(info)))
        return info

    def get_w0(self):
        w0 = C.c_double(0)
        self._chk(self.lib.fmx_get_w0(self.h, C.byref(w0)))
        return w0.value

    def set_groups(self, group):
        """attribute -> group ids (`-meta`, Data.h:85-97); None = one group."""
        if group is None:
            self._chk(self.lib.fmx_set_groups(self.h, None, 1))
            self.G = 1
            return
        group = np.ascontiguousarray(group, dtype=np.uint32)
        if len(group) != self.n:
            raise ValueError("set_groups: need one group id per feature (%d), got %d" % (self.n, len(group)))
        G = int(group.max()) + 1 if len(group) else 1
        self._chk(self.lib.fmx_set_groups(self.h, _ptr(group), G))
        self.G = max(G, 1)

    # rows ------------------------------------------------------------------------------------
    def upload_rows(self, slot, entries, row_ptr, target):
        entries = np.ascontiguousarray(entries, dtype=ENTRY_DTYPE)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        target = None if target is None else np.ascontiguousarray(target, dtype=np.float32)
        n_rows = len(row_ptr) - 1
        self._chk(self.lib.fmx_upload_rows(self.h, slot, _ptr(entries) if len(entries) else None, _ptr(row_ptr),
                                           _ptr(target), n_rows, len(entries)))
        return n_rows

    def synth_rows(self, slot, seed, row0, n_rows, nnz, shape=SYNTH_UNIFORM):
        self._chk(self.lib.fmx_synth_rows_ex(self.h, slot, int(seed), int(row0), int(n_rows), int(nnz), int(shape)))

    def download_rows(self, slot):
        n_rows, nnz = C.c_uint32(0), C.c_uint64(0)
        self._chk(self.lib.fmx_rows_info(self.h, slot, C.byref(n_rows), C.byref(nnz)))
        ent = np.zeros(nnz.value, dtype=ENTRY_DTYPE)
        rp = np.zeros(n_rows.value + 1, dtype=np.uint64)
        y = np.zeros(n_rows.value, dtype=np.float32)
        self._chk(self.lib.fmx_download_rows(self.h, slot, _ptr(ent) if nnz.value else None, _ptr(rp), _ptr(y)))
        return ent, rp, y

    def wtrain_info(self, slot):
        """(singles of the slot, whether its training-side weight stream was kept) -- as the slot's first one-pass epoch left them"""
        singles, kept = C.c_uint64(0), C.c_int(0)
        self._chk(self.lib.fmx_wtrain_info(self.h, slot, C.byref(singles), C.byref(kept)))
        return int(singles.value), bool(kept.value)

    def free_rows(self, slot):
        self._chk(self.lib.fmx_free_rows(self.h, slot))

    # compute ---------------------------------------------------------------------------------
    def upload_block_rows(self, slot, entries, row_ptr, target, relations, keep=False):
        """relations: list of (entries, row_ptr, data_row_to_relation_row, attr_offset) -- `-relation` blocks
        (relation.h:32-60).  keep=False: the joined rows are expanded on the device; keep=True (FMX_BLOCKS_KEEP): main rows and
        blocks stay apart, ALS / MCMC sweep the blocks through per-block-row caches like the reference."""
        args, alive = _block_args(entries, row_ptr, target, relations, keep)
        self._chk(self.lib.fmx_upload_block_rows_ex(self.h, slot, *args))
        return args[3]

    def predict(self, slot, n_rows):
        out = np.zeros(n_rows, dtype=np.float64)
        self._chk(self.lib.fmx_predict(self.h, slot, _ptr(out)))
        return out

    def evaluate(self, slot):
        ev = Eval()
        self._chk(self.lib.fmx_evaluate(self.h, slot, C.byref(ev)))
        return ev

    def evaluate_ex(self, slot, link=LINK_LOGISTIC):
        """exact AUC, log loss and the counts behind them, reduced on the device (fmx_evaluate_ex)"""
        opts, ev = EvalOpts(link, 0), EvalEx()
        self._chk(self.lib.fmx_evaluate_ex(self.h, slot, C.byref(opts), C.byref(ev)))
        return ev

    def set_row_queries(self, slot, qid, n_queries=None):
        """per-row query ids of a slot (fmx_set_row_queries); n_queries None = max + 1, qid None drops them"""
        self._nq[slot] = _set_row_queries(self, self.lib.fmx_set_row_queries, self.h, slot, qid, n_queries)

    def set_row_weights(self, slot, weights):
        """per-row weights of a slot (fmx_set_row_weights): one finite float32 >= 0 per row; None drops them.  fmx_adapt / fmx_ftrl
        epochs on the slot then scale every row's loss by its weight; the trainers without a weighted form refuse the slot"""
        if weights is None:
            self._chk(self.lib.fmx_set_row_weights(self.h, slot, None))
            return
        n_rows = C.c_uint32(0)
        self._chk(self.lib.fmx_rows_info(self.h, slot, C.byref(n_rows), None))
        w = np.ascontiguousarray(np.asarray(weights).reshape(-1), dtype=np.float32)
        if len(w) != n_rows.value:
            raise ValueError("set_row_weights: %d weights for %d rows" % (len(w), n_rows.value))
        buf = w if len(w) else np.zeros(1, dtype=np.float32)           # (an empty slot still takes a non-NULL pointer: NULL drops)
        self._chk(self.lib.fmx_set_row_weights(self.h, slot, _ptr(buf)))

    def get_row_weights(self, slot):
        """the weights as stored (fmx_get_row_weights): float32 [n_rows]"""
        n_rows = C.c_uint32(0)
        self._chk(self.lib.fmx_rows_info(self.h, slot, C.byref(n_rows), None))
        out = np.zeros(n_rows.value, dtype=np.float32)
        self._chk(self.lib.fmx_get_row_weights(self.h, slot, _ptr(out) if len(out) else None))
        return out

    def evaluate_weighted(self, slot, link=LINK_LOGISTIC):
        """weighted log loss / accuracy (classification) or RMSE / MAE (regression) and the sums behind them, reduced on the device
        in a fixed order (fmx_evaluate_weighted): the EvalWeighted struct"""
        opts, ev = EvalOpts(link, 0), EvalWeighted()
        self._chk(self.lib.fmx_evaluate_weighted(self.h, slot, C.byref(opts), C.byref(ev)))
        return ev

    def evaluate_by_query(self, slot, link=LINK_LOGISTIC, per_query=False):
        """exact AUC inside every query (GAUC), reduced on the device (fmx_evaluate_by_query): the EvalQuery struct, or with
        per_query (struct, num2_q uint64, pos_q uint32, neg_q uint32), each [n_queries]"""
        return _evaluate_by_query(self, self.lib.fmx_evaluate_by_query, self.h, slot, link, per_query, self._nq.get(slot))

    def evaluate_rank(self, slot, cutoffs, link=LINK_LOGISTIC, per_query=False):
        """exact tie-averaged NDCG / recall / precision at up to four ascending cutoffs inside every query, reduced on the device
        (fmx_evaluate_rank): the EvalRank struct, or with per_query=True (EvalRank, dcg_q, hits_q), float64 [n_queries, n_cutoffs]"""
        return _evaluate_rank(self, self.lib.fmx_evaluate_rank, self.h, slot, cutoffs, link, per_query, self._nq.get(slot))

    # the posterior accumulator of a slot (fmx_post_*): MCMC's averaged predictions on the device
    def post_begin(self, slot, burn_in=5, eval_rows=0):
        opts = PostOpts(int(burn_in), int(eval_rows), 0, 0)
        self._chk(self.lib.fmx_post_begin(self.h, slot, C.byref(opts)))

    def post_accumulate(self, slot):
        """add the draw of the current parameters; the reference's metrics of the three vectors (PostStats.m[POST_*])"""
        st = PostStats()
        self._chk(self.lib.fmx_post_accumulate(self.h, slot, C.byref(st)))
        return st

    def post_evaluate_ex(self, slot, which=POST_ALL):
        ev = EvalEx()
        self._chk(self.lib.fmx_post_evaluate_ex(self.h, slot, int(which), C.byref(ev)))
        return ev

    def post_get(self, slot, which, n_rows):
        """(the sum over the draws -- or the last draw itself for POST_THIS -- as float64 [n_rows], the number of draws in it)"""
        out, draws = np.zeros(n_rows, dtype=np.float64), C.c_uint64(0)
        self._chk(self.lib.fmx_post_get(self.h, slot, int(which), _ptr(out), C.byref(draws)))
        return out, int(draws.value)

    def post_end(self, slot):
        self._chk(self.lib.fmx_post_end(self.h, slot))

    def sgd_epoch(self, slot, mode, apply=APPLY_DEFAULT, batch=0, w0_chunk=0, flags=0, bias_lag=0):
        opts = SgdOpts(mode, apply, batch, w0_chunk, flags, bias_lag)
        st = EpochStats()
        self._chk(self.lib.fmx_sgd_epoch(self.h, slot, C.byref(opts), C.byref(st)))
        return st

    def sgd_batch_info(self, slot, batch=0, mode=SGD_MINIBATCH, apply=APPLY_DEFAULT):
        """the batch fmx_sgd_epoch would run with on this slot, the rows' collision mass and the gain (fmx_batch_info)"""
        opts = SgdOpts(mode, apply, batch, 0, 0, 0)
        bi = BatchInfo()
        self._chk(self.lib.fmx_sgd_batch_info(self.h, slot, C.byref(opts), C.byref(bi)))
        return bi

    def place_info(self):
        """how fmx_create placed the parameter tables (fmx_place_info)"""
        pi = PlaceInfo()
        self._chk(self.lib.fmx_get_place_info(self.h, C.byref(pi)))
        return pi

    def partial_floats(self, batch):
        n = C.c_uint64(0)
        self._chk(self.lib.fmx_partial_floats(self.h, batch, C.byref(n)))
        return n.value

    def sgd_partial(self, slot, row0, n_rows, d_partial_ptr, stream=None):
        self._chk(self.lib.fmx_sgd_partial(self.h, slot, row0, n_rows, d_partial_ptr, stream))

    def sgd_finish(self, slot, row0, n_rows, d_partial_ptr, apply=APPLY_DEFAULT, w0_chunk=0, stream=None, batch=0, flags=0, bias_lag=0):
        opts = SgdOpts(SGD_MINIBATCH, apply, batch or n_rows, w0_chunk, flags, bias_lag)
        self._chk(self.lib.fmx_sgd_finish(self.h, slot, row0, n_rows, d_partial_ptr, C.byref(opts), stream))

    def predict_finish(self, n_rows, d_partial_ptr, d_yhat_ptr, stream=None):
        self._chk(self.lib.fmx_predict_finish(self.h, n_rows, d_partial_ptr, d_yhat_ptr, stream))

    # pairwise ranking (BPR) -----------------------------------------------------------------
    def upload_pairs(self, slot, row_a, row_b):
        """the pairs of a row slot: row_a[t] is preferred to row_b[t] (0-based rows of the slot); replaces earlier pairs"""
        row_a = np.ascontiguousarray(row_a, dtype=np.uint32)
        row_b = np.ascontiguousarray(row_b, dtype=np.uint32)
        if row_a.shape != row_b.shape or row_a.ndim != 1:
            raise ValueError("upload_pairs: row_a and row_b must be 1-d arrays of one length")
        self._chk(self.lib.fmx_upload_pairs(self.h, slot, _ptr(row_a) if len(row_a) else None,
                                            _ptr(row_b) if len(row_b) else None, len(row_a)))

    def pair_epoch(self, slot, mode=SGD_SEQUENTIAL, batch=0, flags=0):
        """one epoch of the pairwise learner over the slot's pairs (fmx_pair_epoch); returns EpochStats (rows = pairs)"""
        opts = PairOpts(int(mode), int(batch), int(flags), 0)
        st = EpochStats()
        self._chk(self.lib.fmx_pair_epoch(self.h, slot, C.byref(opts), C.byref(st)))
        return st

    def pair_evaluate(self, slot):
        """pair accuracy (y_a > y_b) and mean -ln sigmoid(y_a - y_b) over the slot's pairs (fmx_pair_evaluate)"""
        ev = PairEval()
        self._chk(self.lib.fmx_pair_evaluate(self.h, slot, C.byref(ev)))
        return ev

    # BPR on query x candidate interactions, negatives drawn on the device ---------------------
    def upload_interactions(self, query_slot, cand_slot, q_row, c_row, exclude=None):
        """the observed (query row, candidate row) interactions of query_slot against cand_slot; replaces earlier ones.
        exclude: None, or (ptr [Q + 1], idx) -- a CSR over ALL query rows of candidate rows never drawn as negatives -- or a
        list of Q iterables; any order, repeats allowed."""
        q_row = np.ascontiguousarray(q_row, dtype=np.uint32)
        c_row = np.ascontiguousarray(c_row, dtype=np.uint32)
        if q_row.shape != c_row.shape or q_row.ndim != 1:
            raise ValueError("upload_interactions: q_row and c_row must be 1-d arrays of one length")
        ex_ptr = ex_idx = None
        if exclude is not None:
            if isinstance(exclude, tuple) and len(exclude) == 2:
                ex_ptr = np.ascontiguousarray(exclude[0], dtype=np.uint64)
                ex_idx = np.ascontiguousarray(exclude[1], dtype=np.uint32)
            else:
                lists = [np.asarray(list(e), dtype=np.uint32) for e in exclude]
                ex_ptr = np.zeros(len(lists) + 1, dtype=np.uint64)
                ex_ptr[1:] = np.cumsum([len(e) for e in lists])
                ex_idx = np.concatenate(lists).astype(np.uint32) if lists else np.zeros(0, dtype=np.uint32)
            n_rows = C.c_uint32(0)
            self._chk(self.lib.fmx_rows_info(self.h, query_slot, C.byref(n_rows), None))
            if len(ex_ptr) != n_rows.value + 1:
                raise ValueError("upload_interactions: exclude_ptr must hold one offset per query row + 1 = %d" % (n_rows.value + 1))
        self._chk(self.lib.fmx_upload_interactions(self.h, query_slot, cand_slot, _ptr(q_row) if len(q_row) else None,
                                                   _ptr(c_row) if len(c_row) else None, len(q_row), _ptr(ex_ptr),
                                                   _ptr(ex_idx) if ex_idx is not None and len(ex_idx) else None))

    def interactions_info(self, query_slot):
        """(candidate slot, number of interactions) of the interactions that live on query_slot (fmx_interactions_info)"""
        cand, n = C.c_int(0), C.c_uint64(0)
        self._chk(self.lib.fmx_interactions_info(self.h, query_slot, C.byref(cand), C.byref(n)))
        return cand.value, int(n.value)

    def pair_sample(self, query_slot, n_neg=1, seed=0, epoch=0, draws=1):
        """the negatives fmx_pair_epoch_sampled trains on for (seed, epoch): (neg uint32 [n * n_neg], forced) (fmx_pair_sample);
        draws = M > 1: the hardest of M accepted draws under the current parameters"""
        opts = PairNegOpts(SGD_SEQUENTIAL, 0, int(n_neg), neg_flags(draws), int(seed), int(epoch))
        neg = np.zeros(self.interactions_info(query_slot)[1] * max(int(n_neg), 0), dtype=np.uint32)
        forced = C.c_uint64(0)
        self._chk(self.lib.fmx_pair_sample(self.h, query_slot, C.byref(opts), _ptr(neg) if len(neg) else None, C.byref(forced)))
        return neg, int(forced.value)

    def pair_epoch_sampled(self, query_slot, mode=SGD_SEQUENTIAL, batch=0, n_neg=1, seed=0, epoch=0, flags=0, draws=1):
        """one epoch over the interactions with the negatives of (seed, epoch) (fmx_pair_epoch_sampled): (EpochStats, forced);
        draws = M > 1: hardest of M, scored with the parameters at the start of the epoch (OR-ed into flags)"""
        opts = PairNegOpts(int(mode), int(batch), int(n_neg), int(flags) | neg_flags(draws), int(seed), int(epoch))
        st = EpochStats()
        forced = C.c_uint64(0)
        self._chk(self.lib.fmx_pair_epoch_sampled(self.h, query_slot, C.byref(opts), C.byref(st), C.byref(forced)))
        return st, int(forced.value)

    def pair_evaluate_sampled(self, query_slot, n_neg=1, seed=0, epoch=0, draws=1):
        """pair accuracy and mean -ln sigmoid(y_a - y_b) over the pairs of (seed, epoch) (fmx_pair_evaluate_sampled)"""
        opts = PairNegOpts(SGD_SEQUENTIAL, 0, int(n_neg), neg_flags(draws), int(seed), int(epoch))
        ev = PairEval()
        self._chk(self.lib.fmx_pair_evaluate_sampled(self.h, query_slot, C.byref(opts), C.byref(ev)))
        return ev

    # top-K retrieval -------------------------------------------------------------------------
    def topk(self, query_slot, cand_slot, topk, query_row0=0, n_query=None, exclude=None, stats=False, _fn=None):
        """the topk best candidate rows of cand_slot for every query row [query_row0, query_row0 + n_query) of query_slot
        (fmx_topk): returns (idx uint32 [n, topk], score float64 [n, topk]), padded with (TOPK_NONE, -inf); with stats=True
        also the TopkStats.  exclude: None, or (ptr [n + 1], idx) -- a CSR of candidate rows per query of this call -- or a
        list of n iterables of candidate rows."""
        if n_query is None:
            n_rows = C.c_uint32(0)
            self._chk(self.lib.fmx_rows_info(self.h, query_slot, C.byref(n_rows), None))
            n_query = max(n_rows.value - int(query_row0), 0)
        n_query = int(n_query)
        topk = int(topk)
        ex_ptr = ex_idx = None
        if exclude is not None:
            if isinstance(exclude, tuple) and len(exclude) == 2:
                ex_ptr = np.ascontiguousarray(exclude[0], dtype=np.uint64)
                ex_idx = np.ascontiguousarray(exclude[1], dtype=np.uint32)
            else:
                lists = [np.asarray(list(e), dtype=np.uint32) for e in exclude]
                ex_ptr = np.zeros(len(lists) + 1, dtype=np.uint64)
                ex_ptr[1:] = np.cumsum([len(e) for e in lists])
                ex_idx = np.concatenate(lists).astype(np.uint32) if lists else np.zeros(0, dtype=np.uint32)
            if len(ex_ptr) != n_query + 1:
                raise ValueError("topk: exclude_ptr must hold n_query + 1 = %d offsets" % (n_query + 1))
        opts = TopkOpts(topk, 0, int(query_row0), n_query, 0, _ptr(ex_ptr), _ptr(ex_idx) if ex_idx is not None and len(ex_idx) else None)
        idx = np.zeros((n_query, max(topk, 0)), dtype=np.uint32)
        score = np.zeros((n_query, max(topk, 0)), dtype=np.float64)
        st = TopkStats()
        self._chk((_fn or self.lib.fmx_topk)(self.h, query_slot, cand_slot, C.byref(opts), _ptr(idx), _ptr(score), C.byref(st)))
        return (idx, score, st) if stats else (idx, score)

    # SGDA ------------------------------------------------------------------------------------
    def sgda_begin(self):
        self._chk(self.lib.fmx_sgda_begin(self.h))

    def sgda_epoch(self, train_slot, val_slot, do_lambda):
        st = EpochStats()
        self._chk(self.lib.fmx_sgda_epoch(self.h, train_slot, val_slot, int(do_lambda), C.byref(st)))
        return st

    def sgda_epoch_minibatch(self, train_slot, val_slot, do_lambda, batch=0, w0_chunk=0):
        st = EpochStats()
        self._chk(self.lib.fmx_sgda_epoch_minibatch(self.h, train_slot, val_slot, int(do_lambda), int(batch), int(w0_chunk), C.byref(st)))
        return st

    def sgda_get_reg(self):
        """[G][1 + k]: column 0 = reg_w(g), columns 1.. = reg_v(g, f)."""
        out = np.zeros((self.G, 1 + self.k), dtype=np.float64)
        self._chk(self.lib.fmx_sgda_get_reg(self.h, _ptr(out)))
        return out

    def sgda_end(self):
        self._chk(self.lib.fmx_sgda_end(self.h))

    # AdaGrad on the minibatch rule (include/fmx.h "fmx_adapt_*") --------------------------------
    def adapt_begin(self, rule="adagrad", init_acc=0.0, learn_rate=0.0):
        """opens (or resets) the session: every accumulator = init_acc (0 = 1.0); learn_rate 0 = the handle's"""
        if isinstance(rule, str):                    # (an integer goes to the library as it is: it refuses the ones it does not know)
            if rule != "adagrad":
                raise ValueError("adapt_begin: unknown rule %r (adagrad)" % (rule,))
            rule = ADAPT_ADAGRAD
        opts = AdaptOpts(int(rule), 0, float(init_acc), float(learn_rate))
        self._chk(self.lib.fmx_adapt_begin(self.h, C.byref(opts)))

    def adapt_epoch(self, slot, batch=0, w0_chunk=0):
        st = EpochStats()
        self._chk(self.lib.fmx_adapt_epoch(self.h, int(slot), int(batch), int(w0_chunk), C.byref(st)))
        return st

    def adapt_state_rows(self, ids):
        """(n_w[ids], n_v[:, ids]): the accumulators, in the layout of get_param_rows"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        nw = np.zeros(len(ids), dtype=np.float64)
        nv = np.zeros((len(ids), max(self.k, 1)), dtype=np.float64)
        self._chk(self.lib.fmx_adapt_get_state_rows(self.h, _ptr(ids), len(ids), _ptr(nw), _ptr(nv) if self.k > 0 else None))
        return nw, nv[:, :self.k].T.copy()

    def adapt_end(self):
        self._chk(self.lib.fmx_adapt_end(self.h))

    # FTRL-proximal with L1 on the minibatch rule (include/fmx.h "fmx_ftrl_*") -------------------
    def ftrl_begin(self, alpha=0.0, beta=1.0, l1_w=0.0, l1_v=0.0, l2_w=0.0, l2_v=0.0, init_acc=0.0):
        """opens (or resets) the session: n = init_acc, z derived from the parameters the handle holds now; alpha 0 = the handle's
        learn_rate"""
        opts = FtrlOpts(0, 0, float(alpha), float(beta), float(l1_w), float(l1_v), float(l2_w), float(l2_v), float(init_acc))
        self._chk(self.lib.fmx_ftrl_begin(self.h, C.byref(opts)))

    def ftrl_epoch(self, slot, batch=0, w0_chunk=0):
        st = EpochStats()
        self._chk(self.lib.fmx_ftrl_epoch(self.h, int(slot), int(batch), int(w0_chunk), C.byref(st)))
        return st

    def ftrl_state_rows(self, ids):
        """(z_w[ids], z_v[:, ids], n_w[ids], n_v[:, ids]), each pair in the layout of get_param_rows"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        zw, nw = np.zeros(len(ids), dtype=np.float64), np.zeros(len(ids), dtype=np.float64)
        zv, nv = (np.zeros((len(ids), max(self.k, 1)), dtype=np.float64) for _ in range(2))
        self._chk(self.lib.fmx_ftrl_get_state_rows(self.h, _ptr(ids), len(ids), _ptr(zw), _ptr(zv) if self.k > 0 else None,
                                                   _ptr(nw), _ptr(nv) if self.k > 0 else None))
        return zw, zv[:, :self.k].T.copy(), nw, nv[:, :self.k].T.copy()

    def ftrl_end(self):
        self._chk(self.lib.fmx_ftrl_end(self.h))

    # pairwise ranking stepped by the open session's rule (include/fmx.h "fmx_adapt_pair_epoch") --
    def _rule_pair_epoch(self, fn, slot, batch, mode):
        opts = PairOpts(int(mode), int(batch), 0, 0)
        st = EpochStats()
        self._chk(fn(self.h, int(slot), C.byref(opts), C.byref(st)))
        return st

    def _rule_pair_epoch_sampled(self, fn, query_slot, batch, n_neg, seed, epoch, draws, mode):
        opts = PairNegOpts(int(mode), int(batch), int(n_neg), neg_flags(draws), int(seed), int(epoch))
        st = EpochStats()
        forced = C.c_uint64(0)
        self._chk(fn(self.h, int(query_slot), C.byref(opts), C.byref(st), C.byref(forced)))
        return st, int(forced.value)

    def adapt_pair_epoch(self, slot, batch=0, mode=SGD_MINIBATCH):
        """one epoch over the slot's pairs by the batch rule, every touched coordinate stepped by the open AdaGrad session
        (fmx_adapt_pair_epoch); returns EpochStats.  mode is there for the library's refusal of the other schedules."""
        return self._rule_pair_epoch(self.lib.fmx_adapt_pair_epoch, slot, batch, mode)

    def adapt_pair_epoch_sampled(self, query_slot, batch=0, n_neg=1, seed=0, epoch=0, draws=1, mode=SGD_MINIBATCH):
        """the same over the interactions with the negatives of (seed, epoch) (fmx_adapt_pair_epoch_sampled): (EpochStats, forced)"""
        return self._rule_pair_epoch_sampled(self.lib.fmx_adapt_pair_epoch_sampled, query_slot, batch, n_neg, seed, epoch, draws, mode)

    def ftrl_pair_epoch(self, slot, batch=0, mode=SGD_MINIBATCH):
        """one epoch over the slot's pairs by the batch rule, every touched coordinate stepped by the open FTRL session
        (fmx_ftrl_pair_epoch); returns EpochStats"""
        return self._rule_pair_epoch(self.lib.fmx_ftrl_pair_epoch, slot, batch, mode)

    def ftrl_pair_epoch_sampled(self, query_slot, batch=0, n_neg=1, seed=0, epoch=0, draws=1, mode=SGD_MINIBATCH):
        """the same over the interactions with the negatives of (seed, epoch) (fmx_ftrl_pair_epoch_sampled): (EpochStats, forced)"""
        return self._rule_pair_epoch_sampled(self.lib.fmx_ftrl_pair_epoch_sampled, query_slot, batch, n_neg, seed, epoch, draws, mode)

    def param_sparsity(self):
        """fmx_sparsity: how many coordinates of the model are exactly zero"""
        sp = Sparsity()
        self._chk(self.lib.fmx_param_sparsity(self.h, C.byref(sp)))
        return sp

    # the serving snapshot (include/fmx.h "fmx_compact_*") --------------------------------------
    def compact_begin(self, format=COMPACT_BF16, flags=0):
        """takes (or replaces) the frozen copy of the model as it stands (COMPACT_BF16 or COMPACT_INT8); returns its CompactInfo"""
        opts, info = CompactOpts(int(format), int(flags)), CompactInfo()
        self._chk(self.lib.fmx_compact_begin(self.h, C.byref(opts), C.byref(info)))
        return info

    def compact_begin_pruned(self, format=COMPACT_BF16, seen_slot=None):
        """takes (or replaces) a snapshot that keeps only the features that can score (fmx_compact_begin_pruned): the dead ones go, and
        with seen_slot also those without an entry in that slot; returns (CompactInfo, CompactPruneInfo)"""
        opts = CompactPruneOpts(int(format), PRUNE_DEAD | (PRUNE_SEEN if seen_slot is not None else 0),
                                -1 if seen_slot is None else int(seen_slot), 0)
        info, pinfo = CompactInfo(), CompactPruneInfo()
        self._chk(self.lib.fmx_compact_begin_pruned(self.h, C.byref(opts), C.byref(info), C.byref(pinfo)))
        return info, pinfo

    def compact_slot_of(self, ids):
        """the stored row of each feature id in the pruned snapshot, SLOT_NONE for a dropped one (fmx_compact_slot_of)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.zeros(len(ids), dtype=np.uint32)
        self._chk(self.lib.fmx_compact_slot_of(self.h, _ptr(ids), len(ids), _ptr(out)))
        return out

    def compact_predict(self, slot, n_rows):
        out = np.zeros(n_rows, dtype=np.float64)
        self._chk(self.lib.fmx_compact_predict(self.h, slot, _ptr(out)))
        return out

    def compact_evaluate(self, slot):
        ev = Eval()
        self._chk(self.lib.fmx_compact_evaluate(self.h, slot, C.byref(ev)))
        return ev

    def compact_evaluate_ex(self, slot, link=LINK_LOGISTIC):
        opts, ev = EvalOpts(link, 0), EvalEx()
        self._chk(self.lib.fmx_compact_evaluate_ex(self.h, slot, C.byref(opts), C.byref(ev)))
        return ev

    def compact_topk(self, query_slot, cand_slot, topk, query_row0=0, n_query=None, exclude=None, stats=False):
        """topk() with the factor sums of both slots taken from the snapshot (fmx_compact_topk)"""
        return self.topk(query_slot, cand_slot, topk, query_row0, n_query, exclude, stats, _fn=self.lib.fmx_compact_topk)

    def compact_rows(self, ids):
        """(w[ids], dequantised v[:, ids]) of the snapshot, in the layout of get_param_rows"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        w = np.zeros(len(ids), dtype=np.float64)
        v = np.zeros((len(ids), max(self.k, 1)), dtype=np.float64)
        self._chk(self.lib.fmx_compact_get_rows(self.h, _ptr(ids), len(ids), _ptr(w), _ptr(v) if self.k > 0 else None))
        return w, v[:, :self.k].T.copy()

    def compact_end(self):
        self._chk(self.lib.fmx_compact_end(self.h))

    def compact_save(self, path):
        """the snapshot as a file, straight from its device tables (fmx_compact_save); returns SnapInfo"""
        info = SnapInfo()
        self._chk(self.lib.fmx_compact_save(self.h, os.fsencode(path), C.byref(info)))
        return info

    def compact_load(self, path):
        """take (or replace) the snapshot from a file (fmx_compact_load): the model is untouched, and so is the earlier snapshot when
        the file is refused; returns SnapInfo"""
        info = SnapInfo()
        self._chk(self.lib.fmx_compact_load(self.h, os.fsencode(path), C.byref(info)))
        return info

    # ALS / MCMC ----------------------------------------------------------------------------
    def als_begin(self, train_slot):
        self._chk(self.lib.fmx_als_begin(self.h, train_slot))

    def als_moments(self):
        """(sum e^2, sum e, m) with m[1 + k][G][2]: row 0 = w, row 1+f = v_f; per group {sum theta, sum theta^2}."""
        out = np.zeros(2 + 2 * self.G * (1 + self.k), dtype=np.float64)
        self._chk(self.lib.fmx_als_moments(self.h, _ptr(out)))
        return out[0], out[1], out[2:].reshape(1 + self.k, self.G, 2)

    def als_sweep(self, w_lambda, v_lambda, alpha=1.0, w_mu=0.0, v_mu=0.0, do_sample=False, seed=0):
        """w_lambda / w_mu: scalar or [G]; v_lambda / v_mu: scalar, [k] or [G][k] (the reference's w_lambda(g),
        v_lambda(g,f); fm_learn_mcmc.h:1116-1122)."""
        opts, keep = self._als_opts(w_lambda, v_lambda, alpha, w_mu, v_mu, do_sample, seed)
        st = AlsStats()
        self._chk(self.lib.fmx_als_sweep(self.h, C.byref(opts), C.byref(st)))
        return st

    def _als_opts(self, w_lambda, v_lambda, alpha, w_mu, v_mu, do_sample, seed):
        G, k = self.G, max(self.k, 1)

        def tab_w(x):
            return np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (G,)))

        def tab_v(x):
            x = np.asarray(x, dtype=np.float64)
            if x.ndim == 1 and x.shape[0] != 1:
                if G > 1 and G == k:                 # a [G] per-group vector and a [k] per-factor vector look the same
                    raise ValueError("1-D v_lambda / v_mu is ambiguous with num_groups == num_factor: pass a [G][k] table")
                if x.shape[0] == G and G > 1:
                    x = x[:, None]                   # one value per group
                elif x.shape[0] != k:
                    raise ValueError("1-D v_lambda / v_mu must have num_groups (%d) or num_factor (%d) entries" % (G, k))
            return np.ascontiguousarray(np.broadcast_to(x, (G, k)))
        wl, wm, vl, vm = tab_w(w_lambda), tab_w(w_mu), tab_v(v_lambda), tab_v(v_mu)
        opts = AlsOpts(alpha, float(wm[0]), float(wl[0]), float(vm[0, 0]), float(vl[0, 0]), int(do_sample), 0, seed,
                       _ptr(vm[0]) if G == 1 else None, _ptr(vl[0]) if G == 1 else None,
                       G if G > 1 else 0, 0, _ptr(wm), _ptr(wl), _ptr(vm), _ptr(vl))
        if G > 1 and self.k != k:                    # k == 0: tables are [G][0]
            opts.v_mu_gf = opts.v_lambda_gf = None
        return opts, (wl, wm, vl, vm)                # the arrays must outlive the call

    def als_end(self):
        self._chk(self.lib.fmx_als_end(self.h))

    # one process per GPU ---------------------------------------------------------------------
    def comm_init_rank(self, unique_id, rank, world):
        """unique_id: the COMM_ID_BYTES bytes rank 0 got from comm_unique_id() (handed over by the launcher)"""
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        self._chk(self.lib.fmx_comm_init_rank(self.h, buf, int(rank), int(world)))

    def comm_destroy(self):
        self._chk(self.lib.fmx_comm_destroy(self.h))

    def info(self):
        inf = Info()
        self._chk(self.lib.fmx_get_info(self.h, C.byref(inf)))
        return inf

    def synchronize(self):
        self._chk(self.lib.fmx_synchronize(self.h))


def checkpoint_info(path):
    """the header of a checkpoint file (fmx_checkpoint_info: no handle, no device); raises FmxError with the parser's reason"""
    info, err = CkptInfo(), C.create_string_buffer(256)
    rc = load().fmx_checkpoint_info(os.fsencode(path), C.byref(info), err, len(err))
    if rc:
        raise FmxError(rc, err.value.decode())
    return info


def snapshot_info(path):
    """the header of a snapshot file (fmx_snapshot_info: no handle, no device); raises FmxError with the parser's reason"""
    info, err = SnapInfo(), C.create_string_buffer(256)
    rc = load().fmx_snapshot_info(os.fsencode(path), C.byref(info), err, len(err))
    if rc:
        raise FmxError(rc, err.value.decode())
    return info


def serve_open(path, device=-1):
    """a SERVE-ONLY Handle from a snapshot file alone (fmx_serve_open): it holds the file's snapshot and no model, so only the row side,
    the compact_* calls, info, place_info, synchronize and close work on it -- everything else raises FmxError(FMX_E_STATE).
    snap_info is the file's SnapInfo."""
    lib = load()
    h, info = H(), SnapInfo()
    rc = lib.fmx_serve_open(os.fsencode(path), int(device), C.byref(h), C.byref(info))
    if rc != FMX_OK:
        raise FmxError(rc, (lib.fmx_last_error(None) or b"").decode())
    obj = Handle.__new__(Handle)
    obj.lib, obj.h = lib, h
    obj.cfg = Config(num_attribute=int(info.num_attribute), num_factor=int(info.num_factor), k0=int(info.k0), k1=int(info.k1),
                     task=int(info.task), min_target=float(info.min_target), max_target=float(info.max_target), device=int(device),
                     shard_world=1)                  # (what fmx_serve_open made the handle's config: the file's, everything else 0)
    obj._opened()
    obj.serve_only, obj.snap_info = True, info
    return obj


def release_cached_memory():
    """fmx_release_cached_memory: the placed arena fmx_destroy keeps per device for the next fmx_create goes back to the device"""
    load().fmx_release_cached_memory()


def batch_rule(task, learn_rate, collision_mass, requested=0):
    """the batch fmx_sgd_epoch would run with for rows of this collision mass (fmx_batch_rule; host arithmetic)"""
    bi = BatchInfo()
    rc = load().fmx_batch_rule(int(task), float(learn_rate), float(collision_mass), int(requested), C.byref(bi))
    if rc != 0:
        raise FmxError(rc, "fmx_batch_rule: bad argument")
    return bi


def place_layout(v_bytes, w_bytes):
    """(chunk_bytes, chunks, w_offset) of the arena fmx_create builds for tables of these sizes (fmx_place_layout; host arithmetic)"""
    ch, t, off = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    rc = load().fmx_place_layout(int(v_bytes), int(w_bytes), C.byref(ch), C.byref(t), C.byref(off))
    if rc != 0:
        raise FmxError(rc, "fmx_place_layout: bad argument")
    return ch.value, t.value, off.value


def shard_place(n, world, shard_hash, ids):
    """(owner, local_row) of every feature id under the library's ownership rule (host arithmetic, no device)"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    owner, local = np.zeros(len(ids), dtype=np.int32), np.zeros(len(ids), dtype=np.uint32)
    rc = load().fmx_shard_place(int(n), int(world), int(shard_hash), _ptr(ids), len(ids), _ptr(owner), _ptr(local))
    if rc != FMX_OK:
        raise FmxError(rc, "fmx_shard_place: bad argument")
    return owner, local


def shard_global(n, world, shard_hash, rank, local_rows):
    local_rows = np.ascontiguousarray(local_rows, dtype=np.uint32)
    ids = np.zeros(len(local_rows), dtype=np.uint32)
    rc = load().fmx_shard_global(int(n), int(world), int(shard_hash), int(rank), _ptr(local_rows), len(local_rows), _ptr(ids))
    if rc != FMX_OK:
        raise FmxError(rc, "fmx_shard_global: bad argument")
    return ids


def comm_unique_id():
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().fmx_comm_unique_id(buf)
    if rc != FMX_OK:
        raise FmxError(rc, load().fmx_last_error(None).decode())
    return buf.raw


class Group:
    """fmx_group: the feature shards of one model, driven by this one process (RCCL between devices, a local reduction
    when all shards share a device)."""

    def __init__(self, handles):
        self.lib = load()
        self.handles = list(handles)
        self._nq = {}                                # slot -> n_queries of the last set_row_queries
        arr = (H * len(self.handles))(*[h.h for h in self.handles])
        self.g = H()
        rc = self.lib.fmx_group_create(arr, len(self.handles), C.byref(self.g))
        if rc != FMX_OK:
            raise FmxError(rc, (self.lib.fmx_last_error(self.handles[0].h) or self.lib.fmx_last_error(None)).decode())

    def _chk(self, rc):
        if rc != FMX_OK:
            raise FmxError(rc, self.lib.fmx_group_last_error(self.g).decode())

    @property
    def G(self):
        """attribute groups (set_groups on the member handles)"""
        return self.handles[0].G

    def set_params(self, w0, w, v):
        """the full fm_model block for every shard, crossing PCIe once (fmx_group_set_params)"""
        h0 = self.handles[0]
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        v = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        self._chk(self.lib.fmx_group_set_params(self.g, float(w0), _ptr(w), _ptr(v) if h0.k > 0 else None))

    def upload_rows(self, slot, entries, row_ptr, target):
        """rows for every shard, crossing PCIe once; each shard filters its own features on its device (fmx_group_upload_rows)"""
        entries = np.ascontiguousarray(entries, dtype=ENTRY_DTYPE)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        target = None if target is None else np.ascontiguousarray(target, dtype=np.float32)
        self._chk(self.lib.fmx_group_upload_rows(self.g, slot, _ptr(entries) if len(entries) else None, _ptr(row_ptr), _ptr(target),
                                                 len(row_ptr) - 1, len(entries)))

    def upload_block_rows(self, slot, entries, row_ptr, target, relations, keep=False):
        """Handle.upload_block_rows for every shard (fmx_group_upload_block_rows_ex).  keep=True: main rows and blocks stay apart
        on every shard, each shard holding the block attributes it owns; keep=False: every shard joins the rows on the host."""
        args, alive = _block_args(entries, row_ptr, target, relations, keep)
        self._chk(self.lib.fmx_group_upload_block_rows_ex(self.g, slot, *args))
        return args[3]

    def sgd_epoch(self, slot, mode=SGD_MINIBATCH, apply=APPLY_DEFAULT, batch=0, w0_chunk=0, flags=0, bias_lag=0):
        opts = SgdOpts(mode, apply, batch, w0_chunk, flags, bias_lag)
        st = EpochStats()
        self._chk(self.lib.fmx_group_sgd_epoch(self.g, slot, C.byref(opts), C.byref(st)))
        return st

    def predict(self, slot, n_rows):
        out = np.zeros(n_rows, dtype=np.float64)
        self._chk(self.lib.fmx_group_predict(self.g, slot, _ptr(out)))
        return out

    def evaluate(self, slot):
        ev = Eval()
        self._chk(self.lib.fmx_group_evaluate(self.g, slot, C.byref(ev)))
        return ev

    def evaluate_ex(self, slot, link=LINK_LOGISTIC):
        """Handle.evaluate_ex over the shards; the predictions stay on the first shard's device (fmx_group_evaluate_ex)"""
        opts, ev = EvalOpts(link, 0), EvalEx()
        self._chk(self.lib.fmx_group_evaluate_ex(self.g, slot, C.byref(opts), C.byref(ev)))
        return ev

    def set_row_queries(self, slot, qid, n_queries=None):
        """Handle.set_row_queries; the ids go to the first shard's slot, where the targets live (fmx_group_set_row_queries)"""
        self._nq[slot] = _set_row_queries(self, self.lib.fmx_group_set_row_queries, self.g, slot, qid, n_queries)

    def evaluate_by_query(self, slot, link=LINK_LOGISTIC, per_query=False):
        """Handle.evaluate_by_query over the shards (fmx_group_evaluate_by_query)"""
        return _evaluate_by_query(self, self.lib.fmx_group_evaluate_by_query, self.g, slot, link, per_query, self._nq.get(slot))

    def evaluate_rank(self, slot, cutoffs, link=LINK_LOGISTIC, per_query=False):
        """Handle.evaluate_rank over the shards (fmx_group_evaluate_rank)"""
        return _evaluate_rank(self, self.lib.fmx_group_evaluate_rank, self.g, slot, cutoffs, link, per_query, self._nq.get(slot))

    # the posterior accumulator of a slot (fmx_post_*): MCMC's averaged predictions on the device
    def post_begin(self, slot, burn_in=5, eval_rows=0):
        opts = PostOpts(int(burn_in), int(eval_rows), 0, 0)
        self._chk(self.lib.fmx_group_post_begin(self.g, slot, C.byref(opts)))

    def post_accumulate(self, slot):
        """add the draw of the current parameters; the reference's metrics of the three vectors (PostStats.m[POST_*])"""
        st = PostStats()
        self._chk(self.lib.fmx_group_post_accumulate(self.g, slot, C.byref(st)))
        return st

    def post_evaluate_ex(self, slot, which=POST_ALL):
        ev = EvalEx()
        self._chk(self.lib.fmx_group_post_evaluate_ex(self.g, slot, int(which), C.byref(ev)))
        return ev

    def post_get(self, slot, which, n_rows):
        """(the sum over the draws -- or the last draw itself for POST_THIS -- as float64 [n_rows], the number of draws in it)"""
        out, draws = np.zeros(n_rows, dtype=np.float64), C.c_uint64(0)
        self._chk(self.lib.fmx_group_post_get(self.g, slot, int(which), _ptr(out), C.byref(draws)))
        return out, int(draws.value)

    def post_end(self, slot):
        self._chk(self.lib.fmx_group_post_end(self.g, slot))

    # ALS / MCMC over the shards ----------------------------------------------------------------
    def als_begin(self, train_slot):
        self._chk(self.lib.fmx_group_als_begin(self.g, train_slot))

    def als_sweep(self, w_lambda, v_lambda, alpha=1.0, w_mu=0.0, v_mu=0.0, do_sample=False, seed=0):
        opts, keep = self.handles[0]._als_opts(w_lambda, v_lambda, alpha, w_mu, v_mu, do_sample, seed)
        st = AlsStats()
        self._chk(self.lib.fmx_group_als_sweep(self.g, C.byref(opts), C.byref(st)))
        return st

    def als_moments(self):
        h0 = self.handles[0]
        out = np.zeros(2 + 2 * h0.G * (1 + h0.k), dtype=np.float64)
        self._chk(self.lib.fmx_group_als_moments(self.g, _ptr(out)))
        return out[0], out[1], out[2:].reshape(1 + h0.k, h0.G, 2)

    def als_end(self):
        self._chk(self.lib.fmx_group_als_end(self.g))

    # AdaGrad and FTRL over the shards (include/fmx.h "fmx_group_adapt_*"), mirroring Handle -------
    def adapt_begin(self, rule="adagrad", init_acc=0.0, learn_rate=0.0):
        """Handle.adapt_begin on every member, all or nothing (fmx_group_adapt_begin)"""
        if isinstance(rule, str):
            if rule != "adagrad":
                raise ValueError("adapt_begin: unknown rule %r (adagrad)" % (rule,))
            rule = ADAPT_ADAGRAD
        opts = AdaptOpts(int(rule), 0, float(init_acc), float(learn_rate))
        self._chk(self.lib.fmx_group_adapt_begin(self.g, C.byref(opts)))

    def adapt_epoch(self, slot, batch=0, w0_chunk=0):
        st = EpochStats()
        self._chk(self.lib.fmx_group_adapt_epoch(self.g, int(slot), int(batch), int(w0_chunk), C.byref(st)))
        return st

    def adapt_state_rows(self, ids):
        """(n_w[ids], n_v[:, ids]) for GLOBAL ids in any order, each read on the shard that owns it"""
        k = self.handles[0].k
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        nw = np.zeros(len(ids), dtype=np.float64)
        nv = np.zeros((len(ids), max(k, 1)), dtype=np.float64)
        self._chk(self.lib.fmx_group_adapt_get_state_rows(self.g, _ptr(ids), len(ids), _ptr(nw), _ptr(nv) if k > 0 else None))
        return nw, nv[:, :k].T.copy()

    def adapt_end(self):
        self._chk(self.lib.fmx_group_adapt_end(self.g))

    def ftrl_begin(self, alpha=0.0, beta=1.0, l1_w=0.0, l1_v=0.0, l2_w=0.0, l2_v=0.0, init_acc=0.0):
        """Handle.ftrl_begin on every member, all or nothing (fmx_group_ftrl_begin)"""
        opts = FtrlOpts(0, 0, float(alpha), float(beta), float(l1_w), float(l1_v), float(l2_w), float(l2_v), float(init_acc))
        self._chk(self.lib.fmx_group_ftrl_begin(self.g, C.byref(opts)))

    def ftrl_epoch(self, slot, batch=0, w0_chunk=0):
        st = EpochStats()
        self._chk(self.lib.fmx_group_ftrl_epoch(self.g, int(slot), int(batch), int(w0_chunk), C.byref(st)))
        return st

    def ftrl_state_rows(self, ids):
        """(z_w[ids], z_v[:, ids], n_w[ids], n_v[:, ids]) for GLOBAL ids in any order, each read on the shard that owns it"""
        k = self.handles[0].k
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        zw, nw = np.zeros(len(ids), dtype=np.float64), np.zeros(len(ids), dtype=np.float64)
        zv, nv = (np.zeros((len(ids), max(k, 1)), dtype=np.float64) for _ in range(2))
        self._chk(self.lib.fmx_group_ftrl_get_state_rows(self.g, _ptr(ids), len(ids), _ptr(zw), _ptr(zv) if k > 0 else None,
                                                         _ptr(nw), _ptr(nv) if k > 0 else None))
        return zw, zv[:, :k].T.copy(), nw, nv[:, :k].T.copy()

    def ftrl_end(self):
        self._chk(self.lib.fmx_group_ftrl_end(self.g))

    def param_sparsity(self):
        """fmx_sparsity of the whole model: the shards' counts summed (fmx_group_param_sparsity)"""
        sp = Sparsity()
        self._chk(self.lib.fmx_group_param_sparsity(self.g, C.byref(sp)))
        return sp

    # group checkpoints (include/fmx.h "fmx_group_checkpoint_*"): the unsharded handle's file, in global feature order
    def checkpoint_save(self, path, dense=False, model_only=False):
        """Handle.checkpoint_save of the model and the session the members hold between them: byte for byte the file one unsharded
        handle with the same state writes, loadable by a group of any shard count or by a Handle (fmx_group_checkpoint_save)"""
        opts, info = CkptOpts((CKPT_DENSE_STATE if dense else 0) | (CKPT_MODEL_ONLY if model_only else 0), 0), CkptInfo()
        self._chk(self.lib.fmx_group_checkpoint_save(self.g, None if path is None else os.fsencode(path), C.byref(opts), C.byref(info)))
        return info

    def checkpoint_load(self, path, model_only=False):
        """Handle.checkpoint_load on every member, each taking the rows it owns; sessions on all members or none
        (fmx_group_checkpoint_load)"""
        opts, info = CkptOpts(CKPT_MODEL_ONLY if model_only else 0, 0), CkptInfo()
        self._chk(self.lib.fmx_group_checkpoint_load(self.g, None if path is None else os.fsencode(path), C.byref(opts), C.byref(info)))
        return info

    def get_params(self, w=None, v=None):
        """the full model: every shard writes its own features into the same host arrays"""
        h0 = self.handles[0]
        w = np.zeros(h0.n, dtype=np.float64) if w is None else w
        v = np.zeros((h0.k, h0.n), dtype=np.float64) if v is None else v
        w0 = 0.0
        for h in self.handles:
            w0, w, v = h.get_params(w, v)
        return w0, w, v

    def close(self):
        if self.g:
            self.lib.fmx_group_destroy(self.g)
            self.g = H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
