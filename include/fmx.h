/*
 * fmx.h -- C-ABI of the MI355X-native Factorization Machine hot path (libfmx.so).
 *
 * This is the drop-in boundary for srendle/libfm's learner interface.  libFM has no plugin/FFI API;
 * its de-facto operator interface is `class fm_learn` (/root/reference/src/libfm/src/fm_learn.h:31-60)
 * driven by main() (/root/reference/src/libfm/libfm.cpp:271-434).  Each entry point below names the
 * reference interface it replaces.  The reference-side bindings (fm_learn subclasses calling these
 * functions) are shown in INTEGRATION.md and live in adapter/fm_learn_sgd_gpu.h (-method sgd, sgda) and
 * adapter/fm_learn_mcmc_gpu.h (-method als, mcmc); examples/fmx_demo.c uses the library from plain C.
 *
 * Conventions
 *   - plain C: opaque handle, POD structs, raw pointers and sizes; no C++/torch types cross the boundary.
 *   - every call returns FMX_OK (0) or a negative FMX_E_* code; fmx_last_error(h) gives the text.
 *     (The reference throws std::string / const char* caught in main, libfm.cpp:436-440; the adapter
 *      re-throws the text so that behaviour is preserved.)
 *   - host parameter layout is the reference's: w0 double, w[n] double, v[k][n] double FACTOR-major
 *     (fm_model.h:46-48, matrix.h:165-170: fm->v.value[0] is one contiguous k*n block).
 *   - host row layout is the reference's: one contiguous array of sparse_entry<float> {uint32 id; float value}
 *     in row order (fmatrix.h:34-42; Data.h:237-270 allocates exactly this) plus row offsets.
 *   - device layout (inside the library): V is FEATURE-major fp32, rows of k rounded up to 16 floats (one 64-byte
 *     sector; the lanes of a wavefront are mapped on the next power of two, those beyond the row take no part),
 *     so one gathered row is one coalesced segment (256 B at k=64, 448 B at k=100).  See DESIGN.md section 2.
 *   - single calling thread per handle (the reference is single threaded).
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails with FMX_E_HIP.
 */
#ifndef FMX_H_
#define FMX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMX_ABI_VERSION 11

enum {
  FMX_OK = 0,
  FMX_E_ARG = -1,       /* bad argument */
  FMX_E_HIP = -2,       /* HIP runtime error (no device, out of memory, launch failure) */
  FMX_E_STATE = -3,     /* call order violated (e.g. slot not uploaded) */
  FMX_E_UNSUPPORTED = -4
};

enum { FMX_TASK_REGRESSION = 0, FMX_TASK_CLASSIFICATION = 1 };   /* fm_learn.h:45-47 */

/* SGD update modes */
enum {
  FMX_SGD_SEQUENTIAL = 0,  /* batch = 1, rows in storage order: the reference trajectory
                              (fm_learn_sgd_element.h:56-67), exact to 1e-4 against the reference's final parameters.
                              Two forms (libfm_amd/csrc/fmx_seq_kernels.h), chosen per slot:
                              - conflict-free runs (FMX_STAT_SEQ_RUNS), where consecutive rows rarely share a feature (the
                                slot's runs average >= 16 rows): the slot is cut once into maximal runs of consecutive rows
                                that share no feature; inside a run the online loop IS one batch step with the bias coupled
                                example by example, and a run is one launch.  BASELINE's headline shape: ~26 M examples/s,
                                ~1000x the reference on one core (24-27 k examples/s);
                              - one example at a time on eight wavefronts (k <= 128) otherwise: ~360 k examples/s whatever
                                the shape -- 14x the reference where its model misses the caches, 30x SLOWER than it where
                                the model is cache-resident (configs[0]: 11 M examples/s on the CPU).
                              The parity mode; the adapters default to MINIBATCH. */
  FMX_SGD_MINIBATCH = 1,   /* restated batch rule (oracle/fm_oracle.h fmo_sgd_epoch_minibatch):
                              partial sums -> [all-reduce] -> w0 micro-chunks + multipliers -> scatter-add */
  FMX_SGD_HOGWILD = 2      /* fused single pass per example (gather, predict, update in registers);
                              asynchronous between wavefronts; single device only.  An update becomes visible when its wavefront
                              retires, so the ~5 000 rows in flight act like a batch: on rows with frequent features (collision mass C,
                              see fmx_sgd_opts::batch) it diverges where learn_rate * curvature * 5 120 * C > 2 -- fmx_epoch_stats
                              reports the gain (batch_used = rows in flight) and FMX_STAT_UNSTABLE, FMX_FLAG_REJECT_UNSTABLE refuses */
};

enum {
  FMX_APPLY_DEFAULT = 0,   /* MINIBATCH: SEGMENTED, HOGWILD: STORE */
  FMX_APPLY_ATOMIC = 1,    /* one wavefront per example, fp32 atomic scatter-add of the per-occurrence deltas
                              (reads of a feature that collides inside the batch may see a partial update) */
  FMX_APPLY_STORE = 2,     /* one wavefront per example, plain read-modify-write stores (colliding ids in a
                              batch lose updates; exact when a batch has no repeated feature) */
  FMX_APPLY_SEGMENTED = 3, /* MINIBATCH only: entries pre-bucketed per (batch, feature); one owner per touched
                              row, no atomics, exactly the batch rule of oracle/fm_oracle.h (deterministic) */
  FMX_APPLY_FUSED = 4      /* MINIBATCH only, implies FMX_FLAG_BIAS_LAG: the SAME batch rule in one pass over HBM.  The rule
                              takes every sum and gradient from batch-start parameters, so a feature that occurs once in its
                              batch is gathered, used and written back by its own example's wavefront (V read once, written
                              once -- the algorithmic minimum); the features that occur more than once in the batch are
                              finished by the segmented kernel from the factor sums their examples leave behind.
                              Deterministic; the result of FMX_APPLY_SEGMENTED with the same bias_lag to fp32 rounding. */
};

typedef struct fmx_context_s *fmx_handle;

/* replaces the fields main() writes into fm_model / fm_learn (libfm.cpp:245-256, 294-309, 366-404) */
typedef struct fmx_config {
  uint64_t num_attribute;   /* fm_model::num_attribute (global n)            fm_model.h:51 */
  int32_t  num_factor;      /* fm_model::num_factor (k), 0 .. 1024           fm_model.h:54 */
  int32_t  k0;              /* use bias                                       fm_model.h:53 */
  int32_t  k1;              /* use 1-way interactions                         fm_model.h:53 */
  int32_t  task;            /* fm_learn::task                                 fm_learn.h:45 */
  double   reg0, regw, regv;/* fm_model::reg0/regw/regv                       fm_model.h:56-57 */
  double   learn_rate;      /* fm_learn_sgd::learn_rate                       fm_learn_sgd.h:42 */
  double   min_target;      /* fm_learn::min_target (of the TRAIN set)        libfm.cpp:295-296 */
  double   max_target;
  int32_t  device;          /* HIP device ordinal; -1 = current device */
  int32_t  shard_rank;      /* feature sharding: this handle owns the features j with            */
  int32_t  shard_world;     /*   owner(j) == shard_rank  (shard_world = 1: unsharded)            */
  int32_t  shard_hash;      /* 0: owner(j) = j mod shard_world, local row j div shard_world.
                               1: owner(j) = p(j) mod shard_world, local row p(j) div shard_world with p a fixed pseudo-random
                                  PERMUTATION of [0, num_attribute) (4-round Feistel network, cycle-walked; north_star:
                                  "row-sharded by feature-id hash"): balanced whatever the structure of the ids, still a dense
                                  local table, and invertible, so the shard knows its features' global ids. */
  int32_t  place_candidates;/* placement of the parameter tables (see fmx_create).  0 = default: tables of >= 2 GiB are built from 1 GiB
                               chunks of TWO memory classes of the device, found by probing (transient pool of at most 3 tables' worth
                               of chunks + 64 GiB, never more than half of the free memory); tables of 256 MB .. 2 GiB: best of 2 candidate
                               allocations.  1 = first fit: plain allocations, no probe, no transient memory.  2 .. 6 = the bound of the
                               transient pool in tables' worth (big tables) / the number of candidates (small ones) */
  uint32_t als_split_min;   /* ALS / MCMC: dependency levels with at least this many entries update {e, q} as a row-ordered stream
                               (the split step) instead of inside the fused draw.  0 = library default (65536),
                               1 = every level, 0xFFFFFFFF = never */
  uint32_t exchange_runs;   /* several GPUs over RCCL: a batch's partial sums are exchanged in this many runs of rows, the all-reduce of
                               one run travelling while the next is summed.  0 = default (4), 1 = one all-reduce per batch */
  uint32_t exchange_algo;   /* several GPUs: how the per-batch exchange of the partial sums is carried.  FMX_EXCHANGE_ALLREDUCE (0): one
                               all-reduce (ncclAllReduce; RCCL picks ring / tree).  FMX_EXCHANGE_RS_AG (1): reduce-scatter + all-gather --
                               on a fully connected xGMI node every GPU reduces its 1/P slice over its P - 1 direct links and broadcasts it
                               back over the same links, instead of a ring that is bound by ONE link.  Pieces whose length
                               is not a multiple of the shard count fall back to the all-reduce.  Same sums either way (the loopback exchange
                               of shards sharing a device adds in the same order: bit-identical). */
} fmx_config;
#define FMX_EXCHANGE_ALLREDUCE 0u
#define FMX_EXCHANGE_RS_AG     1u

typedef struct fmx_sgd_opts {
  int32_t  mode;            /* FMX_SGD_* */
  int32_t  apply;           /* FMX_APPLY_* (MINIBATCH and HOGWILD) */
  uint32_t batch;           /* MINIBATCH: rows per minibatch.  0 = library default: 262144, CUT to the largest power of two that
                               keeps the batch rule stable on THIS data set: learn_rate * curvature * batch * C <= 1, C = the
                               collision mass of the slot's rows (fmx_sgd_batch_info).  The rule freezes every parameter for one
                               batch; two examples of a batch that share features push those in the same direction from the
                               same stale state, so the step along "what the rows have in common" is learn_rate * batch * C where
                               the reference (batch 1, fm_sgd.h:33-51) takes `batch` small steps.  Uniform ids over 1e8 features:
                               C = 1e-5, no cut; Criteo-shaped rows (100-id fields, Zipf heads): C = 1, batch 256 at
                               learn_rate 0.01; never below 32).  An explicit batch is honoured (fmx_epoch_stats::status reports FMX_STAT_UNSTABLE;
                               with FMX_FLAG_REJECT_UNSTABLE the call fails with FMX_E_ARG instead of training).
                               HOGWILD: rows per launch during which w0 is frozen (macro-batch), 0 = 262144 */
  uint32_t w0_chunk;        /* w0 micro-chunk of the bias recurrence; 0 = library default (fmx_default_w0_chunk): the largest power
                             * of two <= FMX_W0_CHUNK_CAP with learn_rate * chunk * curvature <= 1 (curvature 1 for regression, 1/4
                             * for classification).  The reference moves w0 after every example (fm_sgd.h:34-37); a chunk is one
                             * batch step of size learn_rate * chunk on the bias and oscillates when that product exceeds
                             * 2 / curvature -- and the smaller the chunk, the closer the rule's bias follows the reference's path
                             * (chunk 1 IS the reference's bias path).  fmx_epoch_stats::w0_chunk_used reports the value used. */
  uint32_t flags;           /* FMX_FLAG_* */
  uint32_t bias_lag;        /* with FMX_FLAG_BIAS_LAG / FMX_APPLY_FUSED: the multipliers of batch b use the bias as it was after
                               the recurrence of batch b - bias_lag (0 = 1 = the bias of the batch start).  fmx_sgd_epoch with
                               FMX_APPLY_FUSED honours 1..4: with bias_lag >= 2 the one-workgroup recurrence of a batch hides
                               under the next launches instead of sitting between them.  The split step
                               (fmx_sgd_partial / fmx_sgd_finish) implements 1 only.
                               Oracle: fmo_sgd_epoch_minibatch_ex(..., bias_lag). */
} fmx_sgd_opts;

#define FMX_FLAG_TIME_MAIN_KERNEL 1u  /* bracket every launch of the dominant kernel with HIP events */
#define FMX_FLAG_PIPELINE 4u          /* fmx_group_sgd_epoch: gather the sums of batch b+1 BEFORE the update of batch b lands, so that
                                         their exchange runs under that update (one batch stale; oracle
                                         fmo_sgd_epoch_minibatch_pipelined) */
#define FMX_FLAG_REJECT_UNSTABLE 8u    /* MINIBATCH: fail with FMX_E_ARG when learn_rate * curvature * batch * C > 2 (the batch rule diverges
                                         there; tests/test_oracle_stability.py) instead of training -- for an explicit batch, and for batch 0
                                         when even the library's floor of 32 rows is unstable (rows with C in the hundreds: the message then
                                         names FMX_SGD_SEQUENTIAL / a lower learn_rate, not "batch 0") */
#define FMX_FLAG_KEEP_WSIDE 32u        /* FMX_APPLY_FUSED on an unsharded handle: this epoch keeps the slot's WEIGHT SIDE STREAM current -- per entry
                                         the new w_j where the entry is the last occurrence of its feature in the slot and its own example
                                         updates it, "gather" otherwise (+128 coalesced bytes per example, 4 bytes per entry of memory).
                                         fmx_predict / fmx_evaluate on that slot then take those weights out of a 4-byte stream instead of one
                                         64-byte fabric request each (fm_model.h:110-115's loop over w: a third of the pass's requests) until
                                         anything else changes w.  For learners that evaluate the train set after every epoch, as
                                         fm_learn_sgd_element::learn does (fm_learn_sgd_element.h:69-70); same numbers either way */
#define FMX_FLAG_EVENT_SYNC 16u        /* FMX_APPLY_FUSED at batches >= 32768: order the launch stream and the recurrence's side stream with
                                         events (four queue packets per batch) instead of the device-side hand-off (bias slots that start as
                                         "pending" + a completion counter: DESIGN.md section 4).  Same numbers either way; the environment
                                         variable FMX_HANDOFF=0 at fmx_create selects events for every epoch of the handle */
#define FMX_FLAG_BIAS_LAG 2u          /* MINIBATCH: the multipliers of a batch use the w0 of the batch START; w0 itself still
                                         advances through the micro-chunk recurrence, which then runs on a side stream
                                         overlapped with the next batch (oracle: fmo_sgd_epoch_minibatch_ex, bias_lag = 1) */

typedef struct fmx_epoch_stats {
  uint64_t rows;            /* examples processed */
  uint64_t batches;
  double   device_seconds;  /* HIP-event time of the epoch's kernels on the handle's stream */
  double   main_kernel_seconds; /* HIP-event time summed over launches of the dominant kernel only */
  uint64_t main_kernel_launches;
  uint32_t max_feature_count; /* MINIBATCH with the segmented update: occurrences of the most frequent feature inside one
                               * batch (the longest segment k_apply_seg sums) */
  uint32_t batch_used;      /* MINIBATCH: rows per batch this epoch ran with (the resolved fmx_sgd_opts::batch) */
  uint64_t deferred_features; /* FMX_APPLY_FUSED: (batch, feature) pairs finished by the segmented kernel, summed over the
                               * epoch's batches (features occurring more than once in their batch; the rest was one pass) */
  double   collision_mass;  /* C of the slot's rows: the mean over pairs of DIFFERENT rows of sum_j |x_ej| |x_e'j| = the expected
                               number of features two rows share (value-weighted) */
  double   batch_gain;      /* learn_rate * curvature * batch_used * C (curvature 1 regression, 1/4 classification): the batch
                               rule follows the reference's online loop for <= 1, degrades above and diverges beyond ~2 */
  uint32_t status;          /* FMX_STAT_*; FMX_STAT_WARN_MASK picks the bits that say something about the rule, the others say how the epoch ran */
  uint32_t w0_chunk_used;   /* MINIBATCH / HOGWILD: the micro-chunk of the bias recurrence this epoch ran with */
  double   setup_seconds;   /* host wall-clock this call spent on ONE-TIME work for the slot (not part of device_seconds): the rows' collision mass
                               and the bucketing of the entries by (batch, feature) -- the segments, masks and lists the MINIBATCH forms
                               walk; libFM never shuffles (fm_learn_sgd_element.h:56), so they are built once per (slot, batch size).
                               0 when everything was cached */
  double   phase_seconds[4]; /* fmx_group_sgd_epoch / feature shards with FMX_FLAG_TIME_MAIN_KERNEL, HIP events on the first local
                               shard's compute stream, summed over the epoch's batches: [0] partial sums of the batch (fmx_sgd_partial),
                               [1] exposed exchange (end of the sums -> the reduced sums are available: what the wire costs beyond
                               what the sums hid), [2] update (multipliers, recurrence hand-off, write-back of the local rows),
                               [3] unused.  Zero on a single unsharded handle. */
} fmx_epoch_stats;

#define FMX_STAT_BATCH_CUT 1u   /* batch = 0 resolved below the 262144 default because of the rows' collision mass */
#define FMX_STAT_UNSTABLE  2u   /* batch_gain > 2: an explicit batch the rule is not stable at on this data */
#define FMX_STAT_WARN_MASK (FMX_STAT_BATCH_CUT | FMX_STAT_UNSTABLE)
/* (ABI 7) how the epoch's bias recurrences and stream ordering actually ran -- same numbers in every form; for tests and diagnosis: */
#define FMX_STAT_SCAN_PIT      4u  /* at least one batch's recurrence was solved parallel in time (k_scan_pit) */
#define FMX_STAT_SCAN_SERIAL   8u  /* at least one ran as the one-wavefront chain (k_scan1 / k_scan / the small-batch form) */
#define FMX_STAT_SCAN_FALLBACK 16u /* a grid-wide exchange of k_scan_pit ran into its bound (a workgroup was not resident: the device is
                                      shared with work the library cannot see); one workgroup evaluated that batch's chain serially -- the
                                      result is still the rule's -- and the handle uses the one-wavefront chain from now on */
#define FMX_STAT_EVENT_SYNC    32u /* the launch stream and the recurrence's side stream were ordered by events, not by the device-side
                                      hand-off: requested (FMX_FLAG_EVENT_SYNC / FMX_HANDOFF=0), bias_lag 1, or the handle found that its two
                                      streams do not run concurrently (serialised dispatch: a counter-collecting profiler, AMD_SERIALIZE_KERNEL) */
/* (ABI 11) bit 128u is reserved and never set: it was FMX_STAT_XCD_RESIDENT, the status of an experiment that has been removed */
#define FMX_STAT_SEQ_RUNS 256u     /* FMX_SGD_SEQUENTIAL ran as conflict-free runs: maximal runs of consecutive rows that share no feature, each one
                                      batch step with the bias recurrence coupled example by example -- the same trajectory as the online loop.
                                      fmx_epoch_stats::batches = the number of runs.  (A run whose workgroups never all arrive -- a shared or
                                      partitioned device -- takes no step for the rows concerned: FMX_E_HIP + FMX_STAT_HANDOFF_TIMEOUT, and the
                                      handle takes two launches per run from then on.) */
#define FMX_STAT_SMALL_ONE 512u    /* small batches (< 1 025 rows) of the one-pass minibatch rule ran as ONE launch per batch across all dies: examples,
                                      deferred features and the bias recurrence exchange through tagged slots (libfm_amd/csrc/fmx_small_kernels.h) */
#define FMX_STAT_HANDOFF_TIMEOUT 64u /* a device-side hand-off wait ran into its bound all the same: the examples concerned took NO step
                                      (multiplier 0; a recurrence that never saw its batch handed the bias on unchanged), every parameter is a
                                      valid number, the call returns FMX_E_HIP with this status set, and the handle orders by events from now on */
/* (ABI 9) which kernels FMX_SGD_SEQUENTIAL ran (libfm_amd/csrc/fmx_seq_kernels.h, fmx_online_kernels.h) -- the same trajectory in every form; for
   tests and diagnosis.  The environment of fmx_create picks among them: FMX_SEQ_ROWS=0, FMX_SEQ_WG=0, FMX_SEQ_RUNS_FUSED=0, FMX_SEQ_RUNS_ONE=0;
   FMX_SEQ_RUNS (0: never runs, 1: always) is read at every epoch: */
#define FMX_STAT_SEQ_ENTRIES   1024u /* entry by entry on one wavefront (k_sequential): the whole slot, or a row that repeats an id inside runs */
#define FMX_STAT_SEQ_WG        2048u /* one example at a time on eight wavefronts (k_sequential_wg) */
#define FMX_STAT_SEQ_ROWS      4096u /* one example at a time on one wavefront, a row at a time (k_sequential_rows) */
#define FMX_STAT_RUN_ONE       8192u /* at least one conflict-free run as ONE launch (k_run_fused) */
#define FMX_STAT_RUN_TWO      16384u /* at least one run as two launches (k_rowsums + k_run_apply) */
#define FMX_STAT_RUN_THREE    32768u /* at least one run as three launches (k_rowsums + the recurrence on its own + k_apply) */
#define FMX_STAT_WSTREAM     131072u /* at least one batch of the one-pass minibatch epoch read the linear weights of the slot's once-only features from
                                        the slot's packed training-side stream instead of gathering them (FMX_WTRAIN=0 at fmx_create: never) */
#define FMX_STAT_WEIGHTED     65536u /* fmx_adapt_epoch / fmx_ftrl_epoch on a slot with row weights (fmx_set_row_weights): every batch's recurrence ran as
                                        k_scan_weighted, a one-wavefront chain (FMX_STAT_SCAN_SERIAL is set with it, FMX_STAT_SCAN_PIT never) */

/* what fmx_sgd_epoch would use for `batch` on this slot (no training): the rows' collision mass (computed once per slot on the
 * device: one histogram pass over the entries), the resolved batch and its gain.  opts may be NULL (= batch 0). */
typedef struct fmx_batch_info {
  double   collision_mass;
  double   batch_gain;
  uint32_t batch;
  uint32_t status;          /* FMX_STAT_* */
} fmx_batch_info;

/* what fm_learn::evaluate_regression / evaluate_classification compute (fm_learn.h:113-153) */
typedef struct fmx_eval {
  double   rmse;            /* regression: sqrt(sum err^2 / N) with clamped predictions */
  double   mae;             /* regression */
  double   accuracy;        /* classification: sign agreement (p>=0 vs y>=0) */
  double   device_seconds;
  uint64_t rows;
  uint32_t flags;           /* FMX_EVAL_WSIDE: the linear weights came out of the slot's weight side stream (FMX_FLAG_KEEP_WSIDE) */
  uint32_t reserved;
} fmx_eval;
#define FMX_EVAL_WSIDE 1u

/* ---- lifetime ------------------------------------------------------------------------------- */
/* replaces: fm_model fm; fm.init() allocation (fm_model.h:91-99) + new fm_learn_* (libfm.cpp:271-293)
 * Parameter tables are PLACED (fmx_config::place_candidates): on MI355X physical memory falls into three classes of ~96 GB (what one
 * would expect of the three ranks of the 12-high HBM3E stacks) and random row traffic inside ONE class runs at 4.9 TB/s, spread over
 * two at 6.1 (scripts/ubench/placement_classes.hip) -- a plain allocation lands in one class or straddles two by
 * luck, which moved the training step by 10-20 % from process to process.  fmx_create therefore takes 1 GiB chunks (hipMemCreate),
 * classifies each by probing it together with a reference chunk, maps chunks of two classes alternately into one virtual range, puts
 * V at its start and w across a chunk boundary behind it, and returns the chunks it does not need.  fmx_place_info reports what it
 * found.  If the virtual-memory API is unavailable the tables are plain allocations (best of two candidates). */
/* Environment read by fmx_create (A/B knobs; none changes a result beyond fp32 rounding): FMX_HANDOFF=0 (events instead of the device-side
 * bias hand-off), FMX_SCAN=serial (the bias recurrence as a one-wavefront chain instead of parallel in time), FMX_ARENA_CACHE=0 (no arena
 * kept for the next handle), FMX_MULTI_FILL=8..32 (entries per 32-slot round the short-row shard kernels group examples for; default 24). */
int fmx_create(const fmx_config *cfg, fmx_handle *out);
int fmx_destroy(fmx_handle h);
/* fmx_destroy keeps ONE placed arena per device alive for the next fmx_create on that device (which then takes it over without
 * probing: fmx_place_info::pool = 0) -- the memory of the largest arena destroyed so far stays allocated until it is reused, this call
 * returns it, ANY device allocation of the library runs short of memory (it is then given back and the allocation retried once), or
 * the process ends.  Other processes on the device do not see it as free before that.  FMX_ARENA_CACHE=0 in the environment turns this off. */
int fmx_release_cached_memory(void);
/* how the parameter tables of a handle were placed */
typedef struct fmx_place_info {
  int32_t  method;          /* 0 = plain allocations (small tables / first fit), 1 = best of several candidate allocations,
                               2 = arena of chunks from two memory classes */
  uint32_t chunks;          /* method 2: 1 GiB chunks the arena holds */
  uint32_t per_class[2];    /*           ... of the first / the second class (equal up to one = balanced) */
  uint32_t pool;            /*           chunks taken and probed to find them (the others were returned before fmx_create ended) */
  uint32_t classes_seen;    /*           memory classes seen among the pool */
  double   seconds;         /* host time of the placement */
} fmx_place_info;
int fmx_get_place_info(fmx_handle h, fmx_place_info *out);
/* the layout of that arena for tables of v_bytes and w_bytes (host arithmetic, no device needed): V at offset 0, w at *w_offset --
 * centred on a chunk boundary --, *chunks chunks of *chunk_bytes */
int fmx_place_layout(uint64_t v_bytes, uint64_t w_bytes, uint64_t *chunk_bytes, uint32_t *chunks, uint64_t *w_offset);
/* text of the last error on this handle (h may be NULL: last creation error). Never NULL. */
const char *fmx_last_error(fmx_handle h);
int fmx_abi_version(void);
/* fmx_sgd_opts::w0_chunk = 0 resolves to this (host arithmetic; task = FMX_TASK_*): the largest power of two <= FMX_W0_CHUNK_CAP with
 * learn_rate * chunk * curvature <= 1.  Until ABI 5 the cap was 256; the reference advances the bias per example (fm_sgd.h:34-37) and the
 * finer recurrence ends 17x closer to its bias path at the bench shape. */
#define FMX_W0_CHUNK_CAP 32
uint32_t fmx_default_w0_chunk(double learn_rate, int task);
/* number of visible HIP devices (0 when none / no driver) */
int fmx_device_count(void);

/* ---- parameters: the fm_model block (fm_model.h:46-48) -------------------------------------- */
/* host -> device. w may be NULL when k1 == 0, v may be NULL when k == 0.  In sharded mode the FULL
 * arrays are passed and the handle keeps its own features. */
int fmx_set_params(fmx_handle h, double w0, const double *w, const double *v);
/* device -> host, same layout; after learn() the host fm_model must hold the result (libfm.cpp:431-434).
 * Sharded mode: only this shard's features are written, the rest of w / v is left untouched. */
int fmx_get_params(fmx_handle h, double *w0, double *w, double *v);
/* device-side fill for workloads too large to stage through the host (bench.py):
 * w0 = 0, w = 0, v[f][j] = mean + fmo_init_value(seed, j, f, stdev) -- a counter-hash uniform with unit
 * variance (same definition as oracle/fm_oracle.c), NOT the reference's rand() stream (fm_model.h:96). */
int fmx_init_params(fmx_handle h, double init_mean, double init_stdev, uint64_t seed);
/* selected rows of the parameter block (spot checks at sizes where the full fm_model does not fit the host):
 * for i < count: w_out[i] = w[ids[i]], v_out[i*num_factor + f] = v[f][ids[i]].  Sharded handles accept only their
 * own features. */
int fmx_get_param_rows(fmx_handle h, const uint32_t *ids, uint32_t count, double *w_out, double *v_out);
/* fm_model::saveModel / loadModel (fm_model.h:132-190; `-save_model`, `-load_model`, libfm.cpp:258-269, 431-434): the
 * reference's text file ("#global bias W0", "#unary interactions Wj", "#pairwise interactions Vj,f": one line per feature,
 * its factors separated by blanks; doubles as an ostream prints them).  The device table is feature-major -- the file's own
 * order -- so it is streamed in row chunks without ever building the fp64 factor-major block on the host.
 * fmx_load_model fails with FMX_E_ARG "malformed model file" where loadModel returns 0 (wrong number of factors per line,
 * truncated file); a k = 1 file, which the reference's splitString cannot read back (fm_model.h:195-205), is accepted.
 * Shards: every shard may load the same file (it keeps its own features); saving a sharded model goes through fmx_get_params. */
int fmx_save_model(fmx_handle h, const char *path);
int fmx_load_model(fmx_handle h, const char *path);
/* the scalar bias alone (cheap; used between minibatches by multi-process drivers) */
int fmx_get_w0(fmx_handle h, double *w0);

/* ---- attribute groups (`-meta`): DataMetaInfo::attr_group, src/libfm/src/Data.h:39-46, loaded by
 * loadGroupsFromFile (:85-97).  group_of_feature[num_attribute] (host, ids < num_groups), indexed by GLOBAL feature id
 * (a feature shard keeps the entries of its own features).
 * Groups select the prior of a coordinate in ALS / MCMC (w_lambda(g), w_mu(g), v_lambda(g,f), v_mu(g,f);
 * fm_learn_mcmc.h:464-466, :583-585) and the learned regularisation in SGDA (reg_w(g), reg_v(g,f);
 * fm_learn_sgd_element_adapt_reg.h:155-166); plain SGD ignores them like the reference does.
 * NULL or num_groups <= 1 goes back to one group.  Not allowed while an ALS / SGDA session is open. */
int fmx_set_groups(fmx_handle h, const uint32_t *group_of_feature, uint32_t num_groups);

/* ---- rows: what Data::load produces (Data.h:237-270) ---------------------------------------- */
/* uploads a data set into `slot` (0..FMX_MAX_SLOTS-1).  entries: {uint32 id; float value}[nnz] in row
 * order (the buffer Data::load allocates), row_ptr: uint64[n_rows+1] prefix sums of sparse_row::size,
 * target: float[n_rows] (already rewritten to +-1 for classification, libfm.cpp:302-306); may be NULL
 * for predict-only slots.  ids must be < num_attribute (asserted by the reference, fm_model.h:112). */
#define FMX_MAX_SLOTS 8
int fmx_upload_rows(fmx_handle h, int slot, const void *entries, const uint64_t *row_ptr,
                    const float *target, uint32_t n_rows, uint64_t nnz);
/* block-structured data (`-relation`; RelationData / RelationJoin, src/libfm/src/relation.h:32-60, loaded at
 * libfm.cpp:172-196): every main row c is joined with row data_row_to_relation_row[c] of each relation block, whose
 * attribute ids start at attr_offset (libfm.cpp:213-216).  The rows are expanded ON THE DEVICE into one CSR
 * (main entries, then the blocks in order) so that the slot behaves like any other; the learners then compute what
 * the reference's per-block caches compute (fm_learn_mcmc.h:478-527, 734-790, 849-909) on the same design matrix.
 * At most 8 relations.  A feature shard (shard_world > 1) joins the rows on the host and keeps its own features
 * (FMX_BLOCKS_EXPAND); to keep the blocks apart on feature shards, upload through fmx_group_upload_block_rows_ex. */
typedef struct fmx_relation {
  const void     *entries;                    /* the block's own rows: sparse_entry<float>[nnz], ids local to the block */
  const uint64_t *row_ptr;                    /* [n_rows + 1] */
  uint32_t        n_rows;                     /* RelationData::num_cases */
  uint32_t        reserved;
  uint64_t        nnz;
  const uint32_t *data_row_to_relation_row;   /* [n_rows of the MAIN data]; RelationJoin, relation.h:56 */
  uint64_t        attr_offset;                /* RelationData::attr_offset */
} fmx_relation;
int fmx_upload_block_rows(fmx_handle h, int slot, const void *entries, const uint64_t *row_ptr, const float *target,
                          uint32_t n_rows, uint64_t nnz, const fmx_relation *relations, uint32_t n_relations);
/* the same with a choice of representation:
 *   FMX_BLOCKS_EXPAND  the joined rows are materialised on the device (what fmx_upload_block_rows does): any learner runs on
 *                      them, at the data volume of the joined table;
 *   FMX_BLOCKS_KEEP    main rows and blocks stay apart, as in the reference: fmx_predict / fmx_evaluate add the block rows'
 *                      sums through the mapping, and fmx_als_* sweeps a block's attributes through per-block-row caches
 *                      (fm_learn_mcmc.h:478-527 cache set-up, :734-790 draw_w_rel, :849-909 draw_v_rel, restated): a block
 *                      attribute costs its column in the BLOCK plus two passes over the main rows per block and coordinate
 *                      family, not a column of the joined table.  ALS / MCMC and predict only (the reference's SGD learners
 *                      reject relations too, fm_learn_sgd.h:61-63).  A feature shard refuses it here (the sweep needs the
 *                      group's global view): fmx_group_upload_block_rows_ex keeps the blocks apart on shards. */
#define FMX_BLOCKS_EXPAND 0u
#define FMX_BLOCKS_KEEP 1u
int fmx_upload_block_rows_ex(fmx_handle h, int slot, const void *entries, const uint64_t *row_ptr, const float *target,
                             uint32_t n_rows, uint64_t nnz, const fmx_relation *relations, uint32_t n_relations, uint32_t flags);
/* synthetic one-hot field rows generated on the device (bench workload; same
 * definition as oracle/fm_oracle.c fmo_synth_rows): rows row0 .. row0+n_rows-1 */
int fmx_synth_rows(fmx_handle h, int slot, uint64_t seed, uint64_t row0, uint32_t n_rows, uint32_t nnz);
/* the same with a choice of id distribution:
 *   FMX_SYNTH_UNIFORM  uniform ids within each of the nnz fields (fmx_synth_rows)
 *   FMX_SYNTH_CRITEO   BASELINE configs[2] / SURVEY section 8d "Criteo-shaped": the first 13 fields ("numeric", binned) hold at
 *                      most 100 ids each with a geometric frequency profile, the other nnz - 13 fields share the remaining ids
 *                      equally and draw them Zipf(s = 1.05) (inverse-CDF of the continuous power law); labels +-1 with a 1:3
 *                      imbalance.  Needs nnz > 13 and num_attribute >= 1300 + (nnz - 13). */
#define FMX_SYNTH_UNIFORM 0u
#define FMX_SYNTH_CRITEO 1u
int fmx_synth_rows_ex(fmx_handle h, int slot, uint64_t seed, uint64_t row0, uint32_t n_rows, uint32_t nnz, uint32_t shape);
int fmx_free_rows(fmx_handle h, int slot);
/* copies a slot back to the host (tests / debugging): sizes via fmx_rows_info first.  Sharded handles return
 * their LOCAL rows (kept entries only, ids = local row of the feature on this shard). Any pointer may be NULL. */
int fmx_rows_info(fmx_handle h, int slot, uint32_t *n_rows, uint64_t *nnz);
int fmx_download_rows(fmx_handle h, int slot, void *entries, uint64_t *row_ptr, float *target);
/* (tests / debugging) the slot's training-side weight stream as its first one-pass epoch left it: *singles = entries whose feature occurs
 * exactly once in the slot (and whose row the one-pass kernel keeps in registers), *kept = 1 when the stream was built for them
 * (FMX_STAT_WSTREAM).  Both 0 before that epoch.  Either pointer may be NULL. */
int fmx_wtrain_info(fmx_handle h, int slot, uint64_t *singles, int *kept);

/* ---- host-side reader of libFM's text format (no device, no handle) ----------------------------------------
 * Data::load, text branch (src/libfm/src/Data.h:180-285): lines "target id:value id:value ...", blank lines and lines
 * starting with '#' skipped, leading / trailing blanks and tabs allowed, anything else rejected with the reference's
 * message ("cannot parse line ..." / "unable to open ...") in `err`.  The buffers are malloc'ed; release them with
 * fmx_free_host_rows.  They are exactly what fmx_upload_rows takes. */
typedef struct fmx_host_rows {
  void     *entries;        /* sparse_entry<float>[nnz] */
  uint64_t *row_ptr;        /* [n_rows + 1] */
  float    *target;         /* [n_rows] */
  uint32_t  n_rows;
  uint32_t  num_feature;    /* largest id + 1 (Data.h:226-228) */
  uint64_t  nnz;
  float     min_target, max_target;   /* Data.h:205-206 */
  uint32_t  flags;          /* FMX_HOST_PINNED: the buffers are page-locked (hipHostMalloc) */
  uint32_t  reserved;
} fmx_host_rows;
#define FMX_HOST_PINNED 1u
int  fmx_read_libsvm(const char *path, fmx_host_rows *out, char *err, size_t err_len);
/* Data::load, binary branch (src/libfm/src/Data.h:119-178): <prefix>.x + <prefix>.y as written by tools/convert.cpp:137-200
 * (LargeSparseMatrix::saveToBinaryFile, src/util/fmatrix.h:44-50,121-140; DVector::saveToBinaryFile, matrix.h:344-358), or --
 * when only the transpose is on disk, which is what als / mcmc runs keep (libfm.cpp:143-147, tools/transpose.cpp) --
 * <prefix>.xt + <prefix>.y, from which the rows are rebuilt; the older .data / .datat / .target names work too.
 * With a HIP device present the buffers are page-locked, so fmx_upload_rows moves them by DMA while it checks the ids. */
int  fmx_read_binary(const char *prefix, fmx_host_rows *out, char *err, size_t err_len);
void fmx_free_host_rows(fmx_host_rows *rows);

/* ---- fm_model::predict over a data set (fm_model.h:105-127 via fm_learn.h:63-65) -------------- */
/* raw y-hat per row (no clamp / sigmoid: fm_learn_sgd::predict applies those on the host,
 * fm_learn_sgd.h:80-87).  out: double[n_rows]. Sharded handles return the PARTIAL sums only. */
int fmx_predict(fmx_handle h, int slot, double *out);
/* fm_learn::evaluate (fm_learn.h:93-153) fused on the device */
int fmx_evaluate(fmx_handle h, int slot, fmx_eval *out);

/* ---- exact AUC and log loss of a slot, reduced on the device -----------------------------------
 * fm_learn::evaluate knows RMSE / MAE and sign accuracy only (fm_learn.h:113-153); for `-task c` on imbalanced labels the
 * metrics people read are AUC and log loss.  fmx_evaluate_ex scores the slot like fmx_evaluate (one pass at the predict
 * roofline, kept `-relation` blocks and the weight side stream included) and reduces on the device.  With p_i the fp32 raw
 * y-hat fmx_predict returns for row i (w0 + rest, no clamp) and s_i = +1 if target_i >= 0, else -1 (the sign rule of fm_learn.h:118):
 *   auc_num2 = sum_{i: s_i = +1} sum_{j: s_j = -1} ( 2 [p_i > p_j] + [p_i == p_j] )      float comparisons: +0 == -0
 *   auc      = auc_num2 / (2 pos neg), NaN when pos neg == 0.  auc_num2 is that INTEGER exactly (tie-aware, no sampling, no
 *              binning: one radix sort of the scores + two scans); for n_rows < 2^31, 2 pos neg < 2^63.
 *   logloss  = (1 / rows) sum_i l(s_i p_i), evaluated in fp64 from the fp32 score:
 *              FMX_LINK_LOGISTIC  l(z) = max(-z, 0) + log1p(exp(-|z|))        = -ln sigmoid(z)
 *              FMX_LINK_PROBIT    l(z) = -log(0.5 erfc(-z / sqrt(2)))         = -ln Phi(z), AS COMPUTED: +inf where erfc underflows
 *                                                                               (z below about -38)
 *              an infinite score gives 0 or +inf accordingly.
 *   NaN scores: nan_rows > 0 makes auc and logloss NaN and auc_num2 0 (nothing is sorted); rows, nan_rows, pos, neg, correct and
 *              accuracy are still right -- a diverged model shows up in the metrics instead of vanishing from their denominators.
 *   regression handles: rmse and mae (clamped, fm_learn.h:138-152); accuracy and the classification counts 0, auc = logloss = NaN,
 *              no sort.  Classification handles: rmse = mae = 0, as in fmx_eval.
 *   an empty slot: FMX_OK, rows = 0, auc = logloss = NaN, everything else 0.
 * Every fp64 sum is taken in a fixed order (per-block partials on a grid that is a fixed function of n_rows, summed in block order
 * by a final kernel; the integer counts likewise, the AUC numerator with integer atomics): two calls with unchanged parameters are
 * bit-identical in every field except the two times -- fmx_evaluate, whose partials meet in fp64 atomics, is not.
 * Device memory, allocated and freed inside the call: 24 bytes per row (8 + 8 the sort's key double buffer, 4 + 4 the two scans) +
 * the radix sort's temporary (a few MiB of histograms) on classification handles; a few KiB of block partials otherwise.
 * fmx_group_evaluate_ex: the same over the feature shards of a loopback / RCCL group of ONE process -- the finished y-hat chunks of
 * fmx_group_predict stay on the first shard's device (no prediction crosses to the host) and are reduced there against the first
 * shard's targets; a one-handle group forwards.
 * Refusals: FMX_E_ARG: NULL out, unknown link, flags != 0.  FMX_E_STATE: a slot never uploaded, a slot without targets (as
 * fmx_evaluate).  FMX_E_UNSUPPORTED: a feature shard or communicator rank passed to fmx_evaluate_ex itself (as fmx_evaluate), more
 * than 2^31 - 1 rows.  Row weights (fmx_set_row_weights) are ignored: every row counts once; fmx_evaluate_weighted is the
 * weighted log loss.
 * Added without an ABI version change: a caller detects the feature by the symbol fmx_evaluate_ex. */
#define FMX_LINK_LOGISTIC 0u   /* q = 1 / (1 + exp(-p)):  fm_learn_sgd::predict, classification (fm_learn_sgd.h:80-87) */
#define FMX_LINK_PROBIT   1u   /* q = Phi(p):              the als / mcmc learners' cdf_gaussian */
typedef struct fmx_eval_opts {
  uint32_t link;            /* FMX_LINK_* */
  uint32_t flags;           /* none defined: 0 */
} fmx_eval_opts;
typedef struct fmx_eval_ex {
  uint64_t rows, nan_rows;      /* nan_rows: rows whose score is NaN */
  uint64_t pos, neg;            /* classification: rows with target >= 0 / < 0 */
  uint64_t correct;             /* classification: rows with (p >= 0) == (target >= 0); a NaN score is never correct */
  uint64_t auc_num2;            /* the AUC numerator above, exact */
  double   auc, logloss;        /* classification */
  double   rmse, mae, accuracy; /* as fmx_eval, reduced in a fixed order */
  double   device_seconds;      /* whole call */
  double   rank_seconds;        /* sort + scans + rank-sum kernel only (0 when nothing was sorted) */
  uint32_t flags;               /* FMX_EVAL_WSIDE as in fmx_eval */
  uint32_t reserved;
} fmx_eval_ex;
/* opts may be NULL (= logistic) */
int fmx_evaluate_ex(fmx_handle h, int slot, const fmx_eval_opts *opts, fmx_eval_ex *out);

/* ---- exact per-query AUC (GAUC) of a slot, reduced on the device -------------------------------
 * The pooled AUC of fmx_evaluate_ex mixes "which query scores higher" with "which row this query prefers".  Click models are
 * judged by the AUC INSIDE each user or session, averaged with the impressions as weights (GAUC); the BPR paper's metric is the
 * per-user AUC.  A QUERY here is that user / session: one id per row ("group" already names `-meta` attribute groups and feature
 * shards).  fmx_set_row_queries attaches the ids to a slot, fmx_evaluate_by_query scores the slot once like fmx_evaluate_ex and
 * reduces per query.  With p_i, s_i and the float comparison (+0 == -0) of fmx_evaluate_ex:
 *   auc_num2_q  = sum_{i, j in q, s_i = +1, s_j = -1} ( 2 [p_i > p_j] + [p_i == p_j] )          that INTEGER exactly
 *   pos_q, neg_q  rows of q with target >= 0 / target < 0
 *   auc_q       = (double)auc_num2_q / (2.0 * (double)pos_q * (double)neg_q)      both operands exact below 2^53
 *   a query is VALID when pos_q > 0 and neg_q > 0; one-class and empty queries take no part in the three means:
 *   auc_within  = num2_within / den2_within = sum_valid auc_num2_q / sum_valid 2 pos_q neg_q
 *   gauc        = sum_valid (pos_q + neg_q) auc_q / valid_rows                    (impression-weighted)
 *   auc_macro   = sum_valid auc_q / valid_queries
 *   NaN scores: with pooled.nan_rows > 0 nothing is sorted: auc_within, gauc and auc_macro are NaN, num2_within, den2_within,
 *               the three query counts and valid_rows 0, the per-query arrays zero-filled; pooled is exactly fmx_evaluate_ex's
 *               NaN result.
 *   valid_queries == 0: the three means are NaN, num2_within, den2_within and valid_rows 0; the counts and the per-query
 *               pos_q / neg_q are still right -- also when the whole slot holds one class (pooled skips its own sort, the
 *               by-query pipeline still runs).
 *   regression handles: pooled as fmx_evaluate_ex fills it; the counts 0, the means NaN, the arrays zero-filled, nothing sorted.
 *   an empty slot: FMX_OK, pooled = the empty result, queries = empty_queries = n_queries, means NaN, arrays zero-filled.
 * Pipeline: the score pass of fmx_evaluate_ex fills `pooled`; the same scores then give one 64-bit key per row (query id <<
 * 33 | fmx_evaluate_ex's 33-bit key), ONE radix sort over 33 + ceil(log2(n_queries)) bits, three library scans and a rank-sum kernel
 * that reduces the query segments inside each wavefront and issues one 64-bit integer atomic per (wavefront, segment).  Only
 * integers meet in atomics; the fp64 sums over the queries run in a fixed order (block partials on a grid that is a fixed function
 * of n_queries): two calls with unchanged parameters are bit-identical in every field except the two times.
 * Device memory: resident, 4 bytes per row (the ids).  Inside the call, allocated and freed: fmx_evaluate_ex's scratch first, then
 * 28 bytes per row (8 + 8 the key double buffer, 4 + 4 + 4 the three scans) + the sort's temporary + 16 bytes per QUERY.
 * fmx_group_set_row_queries puts the ids on the first shard's slot, where the targets live; fmx_group_evaluate_by_query reduces
 * the finished y-hat chunks there like fmx_group_evaluate_ex; a one-handle group forwards.
 * Refusals: as fmx_evaluate_ex (FMX_E_ARG: NULL out, unknown link, flags != 0; FMX_E_STATE: a slot never uploaded or without
 * targets; FMX_E_UNSUPPORTED: a feature shard passed to the per-handle call, more than 2^31 - 1 rows), and FMX_E_STATE when the slot
 * has no query ids.  fmx_set_row_queries: FMX_E_ARG for n_queries == 0 or > 2^31 - 1 and for any qid >= n_queries (the message
 * names the first offending row; nothing changes on failure), FMX_E_STATE for a slot never uploaded; an empty slot with a
 * non-NULL qid is accepted.  Row weights (fmx_set_row_weights) are ignored: every row counts once.
 * Added without an ABI version change: a caller detects the feature by the symbol fmx_evaluate_by_query. */

/* per-row query ids of a slot: qid[n_rows] (host), every qid < n_queries, 1 <= n_queries <= 2^31 - 1.  Kept on the device
 * (4 bytes per row).  A new call replaces them; NULL drops them; fmx_upload_rows and its siblings, fmx_synth_rows* and
 * fmx_free_rows drop them (free_slot), fmx_destroy frees them. */
int fmx_set_row_queries(fmx_handle h, int slot, const uint32_t *qid, uint32_t n_queries);

typedef struct fmx_eval_query {
  fmx_eval_ex pooled;        /* field for field what fmx_evaluate_ex returns for this slot and link (times aside) */
  uint64_t queries;          /* n_queries */
  uint64_t valid_queries;    /* queries holding at least one positive AND one negative row */
  uint64_t one_class_queries;/* non-empty, one class only: they take no part in the three means below */
  uint64_t empty_queries;
  uint64_t valid_rows;       /* rows of the valid queries */
  uint64_t num2_within;      /* sum over valid q of auc_num2_q          (exact) */
  uint64_t den2_within;      /* sum over valid q of 2 pos_q neg_q       (exact) */
  double   auc_within;       /* num2_within / den2_within: the share of correctly ordered within-query (pos, neg) pairs */
  double   gauc;             /* sum_valid rows_q auc_q / valid_rows,  auc_q = auc_num2_q / (2 pos_q neg_q)   (impression-weighted) */
  double   auc_macro;        /* sum_valid auc_q / valid_queries */
  double   device_seconds;   /* whole call */
  double   rank_seconds;     /* the by-query sort, scans, rank-sum and final kernels only */
} fmx_eval_query;

/* opts as fmx_evaluate_ex (NULL = logistic).  num2_q (uint64), pos_q, neg_q (uint32): NULL or host [n_queries], per query. */
int fmx_evaluate_by_query(fmx_handle h, int slot, const fmx_eval_opts *opts, fmx_eval_query *out,
                          uint64_t *num2_q, uint32_t *pos_q, uint32_t *neg_q);

/* ---- exact per-query NDCG, recall and precision at K of a slot, reduced on the device ----------
 * Of the rows of a query, how good are the K the model puts on top?  Relevance of a row is binary, target >= 0 (fm_learn.h:118);
 * the scores are the fp32 raw y-hat of fmx_predict, compared as floats (+0 == -0); the query ids are fmx_set_row_queries'.
 * Inside query q the rows are ranked by descending score.  Rows of equal score form a TIE RUN that occupies the 0-based ranks
 * [a, b), t = b - a rows of which p are relevant.  The metric is the EXPECTATION over a uniformly random order inside every tie
 * run (McSherry & Najork, "Computing information retrieval performance measures efficiently in the presence of tied scores",
 * ECIR 2008), so it does not depend on how a sort placed equal scores.  With the discount table
 *   D[0] = 0,  D[r + 1] = D[r] + 1.0 / log2((double)r + 2.0)            (fmx_rank_discounts: sequential, fp64)
 * and a' = min(a, K), b' = min(b, K), in exactly this operation order:
 *   hits_q@K      = sum over the runs with a < K of ((double)p * (double)(b' - a')) / (double)t
 *   dcg_q@K       = sum over the runs with a < K of ((double)p * (D[b'] - D[a']))   / (double)t
 *   ndcg_q@K      = dcg_q / D[min(pos_q, K)]
 *   recall_q@K    = hits_q / pos_q
 *   precision_q@K = hits_q / K                    (/ K even when the query has fewer rows)
 * Without ties every run is one row and a term is p * (D[a + 1] - D[a]): the textbook 1 / log2(a + 2) up to the rounding of
 * that difference.  A query is RELEVANT when pos_q > 0; only relevant queries enter the means: ndcg, recall and precision are
 * the plain means over the relevant queries, hits is the sum of hits_q over them, tied_queries counts the relevant queries in
 * which some run with a < K has 0 < p < t (where breaking the ties would have changed the classic metric).
 *   NaN scores (pooled.nan_rows > 0) and regression handles: nothing is sorted, every mean is NaN, every count 0, the arrays
 *               zero-filled, topk_seconds 0; by_query is exactly fmx_evaluate_by_query's result for that state.
 *   relevant_queries == 0: the means are NaN, hits and tied_queries 0.
 *   an empty slot: FMX_OK, by_query = the empty result, the means NaN, the arrays zero-filled.
 *   a slot of one class still runs the by-query pipeline.
 * Pipeline: ONE scoring pass and ONE sort -- the call does what fmx_evaluate_by_query does (by_query is field for field its
 * result) and then reduces the top min(rows_q, k_max) sorted positions of every query segment over the same sorted keys and
 * scans: one wavefront per query, the lane at the tail of a tie run adds the run's terms, fp64 sums lane -> wavefront (xor
 * butterfly) -> block partials -> one final wavefront, on a grid that is a fixed function of n_queries.  No float atomics: two
 * calls with unchanged parameters are bit-identical in every field except the times.
 * Device memory beyond fmx_evaluate_by_query's, allocated and freed inside the call: at most 4 + 16 * n_cutoffs bytes per
 * query (4: the end of the query's segment; 16 per cutoff only when dcg_q / hits_q are asked for), 8 * (k_max + 1) bytes of
 * discount table (k_max = the largest cutoff; at most 512 KiB) and (blocks + 1) x 21 x 8 bytes of block partials with the result
 * row behind them (blocks = ceil(n_queries / 4), at most 2048: 344 KiB at most).
 * Refusals: everything fmx_evaluate_by_query refuses, with the same codes; FMX_E_ARG for NULL opts or out, n_cutoffs outside
 * 1 .. FMX_RANK_MAX_CUTOFFS, a k of 0 or above FMX_RANK_MAX_K, cutoffs that are not strictly ascending; FMX_E_UNSUPPORTED for a
 * feature shard passed to the per-handle call.  fmx_rank_discounts: FMX_E_ARG for NULL out or k_max above FMX_RANK_MAX_K.
 * Row weights (fmx_set_row_weights) are ignored; relevance is not graded.
 * Added without an ABI version change: a caller detects the feature by the symbol fmx_evaluate_rank. */
#define FMX_RANK_MAX_CUTOFFS 4
#define FMX_RANK_MAX_K 65536u
typedef struct fmx_rank_opts {
  uint32_t link, flags;                       /* as fmx_eval_opts; flags 0 */
  uint32_t n_cutoffs;                         /* 1 .. FMX_RANK_MAX_CUTOFFS */
  uint32_t k[FMX_RANK_MAX_CUTOFFS];           /* strictly ascending, 1 .. FMX_RANK_MAX_K */
  uint32_t reserved;
} fmx_rank_opts;

typedef struct fmx_rank_at {
  uint32_t k, reserved;
  uint64_t tied_queries;                      /* relevant queries with a mixed tie run that begins above the cutoff */
  double hits, ndcg, recall, precision;       /* hits: a sum; the others: means over the relevant queries */
} fmx_rank_at;

typedef struct fmx_eval_rank {
  fmx_eval_query by_query;                    /* field for field what fmx_evaluate_by_query returns, times aside */
  uint64_t relevant_queries;                  /* pos_q > 0 */
  uint32_t n_cutoffs, reserved;
  fmx_rank_at at[FMX_RANK_MAX_CUTOFFS];
  double device_seconds, topk_seconds;        /* whole call / the added kernels only */
} fmx_eval_rank;

/* D[0 .. k_max] as above into out[k_max + 1].  Host arithmetic: no device, no handle.  The device call uploads this table. */
int fmx_rank_discounts(uint32_t k_max, double *out);

/* dcg_q, hits_q: NULL or host double[n_queries * n_cutoffs], query-major */
int fmx_evaluate_rank(fmx_handle h, int slot, const fmx_rank_opts *opts, fmx_eval_rank *out,
                      double *dcg_q, double *hits_q);

/* ---- the averaged predictions of `-method mcmc`, kept on the device ----------------------------
 * The prediction of fm_learn_mcmc_simultaneous is not that of one model but the running mean over the draws (pred_sum_all / (i + 1),
 * fm_learn_mcmc_simultaneous.h:129-161, 213-264).  A posterior accumulator keeps the three vectors of that file for one slot on the
 * device -- the last draw (pred_this), the sum over all draws (pred_sum_all) and the sum over the draws from burn_in on
 * (pred_sum_all_but5) -- so that no prediction crosses to the host between the sweeps.
 * fmx_post_begin creates the accumulator of a slot with both sums +0 (again = reset; opts NULL = {5, 0, 0}).
 * fmx_post_accumulate scores the slot like fmx_evaluate_ex (one pass at the predict roofline, kept `-relation` blocks and the weight
 * side stream included) and adds the draw.  With d the number of draws accumulated before the call and p_i the fp32 raw y-hat
 * fmx_predict would return for row i now:
 *   regression      this_i = (double)p_i;   v_i = max(min_target, min(max_target, (double)p_i)) with the config's doubles (:132-133);
 *                   a NaN p_i stays NaN (numpy's minimum / maximum, not std::min)
 *   classification  v_i = this_i = 0.5 + 0.5 ref_erf(0.707106781 (double)p_i): the reference's cdf_gaussian with its five-term erf
 *                   polynomial (random.h:45-67), not erfc
 *   sum_all_i += v_i;   sum_late_i += v_i when d >= burn_in.   fp64, one add per row per draw: the order is the draw order.
 * Means: mean = sum * (1.0 / count) -- a product with the reciprocal, as :278 and :296 have it, not a division -- with
 *   count = draws (FMX_POST_ALL) or late_draws (FMX_POST_LATE); FMX_POST_THIS is this_i itself.
 *   FMX_POST_LATE with late_draws == 0: rows = 0 and every metric NaN (the reference's 1.0 / (i - 5 + 1) in unsigned arithmetic is
 *   not reproduced).
 * Metrics of the three vectors over the rows [0, eval_rows) (fmx_post_stats::m, the reference's _evaluate / _evaluate_class):
 *   regression      rmse = sqrt(mean (c_i - target_i)^2), mae = mean |c_i - target_i| with c_i the mean clamped again (:279-283)
 *   classification  correct counts (m_i >= 0.5 && target_i > 0) || (m_i < 0.5 && target_i < 0) (:297), accuracy = correct / rows;
 *                   ll_ref = -(1 / rows) sum_i [ t log10(q) + (1 - t) log10(1 - q) ], t = (target_i + 1) / 2, q = m_i clamped to
 *                   [0.01, 0.99] (:300-304: the reference's Test(ll))
 *   a NaN mean counts in nan_rows, is never correct and makes rmse / mae / ll_ref NaN; the counts stay right.  The metrics of the
 *   other task are 0, as in fmx_eval_ex; with rows = 0 (an empty slot, FMX_POST_LATE before its first draw) every double is NaN.
 * fmx_post_evaluate_ex fills fmx_eval_ex for one of the three vectors over the rows [0, eval_rows): rows, nan_rows, pos / neg
 *   (target >= 0 / < 0), correct / accuracy by the rule above, rmse / mae on regression handles only, and on classification handles
 *   logloss = (1 / rows) sum_i ( target_i >= 0 ? -ln m_i : -ln(1 - m_i) )   natural log, unclamped: +inf where the mean is 0 or 1 on
 *             the wrong side; only the term of the row's own class is taken, so 0 * ln 0 never arises
 *   auc_num2 = the integer of fmx_evaluate_ex with fp64 comparisons of the means (64-bit sort keys: the means are sums of values in
 *             [0, 1] started from +0, so their bit pattern orders them; a mean below +0 is refused with FMX_E_STATE, never clamped)
 *   auc = logloss = NaN on regression handles and with NaN means; before the first draw of the vector: rows = 0 and the empty
 *   result of fmx_evaluate_ex.  rank_seconds / device_seconds as there; flags 0.
 * fmx_post_get copies out[n_rows]: the SUM (FMX_POST_ALL, FMX_POST_LATE; *draws = its count) or this_i (FMX_POST_THIS; *draws = 1
 *   after the first draw, else 0).  out or draws may be NULL.
 * Every fp64 sum of the metrics runs in the fixed order of fmx_evaluate_ex on the same grid: two identical call sequences give
 * bit-identical structs apart from the times.
 * State: at most one accumulator per slot; fmx_upload_rows and its siblings and fmx_free_rows drop it (as interactions are
 * dropped), fmx_destroy frees it.  Resident: 20 bytes per row (8 + 8 the sums, 4 the fp32 last draw; this_i is recomputed from it).
 * fmx_post_evaluate_ex takes fmx_evaluate_ex's 24 bytes per row inside the call.  The calls work while an ALS / MCMC session is open
 * on another slot: train on slot 0, accumulate slot 1.
 * fmx_group_post_*: the same over the feature shards of a loopback / RCCL group of ONE process; the state lives on the first
 * shard's device, where fmx_group_predict's finished y-hat chunks are accumulated.  A one-handle group forwards.
 * Refusals: FMX_E_ARG: which > 2, flags != 0, eval_rows > n_rows, NULL out of _evaluate_ex.  FMX_E_STATE: a slot never uploaded or
 * without targets; _accumulate / _evaluate_ex / _get / _end without _begin.  FMX_E_UNSUPPORTED: a feature shard or communicator rank
 * passed to the per-handle calls, more than 2^31 - 1 rows.  An empty slot: FMX_OK with zero rows.  Row weights
 * (fmx_set_row_weights) are ignored.
 * Added without an ABI version change: a caller detects the feature by the symbol fmx_post_begin. */
#define FMX_POST_THIS 0u   /* the last accumulated draw             (pred_this) */
#define FMX_POST_ALL  1u   /* mean over all accumulated draws       (pred_sum_all * 1 / draws) */
#define FMX_POST_LATE 2u   /* mean over the draws d >= burn_in      (pred_sum_all_but5, burn_in = 5) */
typedef struct fmx_post_opts {
  uint32_t burn_in;         /* reference: 5 */
  uint32_t eval_rows;       /* the metrics cover the rows [0, eval_rows); 0 = all (num_eval_cases) */
  uint32_t flags;           /* none defined: 0 */
  uint32_t reserved;
} fmx_post_opts;
typedef struct fmx_post_metric {
  uint64_t rows, nan_rows, correct;
  double   rmse, mae;           /* regression (:272-289) */
  double   accuracy, ll_ref;    /* classification (:291-309) */
} fmx_post_metric;
typedef struct fmx_post_stats {
  uint64_t draws, late_draws;   /* after this call */
  fmx_post_metric m[3];         /* indexed by FMX_POST_* */
  double   device_seconds;
} fmx_post_stats;
int fmx_post_begin(fmx_handle h, int slot, const fmx_post_opts *opts);
/* out may be NULL */
int fmx_post_accumulate(fmx_handle h, int slot, fmx_post_stats *out);
int fmx_post_evaluate_ex(fmx_handle h, int slot, uint32_t which, fmx_eval_ex *out);
int fmx_post_get(fmx_handle h, int slot, uint32_t which, double *out, uint64_t *draws);
int fmx_post_end(fmx_handle h, int slot);

/* ---- fm_learn_sgd_element::learn, one epoch (fm_learn_sgd_element.h:56-67) -------------------- */
int fmx_sgd_epoch(fmx_handle h, int slot, const fmx_sgd_opts *opts, fmx_epoch_stats *stats);
/* On a handle that is one rank of a communicator (fmx_comm_init_rank, one process per GPU) this call is COLLECTIVE, every time: the
 * shards' shares of the collision mass are summed over RCCL (one 8-byte all-reduce), so every rank must make it -- and fmx_sgd_epoch,
 * which resolves its batch through it, is collective in the same sense.  (Until ABI 5 the sum was cached per rank, which made the
 * decision to enter the collective per rank too: a rank that re-uploaded its slot entered alone.) */
int fmx_sgd_batch_info(fmx_handle h, int slot, const fmx_sgd_opts *opts, fmx_batch_info *out);
/* the same decision as host arithmetic (no device needed): the batch fmx_sgd_epoch runs with for rows of the given collision mass --
 * requested != 0: that batch, with its gain and status; requested == 0: 262144 cut to the largest power of two (never below 32) with
 * learn_rate * curvature * batch * collision_mass <= 1 (curvature 1 for regression, 1/4 for classification) */
int fmx_batch_rule(int32_t task, double learn_rate, double collision_mass, uint32_t requested, fmx_batch_info *out);

/* ---- pairwise ranking (BPR) around fm_pairSGD (fm_sgd.h:53-126) ---------------------------------------------------
 * The reference defines the pairwise update but no learner calls it; the loop around it is this library's.
 * One epoch visits the slot's pairs t = 0 .. P-1 in stored order.  (a, b) = pairs[t] means "row a is preferred to row b":
 *
 *   y_a  = fm.predict(x_a, sum_pos, sum_sqr)            // fm_model.h:105-127, w0 included
 *   y_b  = fm.predict(x_b, sum_neg, sum_sqr)
 *   mult = -(1 - sigmoid(y_a - y_b))                    // BPR: descent on -ln sigmoid(y_a - y_b); sigmoid = util.h:52
 *   fm_pairSGD(&fm, learn_rate, x_a, x_b, mult, sum_pos, sum_neg, grad_visited, grad)
 *
 * Properties of fm_pairSGD kept here (not those of fm_SGD): with k0 every pair does w0 -= reg0 * w0, without learning rate, and
 * nothing else moves w0; a feature's linear gradient is the sum of its values in x_a minus the sum in x_b, its factor gradient
 * sum_pos(f) x - v x x over its entries in x_a minus the same with sum_neg(f) over x_b (ids repeated inside a row and ids in both
 * rows included); each distinct feature of the pair is updated once with ONE regularisation term (grad_visited); every sum and
 * gradient comes from the parameters at the start of the pair; the targets of the rows are not used.
 *
 * Batch rule (FMX_SGD_MINIBATCH): the pairs are cut into batches of B consecutive pairs.  Every pair of a batch takes its sums and
 * multiplier from the parameters at the start of the batch; each feature j touched by the batch is then updated once:
 *   w_j  -= lr * sum_{t in batch, j in t} ( mult_t * gw_tj  + regw * w_j(start) )
 *   v_jf -= lr * sum_{t in batch, j in t} ( mult_t * gv_tjf + regv * v_jf(start) )
 * (gw, gv the per-pair gradients above, one regularisation term per pair); w0 takes w0 -= reg0 * w0 once per pair.  At B = 1 this
 * rule is exactly the loop.  Sums run in a fixed order (pair order inside a (batch, feature) segment, no float atomics): two runs
 * are bit-identical.
 *
 * fmx_upload_pairs : the pairs of a row slot, row_a[t] preferred to row_b[t], 0-based rows of the slot.  Every index must be
 *                    < n_rows (FMX_E_ARG otherwise, nothing changes).  A new call replaces the pairs (resampled negatives);
 *                    fmx_free_rows and a new upload into the slot drop them.
 * fmx_pair_epoch   : one epoch.  mode FMX_SGD_SEQUENTIAL (one workgroup walks the pairs in order: the parity instrument) or
 *                    FMX_SGD_MINIBATCH (batch = 0: FMX_PAIR_DEFAULT_BATCH pairs).  fmx_epoch_stats: rows = pairs, batches,
 *                    batch_used, device_seconds, max_feature_count (MINIBATCH: entries of the longest (batch, feature) segment),
 *                    setup_seconds (the one-time bucketing of the pair-expanded entries, cached per (slot, pairs, batch)).
 *                    FMX_E_UNSUPPORTED: FMX_SGD_HOGWILD, a feature shard or communicator rank, a slot with kept `-relation`
 *                    blocks, more than 2^31 - 1 pair-expanded entries (MINIBATCH).  FMX_E_STATE: no pairs uploaded, an open
 *                    ALS / MCMC session on the slot, an open SGDA session.
 * fmx_pair_evaluate: accuracy = fraction of pairs with y_a > y_b, loss = mean of -ln sigmoid(y_a - y_b); computed on the device
 *                    with fp64 reductions in a fixed order. */
#define FMX_PAIR_DEFAULT_BATCH 1024u
typedef struct fmx_pair_opts {
  int32_t  mode;            /* FMX_SGD_SEQUENTIAL or FMX_SGD_MINIBATCH */
  uint32_t batch;           /* MINIBATCH: pairs per batch; 0 = FMX_PAIR_DEFAULT_BATCH */
  uint32_t flags;           /* none defined yet: 0 */
  uint32_t reserved;
} fmx_pair_opts;
typedef struct fmx_pair_eval {
  double   accuracy;        /* fraction of pairs with y_a > y_b */
  double   loss;            /* mean of -ln sigmoid(y_a - y_b) */
  double   device_seconds;
  uint64_t pairs;
} fmx_pair_eval;
int fmx_upload_pairs(fmx_handle h, int slot, const uint32_t *row_a, const uint32_t *row_b, uint64_t n_pairs);
int fmx_pair_epoch(fmx_handle h, int slot, const fmx_pair_opts *opts, fmx_epoch_stats *stats);
int fmx_pair_evaluate(fmx_handle h, int slot, fmx_pair_eval *out);

/* ---- top-K retrieval of candidate rows per query row ----------------------------------------
 * For query row q of query_slot and candidate row c of cand_slot, score(q, c) is the raw y-hat of the JOINED row x_q ++ x_c
 * (fm_model.h:105-127: w0 once, no clamp, no sigmoid; ids repeated inside a row or across the two rows count separately), computed
 * without the join:
 *   score(q, c) = a_q + b_c + sum_f S_q[f] S_c[f]          S_r[f] = sum_{i in r} v[id_i][f] x_i
 *   a_q = k0 w0 + k1 lin_q + 1/2 sum_f (S_q[f]^2 - SS_q[f]),  b_c = k1 lin_c + 1/2 sum_f (S_c[f]^2 - SS_c[f])
 * evaluated in fp32 on the device (the dot product on the f32 matrix units) and returned widened to double.
 * Result per query: the topk candidates with the highest score in descending order; equal scores by the lower candidate index
 * first; NaN scores are never returned; fewer than topk eligible candidates: padded with index UINT32_MAX and score -INFINITY.
 *   query rows   : [query_row0, query_row0 + n_query) of query_slot; a query's list does not depend on the other queries of the call,
 *                  nor on how the library splits the candidates (FMX_TOPK_SPLITS at fmx_create forces the split count); two calls
 *                  with the same inputs are bit-identical.  query_slot may equal cand_slot.
 *   exclusion    : exclude_ptr (NULL or host [n_query + 1] offsets, query i of THIS call) into exclude_idx: candidate rows that
 *                  query i must not return; repeats and any order allowed.  An index >= the candidate rows fails the call with
 *                  FMX_E_ARG and writes nothing.
 * Preconditions as fmx_predict.  FMX_E_UNSUPPORTED: a feature shard or communicator rank, a slot with kept `-relation` blocks.
 * FMX_E_ARG: topk = 0 or > FMX_TOPK_MAX, a query range outside the slot, NULL outputs or opts, flags != 0.  FMX_E_STATE: a slot that
 * was never uploaded.  Device scratch stays bounded (queries are taken in chunks) besides the factor sums of the two row sets.
 * Added without an ABI version change: a caller detects the feature by the symbol fmx_topk. */
#define FMX_TOPK_MAX 1024u
typedef struct fmx_topk_opts {
  uint32_t topk;                 /* K: results per query, 1 .. FMX_TOPK_MAX */
  uint32_t flags;                /* none defined yet: 0 */
  uint64_t query_row0;           /* first query row of the query slot */
  uint32_t n_query;              /* query rows scored by this call */
  uint32_t reserved;
  const uint64_t *exclude_ptr;   /* NULL, or host [n_query + 1] offsets into exclude_idx (query i of THIS call) */
  const uint32_t *exclude_idx;   /* candidate rows excluded for that query */
} fmx_topk_opts;
typedef struct fmx_topk_stats {
  double   device_seconds;       /* whole call on the device */
  double   score_seconds;        /* the score-and-select kernels only */
  uint64_t scores;               /* n_query * n_cand */
  uint32_t splits;               /* candidate splits the library chose */
  uint32_t reserved;
} fmx_topk_stats;
/* idx_out: uint32 [n_query][topk]; score_out: double [n_query][topk] (the device's fp32 score, widened); stats may be NULL */
int fmx_topk(fmx_handle h, int query_slot, int cand_slot, const fmx_topk_opts *opts,
             uint32_t *idx_out, double *score_out, fmx_topk_stats *stats);

/* ---- BPR on query x candidate interactions, negatives drawn on the device ---------------------
 * The training counterpart of fmx_topk: query rows (users) in one slot, candidate rows (items) in another, T observed interactions
 * (q[t], c[t]) and n_neg >= 1 negatives per interaction.  The pairs of one epoch are p = t * n_neg + s (t = 0 .. T-1,
 * s = 0 .. n_neg-1, in that order):
 *   row a_p = x_{q[t]} ++ x_{c[t]}        (query entries first, then candidate entries: fmx_topk's join)
 *   row b_p = x_{q[t]} ++ x_{neg[p]}
 * and one epoch is exactly fmx_pair_epoch on those joined rows with the pairs (a_p, b_p), in the same two modes, without the joined
 * rows being written: w0 only decays; each distinct feature of the pair (the query's included: linear gradient x - x = 0, the regw
 * term stays) is updated once with one regularisation term; repeated ids count separately; all sums come from the start of the
 * pair (SEQUENTIAL) or of the batch (MINIBATCH); no float atomics, two runs are bit-identical.
 *
 * The sampler is a pure function (libfm_amd.ranking.sample_negatives restates it on the CPU).  With mix64 = the splitmix64
 * finaliser (x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31), all arithmetic mod 2^64
 * and C = the candidate rows:
 *   draw(seed, epoch, p, a) = ( mix64( seed ^ (epoch * 0x9E3779B97F4A7C15)
 *                                      ^ (p * 0xD6E8FEB86659FD93 + a * 0xA24BAED4963EE407 + 0x9FB21C651E98DF25) ) * C ) >> 64
 *   neg[p] = draw(seed, epoch, p, a*),  a* = the first attempt a in 0 .. FMX_NEG_ATTEMPTS-1 whose draw is neither c[t] nor in the
 *   exclusion list of q[t]; when all attempts are rejected the last draw is used as it is and the pair is counted as `forced`.
 *
 * Hardest of M: flags = FMX_NEG_HARDEST | FMX_NEG_DRAWS(M), M = 1 .. FMX_NEG_ATTEMPTS.  An attempt is
 * ACCEPTED when its draw is neither c[t] nor in the exclusion list of q[t].  The attempts a = 0 .. FMX_NEG_ATTEMPTS-1 are walked in
 * order and the walk stops after the M-th accepted one; neg[p] is the accepted draw d with the highest
 *   r(q, d) = b_d + sum_f S_q[f] S_d[f]
 * (fmx_topk's decomposition score(q, c) = a_q + b_c + <S_q, S_c> without a_q, which all draws of a pair share; S and b in fp32 from
 * the same kernels as fmx_topk, k0 = 0).  A later draw replaces the current best only when its r is strictly greater -- equal
 * scores keep the earlier attempt -- or when the best's r is NaN and its own is not.  Fewer than M accepted: the pick is among
 * those; none accepted: the last draw as it is and the pair is `forced`, as above.  The same candidate drawn twice is harmless.
 * M = 1 is the uniform sampler, integer for integer.  S and b are taken from the parameters AS THEY ARE WHEN THE CALL STARTS: the
 * negatives of an epoch are fixed before its first pair in both modes, so fmx_pair_sample with the same options and unchanged
 * parameters returns exactly what fmx_pair_epoch_sampled trains on (and fmx_pair_evaluate_sampled evaluates).
 * FMX_NEG_DRAWS without FMX_NEG_HARDEST, M = 0, M > FMX_NEG_ATTEMPTS and every other bit (bit 0 included) are FMX_E_ARG.
 * libfm_amd.ranking.sample_negatives(..., draws=M, query_sums, cand_sums, cand_scal) restates the rule in float64.
 *
 * fmx_upload_interactions : the interactions live on query_slot and name cand_slot (the two may be equal).  exclude_ptr: NULL, or
 *                    host [Q + 1] offsets into exclude_idx over ALL Q rows of the query slot: candidate rows that must not be
 *                    drawn for that query, in any order, repeats allowed (sorted on upload).  An index outside its slot fails with
 *                    FMX_E_ARG and changes nothing.  A new call replaces the interactions; fmx_upload_rows / fmx_free_rows (and
 *                    the other uploads) on EITHER slot drop them.
 * fmx_pair_sample  : the sampler alone: neg_out[n * n_neg] and the forced count of (seed, epoch).
 * fmx_pair_epoch_sampled : one epoch with the negatives of (seed, epoch).  fmx_epoch_stats: rows = n * n_neg, batches, batch_used
 *                    and device_seconds as fmx_pair_epoch; setup_seconds = everything that is not the sums / apply launches
 *                    (sampling, key expansion, sort).  *forced_out = the forced count.
 * fmx_pair_evaluate_sampled : accuracy and loss over the pairs of (seed, epoch), fixed-order reduction as fmx_pair_evaluate.
 * FMX_E_UNSUPPORTED: FMX_SGD_HOGWILD, a feature shard or communicator rank, kept `-relation` blocks on either slot, more than
 * 2^31 - 1 expanded entries (MINIBATCH) or 2^31 - 2 pairs.  FMX_E_STATE: no interactions, an open ALS / MCMC session on either
 * slot, an open SGDA session.  FMX_E_ARG: n_neg = 0, flags other than the two below, NULL opts, an empty candidate slot with n > 0.
 * Device memory: 20 bytes per pair + 40 bytes per expanded entry (an entry of x_q, x_c+ or x_c-; the query's once) + the radix
 * sort's temporary, and with FMX_NEG_HARDEST and M > 1 the two row tables, (Q + C)(KM + 1) * 4 bytes (KM = the factors padded to
 * a power of two, at least 16; C alone when the query slot is the candidate slot) + at most 64 MiB of raw sums; all kept between
 * epochs; never anything of size Q x C.
 * Added without an ABI version change: a caller detects the feature by the symbol fmx_pair_epoch_sampled, hardest-of-M by the
 * macro FMX_NEG_HARDEST (the struct keeps its layout). */
#define FMX_NEG_ATTEMPTS 16u
#define FMX_NEG_HARDEST   2u                          /* pick the best-scoring of several accepted draws */
#define FMX_NEG_DRAWS(M)  ((uint32_t)(M) << 8)        /* M = 1 .. FMX_NEG_ATTEMPTS, bits 8..15 */
typedef struct fmx_pairneg_opts {
  int32_t  mode;            /* FMX_SGD_SEQUENTIAL or FMX_SGD_MINIBATCH */
  uint32_t batch;           /* MINIBATCH: pairs per batch; 0 = FMX_PAIR_DEFAULT_BATCH */
  uint32_t n_neg;           /* negatives per interaction, >= 1 */
  uint32_t flags;           /* 0, or FMX_NEG_HARDEST | FMX_NEG_DRAWS(M) */
  uint64_t seed;
  uint64_t epoch;           /* caller-supplied counter: the same (seed, epoch) gives the same negatives */
} fmx_pairneg_opts;
int fmx_upload_interactions(fmx_handle h, int query_slot, int cand_slot, const uint32_t *q_row, const uint32_t *c_row, uint64_t n,
                            const uint64_t *exclude_ptr, const uint32_t *exclude_idx);
/* the interactions of query_slot: their candidate slot and their number n (either output may be NULL); FMX_E_STATE without any */
int fmx_interactions_info(fmx_handle h, int query_slot, int *cand_slot, uint64_t *n);
int fmx_pair_sample(fmx_handle h, int query_slot, const fmx_pairneg_opts *o, uint32_t *neg_out, uint64_t *forced_out);
int fmx_pair_epoch_sampled(fmx_handle h, int query_slot, const fmx_pairneg_opts *o, fmx_epoch_stats *stats, uint64_t *forced_out);
int fmx_pair_evaluate_sampled(fmx_handle h, int query_slot, const fmx_pairneg_opts *o, fmx_pair_eval *out);

/* ---- minibatch step split at the exchange point, for one-process-per-GPU drivers --------------
 * partial: floats per batch = fmx_partial_floats(h, batch): [batch][KP] partial factor sums followed by
 *          [batch] scalars (linear term - 0.5*sum of squares).  d_partial is DEVICE memory, 16-byte aligned.
 * The driver all-reduces (sum) d_partial across the feature shards (RCCL), then calls finish on every
 * rank: multipliers + w0 micro-chunks (identical on all ranks) and the scatter-add into the local shard.
 * `stream` is a hipStream_t (NULL = the handle's own stream). */
int fmx_partial_floats(fmx_handle h, uint32_t batch, uint64_t *n_floats);
int fmx_sgd_partial(fmx_handle h, int slot, uint64_t row0, uint32_t n_rows, float *d_partial, void *stream);
int fmx_sgd_finish(fmx_handle h, int slot, uint64_t row0, uint32_t n_rows, const float *d_partial,
                   const fmx_sgd_opts *opts, void *stream);
/* sharded predict: finish a partial buffer into y-hat (device float[n_rows]) */
int fmx_predict_finish(fmx_handle h, uint32_t n_rows, const float *d_partial, float *d_yhat, void *stream);

/* ---- several GPUs --------------------------------------------------------------------------------------------------
 * libFM is ONE process that constructs the learner and calls learn() (libfm.cpp:271-293, :415).  To use P GPUs from that
 * process, create P handles -- shard i of P (fmx_config::shard_rank / shard_world, normally shard_hash = 1) on device i --
 * give every one of them the full parameter block and the full rows (each keeps its own features), and tie them together:
 *   fmx_group_create     P handles on P DISTINCT devices: one RCCL communicator per handle (ncclCommInitRank inside one
 *                        ncclGroupStart/End); P handles on ONE device: "loopback" -- the exchange is a local reduction kernel
 *                        (tests and single-GPU boxes); a single unsharded handle: pass-through.
 *   fmx_group_sgd_epoch  one epoch of the minibatch rule: per batch the partial sums of every shard (fmx_sgd_partial), ONE
 *                        all-reduce of [batch][KP + 1] floats over xGMI, then multipliers / bias recurrence (redundantly,
 *                        identically on every shard) and the update of the shard's own rows (fmx_sgd_finish).  The rule is
 *                        the one a single handle runs with FMX_APPLY_SEGMENTED / FMX_APPLY_FUSED and the same bias_lag.
 *   fmx_group_predict / fmx_group_evaluate   fm_learn::predict / evaluate over the shards.
 * One process PER GPU instead (torchrun-style launchers): rank 0 calls fmx_comm_unique_id and hands the 128 bytes to the
 * other ranks by whatever means the launcher has; every rank creates its shard handle, calls fmx_comm_init_rank and then
 * plain fmx_sgd_epoch, which runs the same schedule with its one local shard.
 * RCCL (librccl.so.1) is loaded on first use; without it only loopback groups and single handles work. */
/* the ownership rule (fmx_config::shard_hash) as host arithmetic -- no device needed: owner[i] / local_row[i] of feature
 * ids[i] (either output may be NULL), and the inverse: the global id of a shard's local row. */
int fmx_shard_place(uint64_t num_attribute, int shard_world, int shard_hash, const uint32_t *ids, uint64_t count,
                    int32_t *owner, uint32_t *local_row);
int fmx_shard_global(uint64_t num_attribute, int shard_world, int shard_hash, int shard_rank, const uint32_t *local_rows,
                     uint64_t count, uint32_t *ids);
#define FMX_COMM_ID_BYTES 128
typedef struct fmx_group_s *fmx_group;
int fmx_comm_unique_id(void *id128);
int fmx_comm_init_rank(fmx_handle h, const void *id128, int rank, int world);
int fmx_comm_destroy(fmx_handle h);
int fmx_group_create(fmx_handle *handles, int n, fmx_group *out);
int fmx_group_destroy(fmx_group g);
const char *fmx_group_last_error(fmx_group g);
/* fmx_set_params / fmx_upload_rows for ALL shards of a group with the host data crossing PCIe ONCE: the fp64 block (51 GB at the
 * north-star size) and the rows are staged on the first shard's device, reach the other devices over xGMI (hipMemcpyPeer), and
 * every shard converts / filters its own features on its device (k_stage_in, k_shard_rows).  Same result as calling the
 * per-handle functions on every shard with the full arrays.  Not for slots with `-relation` blocks. */
int fmx_group_set_params(fmx_group g, double w0, const double *w, const double *v);
int fmx_group_upload_rows(fmx_group g, int slot, const void *entries, const uint64_t *row_ptr, const float *target,
                          uint32_t n_rows, uint64_t nnz);
/* fmx_upload_block_rows_ex for ALL shards of a group (a one-handle group forwards to it).  FMX_BLOCKS_EXPAND: every shard joins
 * the rows on the host and keeps its own features.  FMX_BLOCKS_KEEP: the main rows take the fmx_group_upload_rows path; every
 * shard keeps each block's rows restricted to the block attributes it owns (owner = the shard rule on the global id
 * attr_offset + j), and the mapping whole -- nothing of the size of the joined table is built on any shard.  fmx_group_predict /
 * fmx_group_evaluate and fmx_group_als_* then work block-wise; fmx_group_sgd_epoch refuses such a slot (FMX_E_UNSUPPORTED). */
int fmx_group_upload_block_rows_ex(fmx_group g, int slot, const void *entries, const uint64_t *row_ptr, const float *target,
                                   uint32_t n_rows, uint64_t nnz, const fmx_relation *relations, uint32_t n_relations, uint32_t flags);
int fmx_group_sgd_epoch(fmx_group g, int slot, const fmx_sgd_opts *opts, fmx_epoch_stats *stats);
int fmx_group_predict(fmx_group g, int slot, double *out);
int fmx_group_evaluate(fmx_group g, int slot, fmx_eval *out);
/* fmx_evaluate_ex over the shards of a group (see there) */
int fmx_group_evaluate_ex(fmx_group g, int slot, const fmx_eval_opts *opts, fmx_eval_ex *out);
/* fmx_set_row_queries / fmx_evaluate_by_query over the shards of a group (see there): the ids live on the first shard's slot */
int fmx_group_set_row_queries(fmx_group g, int slot, const uint32_t *qid, uint32_t n_queries);
int fmx_group_evaluate_by_query(fmx_group g, int slot, const fmx_eval_opts *opts, fmx_eval_query *out,
                                uint64_t *num2_q, uint32_t *pos_q, uint32_t *neg_q);
/* fmx_evaluate_rank over the shards of a group (see there): the finished y-hat chunks are reduced on the first shard's device */
int fmx_group_evaluate_rank(fmx_group g, int slot, const fmx_rank_opts *opts, fmx_eval_rank *out, double *dcg_q, double *hits_q);
/* fmx_post_* over the shards of a group (see there) */
int fmx_group_post_begin(fmx_group g, int slot, const fmx_post_opts *opts);
int fmx_group_post_accumulate(fmx_group g, int slot, fmx_post_stats *out);
int fmx_group_post_evaluate_ex(fmx_group g, int slot, uint32_t which, fmx_eval_ex *out);
int fmx_group_post_get(fmx_group g, int slot, uint32_t which, double *out, uint64_t *draws);
int fmx_group_post_end(fmx_group g, int slot);

/* ---- fm_learn_mcmc (ALS = MCMC without sampling, libfm.cpp:135-139) ---------------------------------
 * The learner keeps e(c) = y-hat(c) - target(c) and q_f(c) per training row (e_q_term, fm_learn_mcmc.h:46-49)
 * and sweeps the coordinates through X^T (built on the device from the slot's rows, Data.h:292-341).
 *   fmx_als_begin : fm_learn_mcmc::learn set-up (:1160-1172) + _learn's first prediction and e -= target
 *                   (fm_learn_mcmc_simultaneous.h:69-86).
 *   fmx_als_sweep : one iteration of _learn (:88-196): draw_all (fm_learn_mcmc.h:430-641: draw_w0, draw_w per
 *                   feature, per factor add_main_q + draw_v), full re-prediction of the train rows, train metric,
 *                   new residuals.  Test predictions of the iteration = fmx_predict on the test slot.
 *   fmx_als_end   : frees the caches (:1192-1200).
 * do_sample = 0 is ALS (alpha = 1, mu = 0, lambdas from -regular: reg0 -> w0, w_lambda, v_lambda; libfm.cpp:326-365).
 * do_sample = 1 draws every coordinate from its posterior N(mean, sigma^2) with a counter-based generator (NOT the
 * reference's libc rand() stream: statistical, not bitwise, parity with the reference; the chain itself is deterministic,
 * keyed by (seed, sweep, coordinate family, global feature id), and restated by the test oracle); alpha and the prior means/precisions are
 * supplied per sweep by the caller (the hyper-prior draws of :911-1097 are scalar work that stays on the host).
 * No relations (block structure) -- out of scope. */
typedef struct fmx_als_opts {
  double   alpha;           /* fm_learn_mcmc::alpha (1 for ALS) */
  double   w_mu, w_lambda;  /* prior of the linear weights */
  double   v_mu, v_lambda;  /* prior of the factors */
  int32_t  do_sample;       /* 0 = ALS, 1 = Gibbs draws */
  int32_t  reserved;
  uint64_t seed;
  const double *v_mu_f;     /* optional per-factor prior means v_mu(g=0,f) [num_factor]  (fm_learn_mcmc.h:76); NULL = v_mu */
  const double *v_lambda_f; /* optional per-factor prior precisions v_lambda(g=0,f);              NULL = v_lambda */
  /* with attribute groups (fmx_set_groups, G = num_groups > 1) the priors are per group; any table may be NULL
   * (falls back to the fields above).  Layouts are the reference's: w_*(g) DVector[G], v_*(g,f) DMatrix[G][num_factor]
   * (fm_learn_mcmc.h:1116-1122). num_groups must be 0 (no tables) or equal the handle's group count. */
  uint32_t      num_groups;
  uint32_t      reserved2;
  const double *w_mu_g, *w_lambda_g;     /* [G] */
  const double *v_mu_gf, *v_lambda_gf;   /* [G][num_factor] */
} fmx_als_opts;

typedef struct fmx_als_stats {
  double   train_metric;    /* rmse_train (regression, clamped) or acc_train (classification) of this iteration */
  double   device_seconds;
  uint32_t levels;          /* dependency levels of the sweep (1 launch per level and coordinate family) */
  uint32_t reserved;
  double   sum_e_sqr;       /* sum over train rows of e^2 BEFORE the sweep (draw_alpha's statistic, :918-920) */
} fmx_als_stats;

int fmx_als_begin(fmx_handle h, int train_slot);
/* statistics the hyper-prior draws need (draw_alpha :911-939, draw_w_mu/_lambda :941-1017, draw_v_mu/_lambda
 * :1019-1097), reduced on the device in fp64:
 *   out[0] = sum_c e_c^2 over the train rows (current residuals), out[1] = sum_c e_c,
 *   then a [1 + num_factor][G][2] block (G = attribute groups, 1 without fmx_set_groups): row 0 = w, row 1+f = v_f;
 *   per group g the pair {sum_{j in g} theta_j, sum_{j in g} theta_j^2}  (the per-group loops of :946-951, :987-992,
 *   :1026-1031, :1067-1072).  With one group: out[2] = sum w, out[3] = sum w^2, out[4+2f] = sum v_f, out[5+2f] = sum v_f^2.
 * out must hold 2 + 2*G*(1 + num_factor) doubles. */
int fmx_als_moments(fmx_handle h, double *out);
int fmx_als_sweep(fmx_handle h, const fmx_als_opts *opts, fmx_als_stats *stats);
int fmx_als_end(fmx_handle h);
/* the same learner over the feature shards of a group (BASELINE configs[4]: "V sharded across 8 x MI355X"): every shard
 * sweeps its own features, level by level in the GLOBAL dependency order; the {e, q} cache is replicated, one all-reduce per
 * (coordinate family, level) carries the changes of the level's draws, and the re-prediction all-reduces the shards' partial
 * y-hat and q_f (fm_learn_mcmc.h:430-641 with e / q of :46-49 replicated).  Same results as one
 * unsharded handle: ALS to rounding, MCMC draw for draw (the noise of a coordinate is keyed by its GLOBAL feature id).
 * Kept `-relation` blocks (fmx_group_upload_block_rows_ex): the per-block-row caches are replicated too, a block's levels are
 * global over its rows, and one all-reduce of 4 doubles per block row carries the cache changes of each block level. */
int fmx_group_als_begin(fmx_group g, int train_slot);
int fmx_group_als_moments(fmx_group g, double *out);
int fmx_group_als_sweep(fmx_group g, const fmx_als_opts *opts, fmx_als_stats *stats);
int fmx_group_als_end(fmx_group g);

/* ---- fm_learn_sgd_element_adapt_reg (`-method sgda`; src/libfm/src/fm_learn_sgd_element_adapt_reg.h) -------------
 * Self-adaptive regularisation: theta steps on the train rows alternate with lambda steps on the validation rows,
 * strictly online: fmx_sgda_epoch is that order on one wavefront (a parity instrument), fmx_sgda_epoch_minibatch the batch form.  Regularisation is
 * learned per attribute group (fmx_set_groups): reg_w(g), reg_v(g,f).
 *   fmx_sgda_begin : the learner's start of learn() (:256-262): w := 0, reg_w := 0, reg_v := 0, shadow gradients := 0
 *   fmx_sgda_epoch : one iteration of the epoch loop (:262-279); do_lambda_steps = 0 in the first iteration (:269)
 *   fmx_sgda_get_reg : [G][1 + num_factor]: reg[g*(1+k)] = reg_w(g), reg[g*(1+k)+1+f] = reg_v(g,f)
 *                      (what -rlog reports as regw[g], regv[g,f]; :119-132)
 */
int fmx_sgda_begin(fmx_handle h);
int fmx_sgda_epoch(fmx_handle h, int train_slot, int validation_slot, int do_lambda_steps, fmx_epoch_stats *stats);
/* the learner in BATCH form (oracle fmo_sgda_epoch_minibatch; the online order above is one wavefront and slower than the
 * reference's CPU): per batch of `batch` train rows (0 = the library's choice, as fmx_sgd_opts::batch, with this learner's doubled regression curvature) the theta steps as a minibatch rule -- this learner's
 * multiplier, reg_0 = 0, the learned regularisation 2 reg(g[,f]) theta per occurrence, the shadow gradient of a touched
 * parameter = the sum of its occurrences' gradients -- then, do_lambda_steps, the lambda steps of the next `batch` validation
 * rows (cyclic, :271-274), each as sgd_lambda_step (:201-248) with the regularisation of the batch start, their changes
 * summed and applied, clamped at 0, once.  batch = w0_chunk = 1 is the reference's loop.  w0_chunk 0 = library default. */
int fmx_sgda_epoch_minibatch(fmx_handle h, int train_slot, int validation_slot, int do_lambda_steps, uint32_t batch,
                             uint32_t w0_chunk, fmx_epoch_stats *stats);
int fmx_sgda_get_reg(fmx_handle h, double *reg /* [G][1 + num_factor] */);
int fmx_sgda_end(fmx_handle h);

/* ---- AdaGrad on the minibatch rule (a per-coordinate step size; no counterpart in the reference) ----------------------
 * Every other trainer applies one learn_rate to every coordinate, and the batch rule is only stable while
 * learn_rate * curvature * batch * C <= 1 (fmx_sgd_opts::batch).  Under AdaGrad a coordinate moves by eta * g / sqrt(n + g^2) per
 * batch: |step| < eta however many occurrences the batch sums.  A caller detects the feature by the symbol fmx_adapt_begin.
 *
 * One epoch cuts the slot's rows into batches of `batch` consecutive rows.  Per batch (steps 1 and 2 are exactly the oracle's
 * fmo_sgd_epoch_minibatch with bias_lag = 0):
 *   1. from the batch-start parameters, per example e: S_ef, rest_e;
 *   2. the bias advances in micro-chunks of `w0_chunk` examples with PLAIN SGD at fmx_config::learn_rate and reg0; mult_e is the
 *      multiplier taken with its micro-chunk's own bias.  The bias deliberately stays non-adaptive: every example touches it,
 *      and the micro-chunk rule already chooses a stable step for it;
 *   3. for every feature j that occurs in the batch, from the batch-start w_j, v_jf, its occurrences (e, x) in row order and
 *      nocc = their number (ids repeated inside a row count as separate occurrences, as everywhere else):
 *        g_w  = sum_occ mult_e * x                          + nocc * regw * w_j
 *        g_vf = sum_occ mult_e * (S_ef * x - v_jf * x * x)  + nocc * regv * v_jf
 *        n_w[j]   += g_w^2;   w_j  -= eta * g_w  / sqrt(n_w[j])       (only with k1)
 *        n_v[j,f] += g_vf^2;  v_jf -= eta * g_vf / sqrt(n_v[j,f])
 *      g is the gradient sum the plain rule multiplies by learn_rate.  The accumulators start at init_acc > 0, so there is no
 *      epsilon.  A feature that no batch touches keeps its parameters and accumulators bit for bit.
 * The device works in fp32 (n' = fmaf(g, g, n), theta' = theta - eta * g / sqrtf(n'), correctly rounded), one owner per
 * (batch, feature): no atomics, two runs of the same calls are bit-identical.
 *
 *   fmx_adapt_begin : allocates n_w[n_local] and n_v[n_local][row stride] (the stride of V's rows: num_factor rounded up to 16, or
 *                     to a power of two below 32) and sets every accumulator to init_acc: 4 * n_local * (row stride + 1) bytes stay
 *                     resident until fmx_adapt_end / fmx_destroy.  Called again it resets the accumulators (and takes the new
 *                     options).  Unlike fmx_sgda_begin NOTHING in the model is reset.  fmx_set_params, fmx_load_model and plain
 *                     fmx_sgd_epoch leave the accumulators alone while a session is open; so do plain fmx_pair_epoch and
 *                     fmx_pair_epoch_sampled, which still train with learn_rate (the session's pairwise epochs are
 *                     fmx_adapt_pair_epoch / fmx_adapt_pair_epoch_sampled, below).
 *   fmx_adapt_epoch : one epoch.  batch = 0 resolves exactly as fmx_sgd_opts::batch = 0 does (the plain rule's stability cut --
 *                     conservative on purpose); an explicit batch is honoured.  w0_chunk = 0: fmx_default_w0_chunk.  The stats are
 *                     filled as fmx_sgda_epoch_minibatch fills them (rows, batches, device_seconds, main_kernel_*,
 *                     max_feature_count, batch_used, collision_mass, batch_gain, status) plus w0_chunk_used and setup_seconds.
 *                     An empty slot returns FMX_OK with zero rows.
 *   fmx_adapt_get_state_rows : the accumulators of `count` features, gathered on the device; layout of fmx_get_param_rows
 *                     (nw_out[count], nv_out[count][num_factor]; nv_out may be NULL only when num_factor = 0).
 *   fmx_adapt_end   : frees the accumulators.
 * Refusals.  FMX_E_ARG: NULL opts, unknown rule, flags != 0, init_acc negative, NaN or infinite, learn_rate negative or NaN, NULL
 * outputs of _get_state_rows, an id >= num_attribute.  FMX_E_STATE: _epoch, _get_state_rows or _end without _begin; a slot never
 * uploaded or without targets; an open SGDA session (and fmx_sgda_begin while this session is open); an open ALS / MCMC session
 * on the slot.  FMX_E_UNSUPPORTED: a feature shard or communicator rank; kept `-relation` blocks ("relations are not supported
 * with SGD", fm_learn_sgd.h:61-63).  The handle stays usable after every refusal. */
#define FMX_ADAPT_ADAGRAD 1u
typedef struct fmx_adapt_opts {
  uint32_t rule;        /* FMX_ADAPT_ADAGRAD */
  uint32_t flags;       /* none defined: 0 */
  double   init_acc;    /* start value of every accumulator; 0 = 1.0; otherwise finite and > 0 */
  double   learn_rate;  /* eta of w and V; 0 = fmx_config::learn_rate.  The bias always uses fmx_config::learn_rate */
} fmx_adapt_opts;
int fmx_adapt_begin(fmx_handle h, const fmx_adapt_opts *opts);
int fmx_adapt_epoch(fmx_handle h, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats *stats);
int fmx_adapt_get_state_rows(fmx_handle h, const uint32_t *ids, uint32_t count, double *nw_out, double *nv_out);
int fmx_adapt_end(fmx_handle h);

/* ---- FTRL-proximal with L1 on the minibatch rule (a sparse model; no counterpart in the reference) ----------------------
 * Every other trainer's L2 only shrinks a coordinate.  FTRL-proximal (McMahan et al., "Ad click prediction: a view from the
 * trenches") with an L1 term sets a coordinate whose accumulated gradient stays small to EXACTLY zero, and fmx_param_sparsity
 * counts the zeros.  A caller detects the feature by the symbol fmx_ftrl_begin.
 *
 * One epoch cuts the slot's rows into batches of `batch` consecutive rows.  Steps 1 and 2 of a batch are exactly AdaGrad's (above,
 * "fmx_adapt_*"): S_ef and rest_e from the batch-start parameters; the bias in micro-chunks with PLAIN SGD at
 * fmx_config::learn_rate and reg0; mult_e taken with its micro-chunk's bias.  Step 3, for every feature j of the batch, from the
 * batch-start theta (w_j with k1, every v_jf) and the feature's occurrences (e, x) in row order (an id repeated inside a row counts
 * as separate occurrences):
 *        g_w  = sum_occ mult_e * x                  g_vf = sum_occ mult_e * (S_ef * x - v_jf * x * x)
 *        n'   = n + g^2         sigma = (sqrt(n') - sqrt(n)) / alpha         z' = z + g - sigma * theta
 *        D'   = (beta + sqrt(n')) / alpha + l2
 *        theta' = 0                                  if |z'| <= l1     (with l1 = 0 this catches z' == 0 and yields +0)
 *               = -(z' - sgn(z') * l1) / D'          otherwise
 *      with (l1, l2) = (l1_w, l2_w) for w and (l1_v, l2_v) for V.  g has NO nocc * reg * theta term and fmx_config::regw / regv are
 *      not read: L2 lives in the proximal step, ONE strength per coordinate, not one per occurrence as in the plain rule.
 * Start state.  n = init_acc.  V starts at random non-zero values, and the textbook z = 0 would pull a coordinate most of the way to 0
 * at its first small gradient (theta_1 ~ theta_0 * |g| / (|g| + beta)).  So fmx_ftrl_begin derives z from the parameters the model
 * holds at that moment:
 *        z_0 = -theta_0 * D_0 - sgn(theta_0) * l1,    D_0 = (beta + sqrt(init_acc)) / alpha + l2,    sgn(0) = 0
 *      at which the closed form returns theta_0; with l1 = 0 every step is theta' = theta - g / D', and for theta_0 = 0 this is the
 *      textbook rule.  With l1 = l2 = beta = 0, init_acc = a > 0, alpha = eta and regw = regv = 0 the rule IS fmx_adapt's AdaGrad.
 *      The padding of a V row (f >= num_factor) has theta = z = g = 0 and stays +0.
 * A feature that no batch touches keeps theta, z and n bit for bit; a touched coordinate is always recomputed from z'.
 * The device works in fp32 (n' = fmaf(g, g, n), correctly rounded sqrtf and /), one owner per (batch, feature): no atomics, two
 * runs of the same calls are bit-identical.
 *
 *   fmx_ftrl_begin  : allocates z_w, n_w [n_local] and z_v, n_v [n_local][row stride] (V's row stride: fmx_adapt_begin):
 *                     8 * n_local * (row stride + 1) bytes stay resident until fmx_ftrl_end / fmx_destroy; fills n with init_acc
 *                     and derives z.  Called again it resets both from the parameters of that moment (and takes the new options).
 *                     NOTHING in the model is changed.  fmx_set_params, fmx_load_model and plain fmx_sgd_epoch during a session
 *                     leave z and n alone -- the next epoch then continues from parameters z no longer describes: call
 *                     fmx_ftrl_begin again after them.  The same holds for plain fmx_pair_epoch / fmx_pair_epoch_sampled, which
 *                     still train with learn_rate (the session's pairwise epochs are fmx_ftrl_pair_epoch /
 *                     fmx_ftrl_pair_epoch_sampled, below).
 *   fmx_ftrl_epoch  : one epoch; batch = 0, w0_chunk = 0, the stats and an empty slot exactly as fmx_adapt_epoch.
 *   fmx_ftrl_get_state_rows : z and n of `count` features, gathered on the device; each pair in the layout of fmx_get_param_rows
 *                     (zw[count], zv[count][num_factor], nw[count], nv[count][num_factor]; zv / nv may be NULL only when
 *                     num_factor = 0).
 *   fmx_ftrl_end    : frees the tables.
 * Refusals.  FMX_E_ARG: NULL opts, flags != 0, a negative, NaN or infinite value, alpha (after 0 = fmx_config::learn_rate) not a
 * positive fp32 number with a finite reciprocal, beta == 0 && init_acc == 0 (D would start at 0), NULL outputs of _get_state_rows,
 * an id >= num_attribute.  FMX_E_STATE: _epoch, _get_state_rows or _end without _begin; a slot never uploaded or without targets;
 * an open SGDA or AdaGrad session (and fmx_sgda_begin / fmx_adapt_begin while this session is open); an open ALS / MCMC session
 * on the slot.  FMX_E_UNSUPPORTED: a feature shard or communicator rank; kept `-relation` blocks.  The handle stays usable after
 * every refusal. */
typedef struct fmx_ftrl_opts {
  uint32_t flags;       /* none defined: 0 */
  uint32_t reserved;    /* not read */
  double   alpha;       /* per-coordinate rate; 0 = fmx_config::learn_rate.  The bias always uses fmx_config::learn_rate */
  double   beta;        /* >= 0 (the Python binding's default is 1) */
  double   l1_w, l1_v;  /* >= 0: L1 strength of w and of V */
  double   l2_w, l2_v;  /* >= 0: L2 strength of w and of V, one per coordinate */
  double   init_acc;    /* start value of every n; >= 0, and > 0 where beta == 0 */
} fmx_ftrl_opts;
int fmx_ftrl_begin(fmx_handle h, const fmx_ftrl_opts *opts);
int fmx_ftrl_epoch(fmx_handle h, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats *stats);
int fmx_ftrl_get_state_rows(fmx_handle h, const uint32_t *ids, uint32_t count, double *zw, double *zv, double *nw, double *nv);
int fmx_ftrl_end(fmx_handle h);

/* ---- per-row weights: weighted AdaGrad / FTRL epochs and a weighted log loss ---------------------------
 * Click data is trained on a subsample: keep a fraction r of the negatives and give each kept one the weight 1 / r (the FTRL paper's
 * recipe, whose L1 half is "fmx_ftrl_*").  Without the weight the model's bias and its log loss describe the subsampled stream, not
 * the real one.  c_e is the weight of row e: finite and >= 0.  A caller detects the feature by the symbol fmx_set_row_weights.
 *
 * fmx_adapt_epoch and fmx_ftrl_epoch on a slot WITH weights: steps 1 and 3 of "fmx_adapt_*" / "fmx_ftrl_*" stay word for word.  Step 2
 * becomes, per micro-chunk with its start bias w0s:
 *        m_e  = c_e * multiplier(w0s + rest_e, y_e)              (fp32 product of the fp32 multiplier and the fp32 weight)
 *        w0  -= lr * ( sum_chunk m_e + chunk_rows * reg0 * w0s )  (fp64)
 *        mult_e = m_e
 * The weight scales the LOSS only.  The regularisation terms keep counting occurrences and rows, not weight: nocc * regw * w_j,
 * nocc * regv * v_jf, chunk_rows * reg0 * w0s; FTRL has no per-occurrence term, so for it this is the whole change.  A row of weight
 * 0 adds nothing to any gradient but still counts in nocc and chunk_rows.  All-ones weights give the unweighted rule; integer
 * weights with reg0 = regw = regv = 0 and the whole slot as one batch and one micro-chunk give the model of the set in which every
 * row is repeated c_e times.
 * The bias is plain SGD and its stability is the caller's responsibility, as the micro-chunk already is: its step per micro-chunk
 * is lr * sum_chunk c_e * curvature, so weights of mean mu act like a micro-chunk mu times longer.  Nothing is cut for it.
 * A weighted epoch runs the recurrence as a one-wavefront chain (k_scan_weighted) whatever the batch and the micro-chunk -- any
 * micro-chunk >= 1 and any batch are valid -- and reports FMX_STAT_WEIGHTED | FMX_STAT_SCAN_SERIAL in fmx_epoch_stats::status, never
 * FMX_STAT_SCAN_PIT.  Deterministic: two runs of the same calls are bit-identical.  On a slot without weights both epochs run
 * exactly the code they ran before: same launches, same bits.
 *
 *   fmx_set_row_weights : weight[n_rows] (host), kept on the device at 4 bytes per row.  A new call replaces the weights; NULL drops
 *                     them; fmx_upload_rows and its siblings, fmx_synth_rows* and fmx_free_rows drop them (free_slot), fmx_destroy
 *                     frees them.  FMX_E_ARG for a NaN, infinite or negative weight (the message names the first offending row;
 *                     nothing changes on failure), FMX_E_STATE for a slot never uploaded, FMX_E_UNSUPPORTED on a feature shard or
 *                     communicator rank (there is no group form, so no sharded path can meet a weighted slot).  An empty slot with a
 *                     non-NULL pointer is accepted.
 *   fmx_get_row_weights : the weights as stored, out[n_rows].  FMX_E_STATE when the slot has none.
 * Trainers without a weighted form REFUSE a weighted slot -- training on its targets without its weights would silently give the
 * wrong model -- with FMX_E_UNSUPPORTED, before any launch, in a message that names fmx_set_row_weights: fmx_sgd_epoch,
 * fmx_sgd_partial, fmx_sgd_finish, fmx_sgda_epoch and fmx_sgda_epoch_minibatch (for the train slot), fmx_als_begin.  Dropping the
 * weights makes them work again; the handle stays usable.  Everything that only scores IGNORES the weights: fmx_predict,
 * fmx_evaluate, fmx_evaluate_ex, fmx_evaluate_by_query, fmx_evaluate_rank, fmx_topk, fmx_compact_*, fmx_post_*, and the pair calls
 * (fmx_pair_*, fmx_adapt_pair_* / fmx_ftrl_pair_*: their examples are pairs, not rows).
 *
 * fmx_evaluate_weighted: one scoring pass like fmx_evaluate_ex (its score path, its option and slot checks), then with p_i, s_i and
 * l(z) exactly as defined there ("exact AUC and log loss of a slot"):
 *        weight_sum     = sum_i c_i          pos_weight / neg_weight = sum of c_i over target_i >= 0 / < 0
 *        correct_weight = sum_i c_i [ (p_i >= 0) == (target_i >= 0) ]                (a NaN score is never correct)
 *        loss_sum       = sum_i c_i l(s_i p_i),  logloss = loss_sum / weight_sum      (classification)
 *        sq_sum = sum_i c_i err_i^2,  abs_sum = sum_i c_i |err_i|,  rmse = sqrt(sq_sum / weight_sum),  mae = abs_sum / weight_sum
 *                                                                                     (regression, clamped as fm_learn.h:138-152)
 *        accuracy       = correct_weight / weight_sum                                 (classification)
 *   every term in fp64 from the fp32 score and the fp32 weight.  A row of weight 0 adds exactly 0 to every sum, also where l is +inf
 *   or its score NaN.  nan_rows (classification: rows whose score is NaN, whatever their weight) > 0 or weight_sum == 0 makes the four
 *   ratios NaN; the sums and counts stay right (loss_sum itself is NaN when a NaN score has a positive weight).  Classification
 *   handles leave sq_sum = abs_sum = 0 and rmse = mae = NaN; regression handles leave the classification sums 0, nan_rows 0 (a NaN
 *   score clamps to max_target, as in fmx_evaluate) and logloss = accuracy = NaN.  An empty slot: FMX_OK with zeros and NaN ratios.
 *   FMX_E_STATE when the slot has no weights; the other refusals are fmx_evaluate_ex's.
 *   Every fp64 sum runs in fmx_evaluate_ex's fixed order (block partials on the same grid, summed in block order by a final kernel;
 *   no float atomics): two calls with unchanged parameters are bit-identical except for the time.
 *   There is no weighted AUC, and it is rarely missed: weights that are constant per class -- the subsampling case -- multiply
 *   numerator and denominator of the AUC alike and cancel, so fmx_evaluate_ex's exact value is already the weighted one.
 * Added without an ABI version change. */
typedef struct fmx_eval_weighted {
  uint64_t rows, nan_rows;
  double   weight_sum, pos_weight, neg_weight, correct_weight;
  double   loss_sum, sq_sum, abs_sum;
  double   logloss, rmse, mae, accuracy;
  double   device_seconds;      /* whole call */
} fmx_eval_weighted;
int fmx_set_row_weights(fmx_handle h, int slot, const float *weight);
int fmx_get_row_weights(fmx_handle h, int slot, float *out);
/* opts as fmx_evaluate_ex (NULL = logistic) */
int fmx_evaluate_weighted(fmx_handle h, int slot, const fmx_eval_opts *opts, fmx_eval_weighted *out);

/* ---- pairwise ranking (BPR) stepped by an open session's per-coordinate rule ------------------------------------------------
 * The pairwise batch rule multiplies a (batch, feature) segment's summed gradient by ONE learn_rate; a popular item's segment sums
 * thousands of pair gradients and there is no stability cut.  These four calls run the epoch of fmx_pair_epoch /
 * fmx_pair_epoch_sampled in FMX_SGD_MINIBATCH unchanged up to the owner -- the same pairs, the same negatives (FMX_NEG_HARDEST
 * included), the same sums, multipliers and (batch, feature) bucketing, w0 -= reg0 * w0 once per pair in fp64 -- and then step every
 * touched coordinate with the open session's rule.  For every feature j of a batch, from the batch-start theta (w_j with k1, every
 * v_jf) and the segment's entries in pair order:
 *   fmx_adapt_pair_epoch*  g = sum over the pairs t of the batch that contain j of (mult_t * grad_tj + reg * theta): the sum the plain
 *                          rule multiplies by learn_rate, one regularisation term per distinct pair, in fp64; g32 = (float)g; then
 *                          n' = fmaf(g32, g32, n), theta' = theta - eta * g32 / sqrtf(n') in fp32: |theta' - theta| <= eta whatever
 *                          the batch sums.
 *   fmx_ftrl_pair_epoch*   the same sum WITHOUT the regularisation terms (L2 lives in the proximal step), g32 = (float)g, then the
 *                          proximal step of "fmx_ftrl_*" with the session's constants; a touched coordinate is recomputed from z'.
 * The state is the session's own tables: pointwise fmx_adapt_epoch / fmx_ftrl_epoch and these pairwise epochs may alternate within
 * one session.  The padding of a row beyond num_factor is never read or written; a feature that no batch touches keeps theta and
 * its state bit for bit; batch = 1 gives the per-pair rule (there is no sequential form); one owner per (batch, feature) segment, no
 * atomics: two runs of the same calls are bit-identical.  opts, flags, the stats and forced_out are those of the plain calls.
 * Refusals, each before any launch, the handle usable afterwards: everything the plain counterpart refuses; FMX_E_STATE without the
 * matching open session (and for the fmx_ftrl_ calls while an fmx_adapt session is open); FMX_E_UNSUPPORTED for FMX_SGD_SEQUENTIAL
 * and FMX_SGD_HOGWILD (the rule runs on FMX_SGD_MINIBATCH; batch = 1 is the per-pair rule).
 * The plain fmx_pair_epoch / fmx_pair_epoch_sampled are unchanged: during a session they still train with learn_rate and leave the
 * state alone (after them an FTRL session's z no longer describes the parameters: fmx_ftrl_begin again).
 * Added without an ABI version change: a caller detects the feature by the symbol fmx_adapt_pair_epoch. */
int fmx_adapt_pair_epoch(fmx_handle h, int slot, const fmx_pair_opts *opts, fmx_epoch_stats *stats);
int fmx_adapt_pair_epoch_sampled(fmx_handle h, int query_slot, const fmx_pairneg_opts *o, fmx_epoch_stats *stats, uint64_t *forced_out);
int fmx_ftrl_pair_epoch(fmx_handle h, int slot, const fmx_pair_opts *opts, fmx_epoch_stats *stats);
int fmx_ftrl_pair_epoch_sampled(fmx_handle h, int query_slot, const fmx_pairneg_opts *o, fmx_epoch_stats *stats, uint64_t *forced_out);

/* How many coordinates of the model are exactly zero -- on any unsharded handle, with or without a training session.  One pass over
 * both tables on the device, integer sums only.  `== 0.0f` decides: -0 counts, NaN does not; only f < num_factor of a row is looked
 * at (never its padding).  With num_factor = 0 every row counts as all zero.  FMX_E_ARG: out is NULL.  FMX_E_UNSUPPORTED: a feature
 * shard or communicator rank. */
typedef struct fmx_sparsity {
  uint64_t features;       /* num_attribute */
  uint64_t w_zero;         /* linear weights that are zero (counted whether or not k1 is set) */
  uint64_t v_coords;       /* features * num_factor */
  uint64_t v_zero;         /* factors that are zero */
  uint64_t v_zero_rows;    /* features whose num_factor factors are all zero */
  uint64_t dead_features;  /* such features with (w_j == 0 or k1 == 0): they contribute nothing to any prediction */
} fmx_sparsity;
int fmx_param_sparsity(fmx_handle h, fmx_sparsity *out);

/* ---- AdaGrad and FTRL over feature shards -----------------------------------------------------------
 * The group forms of "fmx_adapt_*", "fmx_ftrl_*" and fmx_param_sparsity: the same rules, options, stats and start state on a model
 * whose features are split over the members of an fmx_group.  The state of a coordinate lives with its feature: every member holds
 * the session's tables for its own n_local rows (4 * n_local * (row stride + 1) bytes for AdaGrad, 8 * ... for FTRL, per shard).
 * Per batch every shard takes its partial row sums, ONE exchange sums them over the shards, and from the summed buffer every shard
 * derives rest_e, runs the bias recurrence (all shards compute the same w0 and multipliers from the same sums, as fmx_sgd_finish
 * does) and steps the features it owns with the rule's owner kernel.  That is the rule of the per-handle call on the whole model;
 * only the association of the fp32 factor sums differs (per-shard partial sums, then their sum).  Exact schedule only: there is no
 * pipelined or bias-lag form.  One owner per (batch, feature), sums in a fixed order: two runs of the same calls are bit-identical.
 *
 *   fmx_group_adapt_begin / fmx_group_ftrl_begin : every refusal of the per-handle call, with its code and message, for every
 *                     member before any member is touched; then the session opens on every member.  If a member cannot allocate its
 *                     tables the sessions already opened by this call are closed and the error is returned: all or nothing.
 *   fmx_group_adapt_epoch / fmx_group_ftrl_epoch : one epoch.  batch = 0 resolves to the batch ONE unsharded handle would choose on
 *                     the same rows (the collision mass summed over the shards, as fmx_group_sgd_epoch); w0_chunk = 0:
 *                     fmx_default_w0_chunk.  The stats are filled as fmx_adapt_epoch fills them; status is OR-ed over the shards,
 *                     setup_seconds and max_feature_count are the largest of any shard.  An empty slot returns FMX_OK with zero rows.
 *   fmx_group_adapt_get_state_rows / fmx_group_ftrl_get_state_rows : the layouts of the per-handle calls (FTRL: z before n).  ids
 *                     are GLOBAL feature ids in any order, repeats allowed; each is read on the shard that owns it.
 *   fmx_group_adapt_end / fmx_group_ftrl_end : closes the session on every member.  fmx_destroy of a member and fmx_group_destroy
 *                     followed by it free the member's tables as always.
 *   fmx_group_param_sparsity : the sum of the shards' counts; equal, field for field, to fmx_param_sparsity of one unsharded handle
 *                     holding the same parameters.
 * A group of one unsharded handle forwards every call to the per-handle form (same bits).  Shards that share a device and shards on
 * distinct devices (RCCL) run the same driver.
 * Refusals, each before any launch, the group usable afterwards.  FMX_E_STATE: _epoch, _get_state_rows or _end before _begin; _begin
 * while the other optimiser's session or an SGDA session is open on any member; an open ALS / MCMC session on any member; members
 * holding different row counts in the slot; a destroyed member.  FMX_E_UNSUPPORTED: a slot with kept `-relation` blocks; a slot with
 * row weights on any member; a member that is a communicator rank (fmx_comm_init_rank).  FMX_E_ARG: as the per-handle calls.
 * Not offered on shards: row weights, the pairwise epochs.  The per-handle fmx_adapt_*, fmx_ftrl_*, fmx_param_sparsity
 * and fmx_checkpoint_* keep refusing a shard handle or group member with FMX_E_UNSUPPORTED; the group form of the checkpoint is
 * fmx_group_checkpoint_save / _load (declared after fmx_checkpoint_*, whose types it takes).
 * Added without an ABI version change: a caller detects the feature by the symbol fmx_group_adapt_begin. */
int fmx_group_adapt_begin(fmx_group g, const fmx_adapt_opts *opts);
int fmx_group_adapt_epoch(fmx_group g, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats *stats);
int fmx_group_adapt_get_state_rows(fmx_group g, const uint32_t *ids, uint32_t count, double *nw_out, double *nv_out);
int fmx_group_adapt_end(fmx_group g);
int fmx_group_ftrl_begin(fmx_group g, const fmx_ftrl_opts *opts);
int fmx_group_ftrl_epoch(fmx_group g, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats *stats);
int fmx_group_ftrl_get_state_rows(fmx_group g, const uint32_t *ids, uint32_t count, double *zw, double *zv, double *nw, double *nv);
int fmx_group_ftrl_end(fmx_group g);
int fmx_group_param_sparsity(fmx_group g, fmx_sparsity *out);

/* ---- a bf16 serving snapshot of the model (no counterpart in the reference) ------------------------
 * Every scoring pass is a random gather of factor rows and is paid for in the bytes of those rows.  Training needs them in fp32 (an
 * update adds learn_rate * g to values a thousand times larger); scoring does not.  fmx_compact_begin takes a frozen, read-only copy
 * of the model with V rounded to bfloat16 -- half the bytes per gathered row, half the memory of a second resident model -- and the
 * other fmx_compact_* calls score from that copy.  No other entry point reads it.  A caller detects the feature by the symbol
 * fmx_compact_begin.
 *
 * Format.  bf16 is the upper half of an fp32: round to nearest, ties to even, on bit 16 -- for a bit pattern u that is not a NaN,
 * (u + 0x7FFF + ((u >> 16) & 1)) >> 16.  +-0, +-inf and fp32 subnormals follow the same rule; a finite value above bf16's largest
 * becomes +-inf; a NaN stays a NaN with its quiet bit set.  Scoring widens a value back with a 16-bit shift, so a score is fm_model::
 * predict of the model (w0, w, q(V)) in the arithmetic of fmx_predict.
 *
 *   fmx_compact_begin       : brings the model up to date, then copies w0, w (fp32, a plain copy) and V as bf16 rows of V's row
 *                             stride rs (2 * rs bytes each, the padding behind num_factor kept at +0):
 *                             n_local * (2 * rs + 4) bytes stay resident until fmx_compact_end / fmx_destroy.  Called again it
 *                             replaces the snapshot.  The model itself is never written, and nothing that happens to it afterwards
 *                             -- epochs of any trainer, fmx_set_params, fmx_load_model -- changes what the calls below return.
 *                             Independent of SGDA / AdaGrad / FTRL / ALS sessions: it may be taken and used while one is open.
 *   fmx_compact_predict     : fmx_predict from the snapshot (its w0, its w, its rows).
 *   fmx_compact_evaluate    : fmx_evaluate from the snapshot; device_seconds is filled, FMX_EVAL_WSIDE never set (the weight side
 *                             stream describes the live w, not the snapshot's).
 *   fmx_compact_evaluate_ex : fmx_evaluate_ex from the snapshot: the same reduction over the snapshot's scores.
 *   fmx_compact_topk        : fmx_topk with the factor sums of both slots taken from the snapshot; the score-and-select kernels
 *                             and every rule of the lists are fmx_topk's.
 *   fmx_compact_get_rows    : w and the dequantised factors of `count` features in the layout of fmx_get_param_rows (w_out[count],
 *                             v_out[count][num_factor]; v_out may be NULL only when num_factor = 0).
 *   fmx_compact_end         : frees the snapshot.
 *
 * FMX_COMPACT_INT8: the row-wise 8-bit format.  Every call above serves it.  One aligned block of P bytes per
 * feature holds the row's k int8 codes, one fp32 scale and w_j (fp32, unchanged) -- there is no separate w array, and a scoring pass
 * makes ONE access per entry where fp32 and bf16 make two.  P = fmx_compact_row_bytes(FMX_COMPACT_INT8, k): the power of two >= k + 8
 * up to 128 (k = 64: 128, k = 32: 64, k = 0: 8), k + 8 rounded up to 64 above (k = 128: 192).  Per row, in fp64: a = max_f |v_f|,
 * q_f = clamp(rint(v_f * (127.0 / a)), -127, 127) with ties to even (all 0 when a = 0), scale = (float)(a / 127.0).  A factor
 * dequantises to the fp32 product scale * (float)q_f, which fmx_compact_get_rows returns exactly: an exact zero stays zero, the largest
 * factor of a row has code +-127, |v - deq| <= (a / 127) (0.5 + a few fp32 roundings).  A row with a non-finite factor has scale NaN
 * and codes 0: all of it dequantises to NaN and every score that touches it is NaN, as from the model; fmx_compact_info::nonfinite
 * counts its num_factor coordinates, max_abs_err and sum_sq_err are |v - deq| over the other rows, bytes_compact = n_local * P.
 *
 * Refusals, each before any launch.  FMX_E_ARG: NULL opts, a format other than FMX_COMPACT_BF16 / FMX_COMPACT_INT8, flags != 0, NULL outputs, an
 * id >= num_attribute, whatever fmx_evaluate_ex / fmx_topk refuse in their own arguments.  FMX_E_STATE: any call but _begin without
 * a snapshot; a slot never uploaded, or without targets where targets are needed.  FMX_E_UNSUPPORTED: a feature shard or
 * communicator rank; a slot with kept `-relation` blocks.  The handle stays usable after every refusal. */
#define FMX_COMPACT_BF16 1u
#define FMX_COMPACT_INT8 3u   /* (2 is not assigned) */
typedef struct fmx_compact_opts {
  uint32_t format;          /* FMX_COMPACT_BF16 or FMX_COMPACT_INT8 */
  uint32_t flags;           /* none defined: 0 */
} fmx_compact_opts;
typedef struct fmx_compact_info {
  uint64_t features;        /* n_local */
  uint64_t bytes_compact;   /* device bytes of the snapshot: n_local * fmx_compact_row_bytes(format, num_factor) */
  uint64_t bytes_params;    /* fmx_info::bytes_params, for comparison */
  uint64_t nonfinite;       /* bf16: coordinates f < num_factor whose bf16 value is inf or NaN; int8: num_factor per row with a
                               non-finite factor (all of such a row dequantises to NaN) */
  double   max_abs_err;     /* max |v - q(v)|, f < num_factor: bf16 over the finite q(v), int8 over the rows without a non-finite factor */
  double   sum_sq_err;      /* sum (v - q(v))^2 over the same, fp64, partial sums added in a fixed order */
} fmx_compact_info;
int fmx_compact_begin(fmx_handle h, const fmx_compact_opts *opts, fmx_compact_info *info /* may be NULL */);
int fmx_compact_predict(fmx_handle h, int slot, double *out);
int fmx_compact_evaluate(fmx_handle h, int slot, fmx_eval *out);
int fmx_compact_evaluate_ex(fmx_handle h, int slot, const fmx_eval_opts *opts, fmx_eval_ex *out);
int fmx_compact_topk(fmx_handle h, int query_slot, int cand_slot, const fmx_topk_opts *opts, uint32_t *idx_out, double *score_out,
                     fmx_topk_stats *stats);
int fmx_compact_get_rows(fmx_handle h, const uint32_t *ids, uint32_t count, double *w_out, double *v_out);
int fmx_compact_end(fmx_handle h);
/* host arithmetic, no handle: snapshot bytes per feature -- 2 * rs + 4 for bf16 (rs = V's DEFAULT row stride in elements: num_factor
 * rounded up to 16 from 32 on, the power of two below; a process run with FMX_ROW_STRIDE_KP=1 pads rows to the power of two and its
 * fmx_compact_info::bytes_compact says so), P for int8 (which does not depend on the stride), 0 for an unknown format or num_factor < 0 */
uint32_t fmx_compact_row_bytes(uint32_t format, int num_factor);

/* ---- a pruned serving snapshot: only the rows that can score ------------------------------------
 * fmx_compact_begin stores one row per feature id, whatever the model holds there.  fmx_compact_begin_pruned stores a row only for
 * the features that can contribute to a score, in ascending id order ("slots"), and a rank directory that maps a feature id to its
 * slot: one 8-byte pair {bits, base} per 32 consecutive ids (bit b of bits: id 32 j + b is kept; base: kept ids below 32 j), so
 * slot = base + popcount(bits below b) and bytes_directory = 8 * ceil(n_local / 32).  Added without an ABI version change: a caller
 * detects the feature by the symbol fmx_compact_begin_pruned.
 *
 *   dead  : fmx_param_sparsity's dead_features rule -- all num_factor factors == 0.0f (-0 counts, NaN does not) and (w_j == 0.0f or
 *           k1 == 0); with num_factor = 0 every factor row counts as all zero.
 *   seen  : the id stands in at least one entry of keep_slot, whatever the value.
 *   kept  : not dead, and seen when FMX_PRUNE_SEEN is set.
 *
 * The snapshot replaces any earlier snapshot of the handle, dense or pruned, and fmx_compact_begin replaces a pruned one; lifetime and
 * independence from training sessions are those of fmx_compact_begin (keep_slot is read during the call only).  fmx_compact_predict /
 * _evaluate / _evaluate_ex / _topk / _get_rows / _end work unchanged on it: a dropped feature behaves as a row of +0 with w_j = +0
 * (fmx_compact_get_rows returns zeros for it), and every score is, bit for bit, the score from the dense snapshot of the model with
 * the dropped rows set to +0.  fmx_compact_info: bytes_compact = bytes_directory + bytes_rows, bytes_rows = kept *
 * fmx_compact_row_bytes(format, num_factor) (bf16: the factor rows and the w array both hold `kept` entries); nonfinite, max_abs_err
 * and sum_sq_err run over the kept rows only.
 *
 *   fmx_compact_slot_of : the slot of each of `count` ids, 0xFFFFFFFF for a dropped one.  FMX_E_STATE without a pruned snapshot.
 *
 * Refusals, each before any launch, the handle usable afterwards.  FMX_E_ARG: NULL opts, an unknown format, flags without
 * FMX_PRUNE_DEAD or with unknown bits, reserved != 0, keep_slot != -1 without FMX_PRUNE_SEEN, a keep_slot out of range, an id >=
 * num_attribute.  FMX_E_STATE: FMX_PRUNE_SEEN with a slot that was never uploaded.  FMX_E_UNSUPPORTED: a feature shard or
 * communicator rank; a keep_slot with kept `-relation` blocks. */
#define FMX_PRUNE_DEAD 1u  /* drop features that contribute to no prediction */
#define FMX_PRUNE_SEEN 2u  /* also drop features with no entry in keep_slot */
typedef struct fmx_compact_prune_opts {
  uint32_t format;     /* FMX_COMPACT_BF16 | FMX_COMPACT_INT8 */
  uint32_t flags;      /* FMX_PRUNE_DEAD, or FMX_PRUNE_DEAD | FMX_PRUNE_SEEN */
  int32_t  keep_slot;  /* with FMX_PRUNE_SEEN: an uploaded slot; else -1 */
  uint32_t reserved;   /* 0 */
} fmx_compact_prune_opts;
typedef struct fmx_compact_prune_info {
  uint64_t features;         /* n_local */
  uint64_t kept;
  uint64_t dropped_dead;
  uint64_t dropped_unseen;   /* not dead, but absent from keep_slot */
  uint64_t bytes_directory;
  uint64_t bytes_rows;
} fmx_compact_prune_info;
int fmx_compact_begin_pruned(fmx_handle h, const fmx_compact_prune_opts *o,
                             fmx_compact_info *info, fmx_compact_prune_info *pinfo); /* either may be NULL */
int fmx_compact_slot_of(fmx_handle h, const uint32_t *ids, uint32_t count, uint32_t *slot_out);

/* ---- exact binary checkpoints of the model and the optimizer state (no counterpart in the reference) -------
 * fmx_save_model / fmx_load_model speak the reference's text format: six significant digits per number, and nothing of an open
 * AdaGrad or FTRL session.  A checkpoint is the other file: w0 in fp64, w and V in fp32 without the row padding and, if an
 * fmx_adapt or fmx_ftrl session is open, that session's constants and tables -- written straight from the device tables and read
 * straight back into them, bit for bit.  The stateful epochs are deterministic, so "train 2 epochs" and "train 1, save, new
 * process, load, train 1" give the same bits.  The byte layout is csrc/fmx_ckpt_format.h (restated by libfm_amd/checkpoint.py).
 * Added without an ABI version change: a caller detects the feature by the symbol fmx_checkpoint_save.
 *
 *   fmx_checkpoint_save : brings the model up to date (as fmx_save_model), synchronises, then streams the sections through two pinned
 *                         buffers.  Writes to `path` + ".tmp" and renames, so a file at `path` is never a partial one; on failure
 *                         the .tmp file is removed.  The file holds no time stamp, host name or pointer: equal state and equal flags
 *                         give byte-identical files.  With a session the state is SPARSE by default: the file holds the state rows of
 *                         the features whose row fmx_*_begin would NOT reproduce from the file's own parameters (AdaGrad: n_w or one
 *                         of the num_factor n_v differs from init_acc; FTRL: some (z, n) differs from the start state of its
 *                         parameter), as an ascending id list and one (1 + num_factor)-float row per id and table (the linear
 *                         coordinate first).  FMX_CKPT_DENSE_STATE writes every feature's rows and no id list.  Both forms load to
 *                         the same bits.  Without k1 the file holds no w and the criterion reads the handle's w table as it is.
 *   fmx_checkpoint_load : the geometry (num_attribute, num_factor, k0, k1) must equal the handle's.  w0, w (with k1) and V are
 *                         replaced bit for bit, the padding of a V row is left +0, and whatever is derived from the parameters is
 *                         invalidated as fmx_load_model does it.  An open serving snapshot is a frozen copy and is untouched.
 *                         A file WITH a session, without FMX_CKPT_MODEL_ONLY: any open fmx_adapt / fmx_ftrl session is replaced by
 *                         the file's (the tables are reused when the kind matches, otherwise freed and allocated); its constants are
 *                         the fp32 values the saved session used, not re-derived from doubles; its tables are the start state of the
 *                         loaded parameters with the stored rows scattered over it -- the saved state on every coordinate.
 *                         A file WITHOUT a session leaves an open session alone, as fmx_load_model does.
 *   fmx_checkpoint_info : the header alone: no handle, no device.  Fills info (seconds = 0) or returns FMX_E_ARG with the reason in
 *                         err (truncated to err_len; may be NULL).
 *
 * Refusals that change nothing, each decided from the header, its section table and the file's length before the first byte
 * reaches the device; the handle stays usable.  FMX_E_ARG: NULL path, unknown flags, a file that cannot be opened or created, bad
 * magic or version, a header whose checksum fails, a geometry mismatch (the message names the field and both values), section
 * sizes that do not add up to the file's length (truncation), state_rows > num_attribute.  FMX_E_STATE: a load during an open SGDA
 * or ALS / MCMC session.  FMX_E_UNSUPPORTED: a feature shard or communicator rank.
 * Found while streaming: a section whose checksum -- computed over what ARRIVED IN DEVICE MEMORY, so it covers file, host and
 * device -- does not match, or an id list that is not strictly ascending or holds an id >= num_attribute (checked on the device
 * before any row is scattered).  FMX_E_ARG naming the section; the parameters are then unspecified and any fmx_adapt / fmx_ftrl
 * session is closed, as the message says; the handle stays usable (fmx_set_params, or load again).
 * Checksum of a section: pad it with zero bytes to a multiple of 8; the sum mod 2^64, over its little-endian 8-byte words u_i, of
 * mix64(u_i ^ (i * 0x9E3779B97F4A7C15)), mix64 being the finaliser x ^= x >> 30, x *= 0xBF58476D1CE4E5B9, x ^= x >> 27,
 * x *= 0x94D049BB133111EB, x ^= x >> 31. */
#define FMX_CKPT_DENSE_STATE 1u   /* save: write every feature's state rows, not only those that differ from the start state */
#define FMX_CKPT_MODEL_ONLY  2u   /* save: write no session even if one is open; load: ignore the file's session, leave the handle's alone */
typedef struct fmx_ckpt_opts { uint32_t flags; uint32_t reserved; } fmx_ckpt_opts;      /* NULL = no flags */
typedef struct fmx_ckpt_info {
  uint32_t version, session;          /* session: 0 none, 1 AdaGrad, 2 FTRL */
  uint64_t num_attribute; uint32_t num_factor, k0, k1, flags;
  uint64_t state_rows;                /* rows of state in the file (= num_attribute when dense) */
  uint64_t bytes;                     /* file size */
  double   seconds, device_seconds;   /* whole call / kernels and copies */
} fmx_ckpt_info;
int fmx_checkpoint_save(fmx_handle h, const char *path, const fmx_ckpt_opts *opts, fmx_ckpt_info *info /* may be NULL */);
int fmx_checkpoint_load(fmx_handle h, const char *path, const fmx_ckpt_opts *opts, fmx_ckpt_info *info /* may be NULL */);
int fmx_checkpoint_info(const char *path, fmx_ckpt_info *info, char *err, size_t err_len);   /* header only; no handle, no GPU */

/* ---- group checkpoints: the same file in global feature order, whatever the shard count ------------------
 * The group forms of fmx_checkpoint_save / _load, for the model and the fmx_group_adapt_* / fmx_group_ftrl_* session that the members
 * of an fmx_group hold between them.  Everything said above holds with "the handle" read as "the model the group holds".  The file
 * is the SAME file: the group writes, byte for byte, what one unsharded handle holding the same parameters and session would write,
 * so it does not record how the model was sharded.  A group of any shard count and either shard_hash loads it, one unsharded handle
 * loads it through fmx_checkpoint_load (and goes on to fmx_save_model, fmx_compact_*, fmx_serve_open), and two saves of equal state
 * from any two groups are byte-identical.  Same format, same version.
 * Added without an ABI version change: a caller detects the feature by the symbol fmx_group_checkpoint_save.
 *
 *   fmx_group_checkpoint_save : every member packs the rows it owns into a chunk of its own, the chunks meet on member 0's device
 *                         (the lead) and are merged there into the chunk the file gets; the lead forms the checksums and writes.
 *                         The sparse id list is the members' flagged rows as global ids, sorted on the lead.  w0 is replicated:
 *                         member 0's is written.
 *   fmx_group_checkpoint_load : the lead reads, forms every checksum over what arrived in ITS device memory and validates the id
 *                         list over its whole length before the list reaches a member and before a row is scattered; every member
 *                         stores the rows it owns.  w0 is set on every member.  Sessions, all members or none: a file with a
 *                         session replaces the session of every member; a file without one, or FMX_CKPT_MODEL_ONLY, leaves
 *                         every member's alone.
 *   info is filled as by the per-handle calls; device_seconds is the sum over the lead's chunks.
 *
 * Refusals that change nothing, the group usable afterwards, the message in fmx_group_last_error: every refusal fmx_checkpoint_load
 * decides from the header, with its code and message shape, against the group's GLOBAL geometry; FMX_E_ARG for a NULL group, a NULL
 * path or unknown flags; FMX_E_STATE for a load during an open SGDA or ALS / MCMC session on any member, for a destroyed member and
 * for members that hold different kinds of session or describe different models; FMX_E_UNSUPPORTED for a member that is a
 * communicator rank (fmx_comm_init_rank: its peers live in other processes).
 * Found while streaming (checksum, bad id list, read error): FMX_E_ARG naming the section; the parameters are then unspecified on
 * every member and every member's fmx_adapt / fmx_ftrl session is closed, as the message says; the group stays usable.
 * A group of one unsharded handle takes the per-handle path: same bits, same bytes. */
int fmx_group_checkpoint_save(fmx_group g, const char *path, const fmx_ckpt_opts *opts, fmx_ckpt_info *info /* may be NULL */);
int fmx_group_checkpoint_load(fmx_group g, const char *path, const fmx_ckpt_opts *opts, fmx_ckpt_info *info /* may be NULL */);

/* ---- a serving snapshot as a file, and a handle that serves from it without the model -------------------
 * fmx_compact_begin* need the fp32 model beside the snapshot they take.  These four calls let a snapshot leave the handle that made it:
 * fmx_compact_save writes it, straight from its device tables, to a file of its own format (csrc/fmx_snap_format.h, restated by
 * libfm_amd/compact.py: same conventions and section checksum as the checkpoint, magic "FMXSNAP\0", version 1), and fmx_serve_open
 * makes a SERVE-ONLY handle from such a file alone: no parameter tables, no placement probe -- its device memory and start-up are the
 * snapshot's.  Added without an ABI version change: a caller detects the feature by the symbol fmx_compact_save.
 *
 * The file holds the format, the geometry (num_attribute, num_factor, k0, k1), task / min_target / max_target (scoring clamps and
 * links by them), pruned and kept, the int8 block size, the figures of fmx_compact_info and fmx_compact_prune_info as they were when
 * the snapshot was taken, then the sections w0 (f64); dir (pruned: the rank directory as the device holds it); int8: rows (the P-byte
 * blocks verbatim); bf16: w (f32) and V (rows of num_factor bf16, WITHOUT the device table's row padding: the file does not depend on
 * FMX_ROW_STRIDE_KP).  No time stamp, host name or pointer: equal snapshots give byte-identical files.
 *
 *   fmx_compact_save  : needs a snapshot (FMX_E_STATE otherwise).  Streams the sections through two pinned buffers, each section's
 *                       checksum formed on the device; writes `path` + ".tmp" and renames, the .tmp file removed on failure.  Touches
 *                       neither the model nor the snapshot.  Works on a serve-only handle: saving what was loaded gives the same bytes.
 *   fmx_compact_load  : the file's num_attribute, num_factor, k0, k1 must equal the handle's (FMX_E_ARG naming the field and both
 *                       values); task / min / max are NOT compared, the handle's own hold.  The new snapshot is built beside the
 *                       handle's and replaces it only after every section's checksum -- over what arrived in device memory -- has
 *                       matched and, for a pruned file, the directory has been validated on the device (bases = running popcounts
 *                       from 0, no bit at or beyond num_attribute, total = kept: without it a file with valid checksums and a wrong
 *                       directory would send scoring kernels out of bounds).  ANY failure leaves the handle's snapshot, if any, and
 *                       its model exactly as they were.  bf16 rows are unpacked to the handle's own row stride, padding +0.
 *   fmx_snapshot_info : the header alone: no handle, no device.  Fills info (seconds = bytes_compact = 0) or returns FMX_E_ARG with
 *                       the reason in err (truncated to err_len; may be NULL).
 *   fmx_serve_open    : a serve-only handle on `device` (-1: the current one), unsharded, whose config is the file's geometry, task
 *                       and target range; then fmx_compact_load.  On any failure *out = NULL and fmx_last_error(NULL) has the reason.
 *
 * A serve-only handle has everything fmx_create makes except the parameter tables.  These calls work on it: fmx_destroy,
 * fmx_last_error, fmx_get_info (bytes_params = 0), fmx_get_place_info (method 0, no chunks, 0 seconds), fmx_synchronize, the row side
 * (fmx_upload_rows, fmx_upload_block_rows[_ex], fmx_synth_rows[_ex], fmx_free_rows, fmx_rows_info, fmx_download_rows), and
 * fmx_compact_predict / _evaluate / _evaluate_ex / _topk / _get_rows / _slot_of / _end / _save / _load.  EVERY other call that takes a
 * handle -- fmx_compact_begin and fmx_compact_begin_pruned, fmx_comm_init_rank and fmx_group_create with such a member included --
 * refuses it first thing: FMX_E_STATE "a serve-only handle holds no model", nothing launched, the handle usable afterwards.
 *
 * Other refusals, the handle usable afterwards.  FMX_E_ARG: NULL path; a file that cannot be opened or created; whatever the header,
 * its section table and the file's length show before any byte reaches the device (bad magic or version, a header checksum
 * mismatch, an unknown format, a geometry no handle can have, kept > num_attribute or kept without pruned, a block size other than
 * fmx_compact_row_bytes(FMX_COMPACT_INT8, num_factor), a section table that is not the plan of the header's fields, a planned length
 * other than the file's); a section checksum mismatch or an inconsistent directory, naming the section.  FMX_E_UNSUPPORTED:
 * fmx_compact_save / _load on a feature shard or communicator rank. */
typedef struct fmx_snap_info {
  uint32_t version, format;           /* format: FMX_COMPACT_BF16 | FMX_COMPACT_INT8 */
  uint64_t num_attribute; uint32_t num_factor, k0, k1; int32_t task;
  double   min_target, max_target;
  uint32_t pruned, row_bytes;         /* row_bytes: the int8 block size P, 0 for bf16 */
  uint64_t kept, rows;                /* kept: 0 unless pruned; rows the tables hold: kept, or num_attribute */
  uint64_t nonfinite; double max_abs_err, sum_sq_err;   /* fmx_compact_info, as the snapshot was taken */
  uint64_t dropped_dead, dropped_unseen;                /* fmx_compact_prune_info (features = num_attribute, kept above) */
  uint64_t bytes;                     /* file size */
  uint64_t bytes_compact;             /* device bytes of the snapshot on the handle (its row stride); 0 from fmx_snapshot_info */
  double   seconds, device_seconds;   /* whole call / kernels and copies */
} fmx_snap_info;
int fmx_compact_save(fmx_handle h, const char *path, fmx_snap_info *info /* may be NULL */);
int fmx_compact_load(fmx_handle h, const char *path, fmx_snap_info *info /* may be NULL */);
int fmx_snapshot_info(const char *path, fmx_snap_info *info, char *err, size_t err_len);   /* header only; no handle, no GPU */
int fmx_serve_open(const char *path, int device, fmx_handle *out, fmx_snap_info *info /* may be NULL */);

/* ---- introspection --------------------------------------------------------------------------- */
typedef struct fmx_info {
  uint64_t n_local;         /* features held by this handle */
  int32_t  k_padded;        /* floats per example in the partial-sum buffers: the power of two >= k (a device ROW is k rounded up to 16) */
  int32_t  device;
  uint64_t bytes_params;    /* device bytes of w + V */
  char     device_name[64];
  char     arch[32];        /* e.g. "gfx950" */
} fmx_info;
int fmx_get_info(fmx_handle h, fmx_info *out);
int fmx_synchronize(fmx_handle h);

#ifdef __cplusplus
}
#endif
#endif /* FMX_H_ */
