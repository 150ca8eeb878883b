// fmx_internal.h -- shared by the translation units of libfmx.so (fmx_core.hip, fmx_sgd.hip, fmx_als.hip, fmx_comm.hip, fmx_pair.hip, fmx_topk.hip,
// fmx_pairneg.hip, fmx_eval.hip, fmx_post.hip, fmx_evalq.hip, fmx_compact.hip, fmx_rankq.hip, fmx_mem.hip, fmx_weighted.hip, fmx_ckpt.hip, fmx_snap.hip; fmx_io.hip needs
// none of it).
// The C-ABI is include/fmx.h; nothing declared here is exported.
#pragma once
#pragma GCC visibility push(default)      // the C-ABI is the only thing libfmx.so exports (-fvisibility=hidden)
#include "../../include/fmx.h"
#pragma GCC visibility pop
#include "fmx_kernels.h"
#include "fmx_als_kernels.h"
#include "fmx_compact_kernels.h"
#include "fmx_place_plan.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

using namespace fmx;

struct Slot {
  Entry*    ent = nullptr;
  uint64_t* row_ptr = nullptr;
  float*    target = nullptr;
  uint32_t  n_rows = 0;
  uint64_t  nnz = 0;
  uint32_t  max_row = 0;
  uint32_t  fixed_nnz = 0;           // != 0: every row holds exactly this many entries (row r starts at r * fixed_nnz)
  // id-only stream of the one-pass SGD kernel (ensure_ids, fmx_core.hip): ids[i] = ent[i].id where fixed_nnz != 0 and EVERY value is 1.0f
  // (one-hot field data), else nullptr.  4 bytes per entry next to the entries' 8; built once per upload, freed with the slot.
  uint32_t* ids = nullptr;
  bool      ids_asked = false;       // the slot's values have been looked at (ids == nullptr then: not such a slot, or FMX_IDS=0)
  bool      used = false;
  double    coll_mass = -1.0;        // collision mass of the rows (ensure_coll_mass); < 0: not computed yet
  double    coll_mass_world = -1.0;  // one process per GPU: the shards' shares summed over the communicator (one collective per slot)
  // per-batch transposed rows for FMX_APPLY_SEGMENTED (built lazily for one batch size)
  uint32_t  seg_B = 0;
  TEntry*   t_ent = nullptr;
  uint32_t* seg_feat = nullptr;
  uint32_t* seg_rel = nullptr;
  uint32_t  nseg = 0;
  bool      all_ones = false;        // every value of the slot is 1.0f (found while the segments are built)
  uint32_t  max_seg_count = 0;       // occurrences of the most frequent feature inside one batch
  std::vector<uint32_t> batch_seg;   // [n_batches+1] first segment of every batch
  std::vector<uint64_t> batch_base;  // [n_batches+1] first entry of every batch
  // FMX_APPLY_FUSED (k_fused<FUSED_EXACT>): which entries the one-pass kernel must leave to k_apply_seg
  uint64_t* cmask = nullptr;         // [n_rows] bit i: entry i's feature occurs more than once in the row's batch
  uint32_t* cseg = nullptr;          // [ncseg] batch-local indices of the segments k_apply_seg finishes
  uint32_t  ncseg = 0;
  CDesc*    cdesc = nullptr;         // [ncseg] the same list as 32-byte records {feature, first entry, end entry, index, first two occurrences}
  uint32_t  fused_cap = 0;           // longest row the k_fused instance of this slot keeps in registers
  std::vector<uint32_t> cbatch;      // [n_batches+1] first cseg entry of every batch
  uint32_t* d_batch_seg = nullptr;   // the three per-batch tables on the device (same contents as batch_seg / cbatch / batch_base)
  uint32_t* d_cbatch = nullptr;
  uint64_t* d_batch_base = nullptr;
  // weight side stream (fmx_kernels.h row_sums; FMX_FLAG_KEEP_WSIDE): wside[i] = w[id of entry i] or NaN, lmask[row] = which entries are
  // the last occurrence of their feature in the slot; current while wside_version == the handle's w_version
  float*    wside = nullptr;
  uint64_t* lmask = nullptr;
  uint64_t  wside_version = 0;
  // training-side weight stream (fmx_kernels.h WTrain; ensure_wtrain): smask[row] = which entries are singles, soff[row] = singles in front
  // of the row (n_rows + 1 elements), wtrain = one float per single; holds the current w while wtrain_version == the handle's w_version
  uint64_t* smask = nullptr;
  uint32_t* soff = nullptr;
  float*    wtrain = nullptr;
  uint64_t  wtrain_n = 0;            // singles of the slot (whether or not the stream was kept)
  uint64_t  wtrain_version = 0;
  bool      wtrain_asked = false;    // the slot's singles have been counted (wtrain == nullptr then: too few of them, or FMX_WTRAIN=0)
  // FMX_SGD_SEQUENTIAL: the slot cut into maximal runs of consecutive rows that share no feature (fmx_seq_kernels.h "Conflict-free runs")
  std::vector<uint32_t> run_start;   // [n_runs + 1]; empty: not built
  std::vector<uint8_t>  run_single;  // [n_runs] 1: one row that repeats an id (entry-by-entry kernel)
  std::vector<struct BlockRows*> blocks;   // `-relation` blocks kept apart from these (main) rows; empty: plain / expanded rows
  // pairwise ranking (fmx_upload_pairs, fmx_pair.hip): row pair_a[t] is preferred to row pair_b[t]
  bool      pairs_set = false;
  uint64_t  n_pairs = 0;
  uint32_t* pair_a = nullptr;
  uint32_t* pair_b = nullptr;
  uint64_t* pair_off = nullptr;      // [n_pairs + 1] first entry of every pair in the pair-expanded stream (x_a, then x_b)
  uint64_t  pair_nnz = 0;            // entries of that stream
  uint32_t  pair_max_len = 0;        // longest |x_a| + |x_b| of a pair
  // its (batch, feature) bucketing for FMX_SGD_MINIBATCH, built for one batch size
  uint32_t  pair_seg_B = 0;
  TEntry*   pair_t_ent = nullptr;    // [pair_nnz] sorted payload {pair in batch << 1 | side, value}
  uint32_t* pair_seg_head = nullptr; // [pair_nseg + 1] first sorted entry of every segment
  uint32_t* pair_seg_feat = nullptr; // [pair_nseg]
  uint32_t  pair_nseg = 0, pair_max_seg = 0;
  std::vector<uint32_t> pair_batch_seg;   // [n_batches + 1] first segment of every batch
  // interactions (fmx_upload_interactions, fmx_pairneg.hip): this slot's rows are the queries, another slot's the candidates
  struct PairNeg* pneg = nullptr;
  // posterior accumulator (fmx_post_begin, fmx_post.hip); on a group it lives on the first shard's slot
  struct PostAcc* post = nullptr;
  // per-row query ids (fmx_set_row_queries, fmx_evalq.hip); on a group they live on the first shard's slot, next to the targets
  uint32_t* qid = nullptr;           // [n_rows]
  uint32_t  n_queries = 0;           // 0: the slot has no query ids
  // per-row weights (fmx_set_row_weights, fmx_weighted.hip); single handles only
  float*    weight = nullptr;        // [n_rows]
  bool      weighted = false;        // the slot has weights (an empty slot has them without an array)
};
void free_pairs(Slot& s);                                                // fmx_pair.hip
void free_interactions(Slot& s);                                         // fmx_pairneg.hip
void drop_interactions(fmx_handle h, int slot);                          // fmx_pairneg.hip: those that live on `slot` or name it as their candidate slot

// one `-relation` block kept apart from the main rows (fmx_upload_block_rows_ex, FMX_BLOCKS_KEEP): RelationData +
// RelationJoin, src/libfm/src/relation.h:32-60
struct BlockRows {
  Slot      rows;                  // the block's own rows (ids local to the block); owns the block's X^T segments too
  uint32_t* map = nullptr;         // [main rows] -> block row (RelationJoin::data_row_to_relation_row)
  uint32_t  attr_offset = 0;       // RelationData::attr_offset: global id of the block's attribute 0
  uint32_t* brow_ptr = nullptr;    // [block rows + 1] / brow_list [main rows]: the main rows that map to a block row
  uint32_t* brow_list = nullptr;
  float*    pbuf = nullptr;        // [block rows][KP + 1] partial sums of the block rows (predict)
};
void free_block(BlockRows* b);
int check_block_rows(fmx_handle h, const void* entries, const uint64_t* row_ptr, uint32_t n_rows, uint64_t nnz,
                     const fmx_relation* relations, uint32_t n_relations);                          // fmx_core.hip
int attach_kept_blocks(fmx_handle h, int slot, uint32_t n_rows, const fmx_relation* relations, uint32_t n_relations);   // fmx_core.hip

struct AlsBlock {                  // ALS / MCMC state of one kept block (fm_learn_mcmc.h:50-58 relation_cache, restated)
  uint32_t* level_list = nullptr;
  std::vector<uint32_t> level_ptr;
  double*   cache = nullptr;       // [7][block rows]: we, weq, wc, wc2, qb, dy, qb0   (struct of arrays)
  double*   qb_all = nullptr;      // [KP][block rows]: the block rows' factor sums of the latest re-prediction
  double*   cpart = nullptr;       // [block rows]: lin - 0.5 * sum of squares of the block rows
  double*   delta = nullptr;       // feature shards: [4][block rows] what the draws of the current level change in we, weq, qb, dy
  int       lanes = 8;
};

struct AlsState {
  int       slot = -1;
  EQ*       e = nullptr;          // [N] {residual, current factor's q}
  double*   q = nullptr;          // [KP][N]
  uint8_t*  seen = nullptr;       // [n_local] feature has a training column
  uint32_t* level_list = nullptr; // segments ordered by level
  uint4*    ldesc = nullptr;      // the same list as {feature, first entry, end entry, segment} records (k_als_ldesc)
  std::vector<uint32_t> level_ptr;
  uint64_t  iter = 0;
  std::vector<AlsBlock> blk;      // kept blocks of the train slot
  EQ*       delta = nullptr;      // feature shards: [N] what the draws of the current (family, level) step change in {e, q}
  double*   epart = nullptr;      // feature shards: [N] partial y-hat of the re-prediction
  float*    vt = nullptr;         // [num_factor][vt_stride] factor-major shadow of the seen features' factors, level order
  size_t    vt_stride = 0;
  // split step (large levels of an unsharded session): the entries of every level in ROW order + the draws' {old, new} pairs
  uint32_t* r_row = nullptr; uint32_t* r_pos = nullptr; float* r_x = nullptr;   // [nnz], level after level
  float2*   dth = nullptr;        // [largest level]
  std::vector<uint32_t> lev_ent;  // [n_levels + 1] entry range of each level in r_*
  std::vector<uint8_t> lev_dense; // [n_levels] the level's entries are the rows 0 .. N-1 in order (k_als_rows_dense); 2: ... and every value is 1
  uint32_t* t_row = nullptr;      // [nnz] the rows of X^T's entries alone: what a level of unit values streams instead of {row, value}
  uint32_t  split_min = 0;        // levels with at least this many entries take the split step (0: none)
  double*   prior = nullptr;      // [1 + k][2][G]: per coordinate family (row 0 = w, 1+f = v_f) lambda[G] then mu[G]
  std::vector<double> prior_host;
};

struct LagState {                 // FMX_FLAG_BIAS_LAG bookkeeping (split step): w0 lives in w0_pp[step & 1] while active
  static constexpr uint32_t RING = 8;                 // >= depth + 2
  bool       active = false;
  uint64_t   step = 0;
  uint32_t   depth = 1;           // batches the multipliers' bias lags behind (fmx_sgd_opts::bias_lag)
  hipEvent_t ev_rest = nullptr, ev_scan[RING] = {};
  hipStream_t in_stream = nullptr;  // small batches: the recurrences ride in the update's launches on THIS stream (not the side stream): lag_flush drains it
};

struct SgdaState { float* gw = nullptr; float* gv = nullptr; double* reg = nullptr; double* dreg = nullptr;   // dreg: [workgroups][G][1 + KP] partial lambda changes
                   size_t dreg_cap = 0; };
// an open fmx_adapt_* session (fmx_sgd.hip): the per-coordinate accumulators, n_v with V's row stride
// (init_acc: the fp32 start value of every accumulator, kept for the checkpoint's sparse criterion and its load)
struct AdaptState { float* nw = nullptr; float* nv = nullptr; float eta = 0.f; float init_acc = 0.f; };
// an open fmx_ftrl_* session (fmx_sgd.hip): z and n per coordinate, the row tables with V's row stride, and the rule's constants
struct FtrlState { float* zw = nullptr; float* zv = nullptr; float* nw = nullptr; float* nv = nullptr;
                   float inv_alpha = 0.f, beta = 0.f, l1_w = 0.f, l1_v = 0.f, l2_w = 0.f, l2_v = 0.f, init_acc = 0.f;
                   // the start denominator D0 of a coordinate with this l2, as fmx_ftrl_begin computes it (base + l2, all fp32)
                   float start_D(float l2) const { const float base = (beta + sqrtf(init_acc)) * inv_alpha; return base + l2; } };
// the serving snapshot (fmx_compact_*, fmx_compact.hip): a frozen copy of w0 and, by format,
//   FMX_COMPACT_BF16  w (fp32, stride 1) and V as bf16 rows of tb.rs elements
//   FMX_COMPACT_INT8  B: one block of P bytes per feature with its scale, its w and its int8 codes (V and w stay null)
// dir != nullptr: a pruned snapshot (fmx_compact_begin_pruned) -- the tables hold `kept` rows in slot order and dir, the rank directory
// of ceil(n_local / 32) pairs (fmx_compact_kernels.h dir_lookup), maps a feature id to its slot
// nonfinite .. dropped_unseen: the figures of fmx_compact_info / fmx_compact_prune_info as they were when the snapshot was taken (or as the
// file it was loaded from holds them), for fmx_compact_save's header
struct CompactState { uint16_t* V = nullptr; float* w = nullptr; double* w0 = nullptr; uint8_t* B = nullptr; uint32_t P = 0; uint32_t format = 0;
                      uint2* dir = nullptr; uint64_t kept = 0;
                      uint64_t nonfinite = 0; double max_abs_err = 0.0, sum_sq_err = 0.0; uint64_t dropped_dead = 0, dropped_unseen = 0; };

struct fmx_context_s {
  fmx_config cfg;
  AlsState   als;
  SgdaState  sgda;
  AdaptState adapt;
  FtrlState  ftrl;
  CompactState compact;
  LagState   lag;
  int        KP = 1;
  double     setup_acc = 0.0;    // host seconds of one-time slot preparation since the epoch entry point last cleared it
  uint32_t*  grp = nullptr;      // [n_local] attribute -> group (fmx_set_groups); nullptr = one group
  uint32_t   num_groups = 1;
  uint64_t   n_local = 0;
  int        device = 0;
  hipStream_t stream = nullptr;
  Tab        tb = {nullptr, nullptr, 0, 0};   // V rows (+ co-located w), see fmx_kernels.h
  float*     w_sep = nullptr;    // the w[] array
  bool       serve_only = false; // fmx_serve_open (fmx_snap.hip): the handle holds a snapshot and NO model -- tb.V, tb.w and w_sep are null and
                                 // every entry point that is not on the allow-list of DESIGN.md section 27 refuses it first (serve_refuse)
  Placed     placed;             // fmx_place_plan.h: the report, and for a big model the ARENA both tables are parts of (nothing to hipFree): one
                                 // virtual range of 1 GiB physical chunks taken alternately from two memory classes
  double*    w0 = nullptr;       // device scalar
  double*    w0_pp = nullptr;    // 8 doubles: ring of bias copies for the overlapped recurrence (hogwild, fused, bias lag)
  hipStream_t stream2 = nullptr; // side stream of the hogwild bias scan
  // device-side hand-off of the bias between the two streams (one-pass batch rule at large batches; fmx_kernels.h)
  bool        handoff = true;               // FMX_HANDOFF=0 in the environment of fmx_create: events instead
  double*     w0_slots = nullptr;           // [w0_slots_cap] bias after every batch of the running epoch
  uint64_t    w0_slots_cap = 0;
  unsigned long long* handoff_ctr = nullptr;   // device: batches whose k_fused has completed (monotonic over the handle's life)
  unsigned long long  handoff_seq = 0;         // host: value of the counter before the running epoch
  uint32_t*   handoff_err = nullptr;        // device: a wait ran into its bound
  uint32_t    handoff_err_host = 0;
  // the parallel-in-time bias recurrence (k_scan_pit): arrival counters of its grid-wide exchanges + the workgroups' slots
  bool        scan_pit = true;              // FMX_SCAN=serial in the environment of fmx_create: the one-wavefront chain (k_scan1 / k_scan) instead
  unsigned long long* pit_ctr = nullptr;    // [PIT_MAX_IT + 1], zeroed on the launch's stream before every launch
  double*     pit_slots = nullptr;          // [2][PIT_MAX_WG][4]
  bool        pit_used = false;             // a launch since the error word was last read
  uint32_t    run_status = 0;               // FMX_STAT_SCAN_* / _EVENT_SYNC / _HANDOFF_TIMEOUT of the running epoch (launch_scan, sgd_epoch_fused)
  int         concurrent = -1;              // do the handle's two streams run concurrently? -1: not probed yet (streams_concurrent)
  unsigned*   probe_flags = nullptr;        // device: 4 words of k_concurrency_probe
  uint32_t    pit_spins = 0;                // bound of a grid-wide exchange's wait (fmx_create: HANDOFF_SPINS, or FMX_DEBUG_PIT_SPINS from the environment)
  int         pit_occ = -1;                 // workgroups of k_scan_pit the device holds at once (occupancy x CUs); -1: not asked yet
  double*     pit_tmp = nullptr;            // bias between the pieces of a batch longer than PIT_MAX_ROWS
  uint64_t    w_version = 1;                // bumped by every entry point that may change a linear weight (a slot's side stream is valid for ONE value)
  int        num_cu = 256;
  double*    acc = nullptr;      // 4 doubles of reduction scratch
  Slot       slots[FMX_MAX_SLOTS];
  float*     partial = nullptr;  // [cap][KP] + [cap]
  float*     mult = nullptr;     // [cap]
  float*     rest = nullptr;     // [cap_rest]
  size_t     cap = 0, cap_rest = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> ev_pool;
  std::vector<hipEvent_t> ev_sync;   // untimed events ordering the two hogwild streams
  std::string err;
  hipDeviceProp_t prop;
  // several GPUs (fmx_comm.hip)
  void*       comm = nullptr;         // ncclComm_t of a one-process-per-GPU job (fmx_comm_init_rank)
  struct fmx_group_s* group = nullptr;
  bool        owns_group = false;     // the 1-handle group fmx_sgd_epoch builds around `comm`
  float*      xbuf[2] = {nullptr, nullptr};   // exchange buffers [batch][KP + 1]
  size_t      xcap = 0;
  hipStream_t stream_comm = nullptr;  // the all-reduce runs here, ordered by ev_x: [which] partial ready, [2 + which] sum ready
  hipEvent_t  ev_x[4] = {};
  std::unordered_map<const void*, int> occ_cache;   // resident_grid: occupancy per kernel on THIS handle's device
  std::unordered_set<const void*> lds_raised;       // kernels whose dynamic-LDS limit was raised on THIS handle's device
  // FMX_SGD_SEQUENTIAL, a conflict-free run as ONE launch (k_run_fused): workgroups of the instance the device holds at once; off after a time-out
  std::unordered_map<const void*, int> run_one_occ;
  bool run_one = true, run_one_used = false;
  // FMX_SGD_SEQUENTIAL's forms, from the environment of fmx_create (default: all on; fmx_sgd_epoch picks by the slot's rows)
  bool seq_rows = true, seq_wg = true, seq_runs_fused = true, seq_runs_one = true;
  uint32_t topk_splits = 0;                          // FMX_TOPK_SPLITS at fmx_create: candidate splits of fmx_topk (0: the library's choice)
  unsigned long long* run_slots = nullptr;          // [RUN_ONE_MAX] {tag, rest_e} of a one-launch run's examples
  // small batches of the minibatch rule as ONE launch per batch (k_small_one, fmx_small_kernels.h): {tag, mult_e} and {tag, rest_e} slots; off after a time-out
  unsigned long long* small_slots = nullptr;        // [3 * SMALL_ONE_MAX]: multipliers, rest_e of even / odd batches
  bool small_one = true, small_one_used = false;
  bool ids = true;                                  // FMX_IDS=0 in the environment of fmx_create: k_fused keeps reading {id, value} entries (Slot::ids is never built)
  bool wtrain = true;                               // FMX_WTRAIN=0 in the environment of fmx_create: every linear weight is gathered (Slot::wtrain is never built)
};

// ---- helpers shared between the translation units -------------------------------------------------------------
int fail(fmx_handle h, int code, const char* fmt, ...);                 // fmx_core.hip
// fmx_create behind its argument checks, for fmx_serve_open too (fmx_core.hip): serve_only = everything but the parameter tables
int create_handle(const fmx_config* cfg, fmx_handle* out, bool serve_only);
// what every entry point that reads or writes the model says to a serve-only handle, as its first statement after the NULL check:
// FMX_E_STATE, nothing launched, the handle usable afterwards.  FMX_OK on an ordinary handle.
inline int serve_refuse(fmx_handle h, const char* who) {
  return h->serve_only ? fail(h, FMX_E_STATE, "%s: a serve-only handle holds no model", who) : FMX_OK;
}
Hyper make_hyper(const fmx_config& c);
Shard make_shard(const fmx_config& c);
constexpr int FMX_GRID_OVER_SGD = 1 << 16;   // effectively uncapped
constexpr int FMX_GRID_OVER_ALS = 2;
#ifndef FMX_GRID_OVER_DEFAULT
#define FMX_GRID_OVER_DEFAULT FMX_GRID_OVER_SGD      // fmx_als.hip defines it as FMX_GRID_OVER_ALS before including this header
#endif
uint32_t resident_grid(fmx_handle h, const void* kernel, uint64_t n_waves_wanted, int over_default = FMX_GRID_OVER_DEFAULT);
int ensure_scratch(fmx_handle h, size_t batch_cap, size_t rest_cap);
int check_slot(fmx_handle h, int slot, bool need_target);
int slot_in_session(fmx_handle h, int slot, const char* what);
void free_segments(Slot& s);
void free_slot(Slot& s);
// fmx_core.hip, the read side.  snap names the rows' source everywhere: nullptr = the model (h->tb, h->w0, the slot's side stream where
// it is current), else the bf16 snapshot (its tables, its w0).
int launch_rest(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n, float* rest, hipStream_t st, const CompactState* snap = nullptr);
// the scores of all n_rows >= 1 rows of a slot, on h->stream and in h->rest: ensure_scratch, h->ev0 (where the call's device work begins),
// the rest pass, and *score = rest (y-hat minus the bias: the reductions add it, add_w0 = 1) or, with want_yhat, the finished y-hat
// (the source's own bias; on a feature shard rank 0 alone adds it)
int slot_scores(fmx_handle h, const Slot& s, const CompactState* snap, bool want_yhat, const float** score);
// fmx_predict / fmx_evaluate after their checks, for the snapshot's entry points too: slot_scores, then the y-hat to the host /
// k_eval with the source's bias to rmse, mae, accuracy and device_seconds (n_rows >= 1; predict_out takes an empty slot too)
int predict_out(fmx_handle h, const Slot& s, const CompactState* snap, double* out);
int evaluate_out(fmx_handle h, const Slot& s, const CompactState* snap, fmx_eval* out);
inline RowsBf16 compact_rows(fmx_handle h, const CompactState& c) { return RowsBf16{CTab{c.V, c.w, h->tb.rs}}; }
inline RowsI8 compact_rows8(const CompactState& c) { return RowsI8{c.B, c.P}; }
inline RowsBf16P compact_rows_p(fmx_handle h, const CompactState& c) { return RowsBf16P{compact_rows(h, c), c.dir}; }
inline RowsI8P compact_rows8_p(const CompactState& c) { return RowsI8P{compact_rows8(c), c.dir}; }
int ensure_segments(fmx_handle h, Slot& s, uint32_t B);                 // fmx_sgd.hip
int ensure_coll_mass(fmx_handle h, Slot& s);                             // fmx_core.hip
int ensure_wside(fmx_handle h, Slot& s);                                 // fmx_core.hip
int ensure_ids(fmx_handle h, Slot& s);                                   // fmx_core.hip
int ensure_wtrain(fmx_handle h, Slot& s, uint32_t row_cap);              // fmx_core.hip (row_cap: longest row of k_fused's register path)
inline void touch_w(fmx_handle h) { if (h) h->w_version++; }
void resolve_batch(const fmx_config& cfg, double coll_mass, uint32_t requested, uint32_t dflt, double curv_scale, fmx_batch_info* out);
constexpr uint32_t FMX_DEFAULT_BATCH = 262144u;                          // fmx_sgd_opts::batch = 0, before the stability cut
// batches of this many rows and more give the bias recurrence a stream of its own; below, a batch is microseconds of work and the recurrence
// rides in the launch stream (k_apply_seg_scan, k_small_one): sgd_epoch_fused, the split step's update (step_plan), the group driver's exchange
constexpr uint32_t FMX_SIDE_STREAM_BATCH = 32768u;
// a batch of the bias-lag schedule small enough for the in-stream forms (+ short rows: step_plan; + the group driver's own terms: its exchange)
inline bool sgd_in_stream_batch(uint32_t batch, uint32_t flags) { return batch != 0 && batch < FMX_SIDE_STREAM_BATCH && (flags & FMX_FLAG_BIAS_LAG); }
int sgd_resolve_batch(fmx_handle h, Slot& s, const fmx_sgd_opts* opts, fmx_batch_info* bi);   // fmx_sgd.hip: + the shards' shares
int sgd_partial_rows(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n_rows, float* S, float* c, hipStream_t st,
                     const CompactState* snap = nullptr);                // fmx_sgd.hip (snap: as launch_rest)
constexpr size_t PREP_RAW_FLOATS = size_t(1) << 24;                      // prep_rows: raw partial sums of one piece of rows (64 MiB)
// fmx_topk.hip: the [rows][KM] factor sums and scalars of section 11 (snap: as launch_rest)
int prep_rows(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n, int k0, float* raw, size_t raw_rows, int KM,
              float* S_out, float* scal, hipStream_t st, const CompactState* snap = nullptr);
// fmx_topk.hip: fmx_topk after the handle check, for fmx_compact_topk too (`who` names the entry point in messages; snap as above)
int topk_impl(fmx_handle h, const char* who, int query_slot, int cand_slot, const fmx_topk_opts* opts, uint32_t* idx_out, double* score_out,
              fmx_topk_stats* stats, const CompactState* snap);
void compact_free(fmx_handle h);                                         // fmx_compact.hip
void compact_release(CompactState& c);                                   // fmx_compact.hip: frees a snapshot's tables, leaves an empty state
int lag_flush(fmx_handle h);                                             // fmx_sgd.hip
// fmx_eval.hip: the argument checks, the empty result and the reduction of fmx_evaluate_ex, shared with fmx_group_evaluate_ex (fmx_comm.hip)
int eval_ex_check_opts(fmx_handle h, const char* who, const fmx_eval_opts* opts, uint32_t* link);
int eval_ex_check_slot(fmx_handle h, const char* who, int slot);
void eval_ex_empty(fmx_eval_ex* out);
int eval_ex_scores(fmx_handle h, const Slot& s, const float* score, int add_w0, uint32_t link, fmx_eval_ex* out);
// ... its rank pipeline (sort, two scans, rank sum) over keys of any width and the finish of an fmx_eval_ex from reduced sums and
// counts, shared with fmx_post_evaluate_ex (fmx_post.hip); the sort and the two scans alone, shared with evalq_scores (fmx_evalq.hip)
struct EvalScratch;
int rank_sort_scan(fmx_handle h, EvalScratch& sc, unsigned long long* keys, uint32_t n, int key_bits, size_t b_more,
                   const unsigned long long** sorted);
int eval_ex_rank(fmx_handle h, unsigned long long* keys, uint32_t n, int key_bits, unsigned long long* d_num2, uint64_t* num2,
                 double* rank_seconds);
int eval_ex_finish(fmx_handle h, uint32_t n, const double* d, uint64_t pos, uint64_t nan_rows, uint64_t correct,
                   unsigned long long* keys, int key_bits, unsigned long long* d_num2, fmx_eval_ex* out);
// fmx_evalq.hip: the checks, the empty result and the whole reduction of fmx_evaluate_by_query (pooled metrics through eval_ex_scores,
// then the by-query pipeline over the same scores), shared with fmx_group_evaluate_by_query (fmx_comm.hip)
int set_row_queries_impl(fmx_handle h, const char* who, int slot, const uint32_t* qid, uint32_t n_queries);
// fmx_weighted.hip: what every trainer without a weighted form says to a slot that has weights (FMX_E_UNSUPPORTED, before any launch)
int refuse_weighted(fmx_handle h, int slot, const char* who);
int evalq_check_slot(fmx_handle h, const char* who, int slot);
void evalq_empty(fmx_eval_query* out, uint32_t n_queries);
void evalq_zero_per_query(uint32_t n_queries, uint64_t* num2_q, uint32_t* pos_q, uint32_t* neg_q);
int evalq_scores(fmx_handle h, const Slot& s, const float* score, int add_w0, uint32_t link, fmx_eval_query* out,
                 uint64_t* num2_q, uint32_t* pos_q, uint32_t* neg_q);
// ... the same with the caller's scratch left alive (the sorted keys, the three scans, the per-query counts), for rankq_scores
int evalq_scores_keep(fmx_handle h, const Slot& s, const float* score, int add_w0, uint32_t link, fmx_eval_query* out,
                      uint64_t* num2_q, uint32_t* pos_q, uint32_t* neg_q, EvalScratch& sc, const unsigned long long** sorted);
// fmx_rankq.hip: the checks, the empty result and the whole reduction of fmx_evaluate_rank (evalq_scores_keep, then the top-K
// reduction over the same sorted keys), shared with fmx_group_evaluate_rank (fmx_comm.hip)
int rankq_check_opts(fmx_handle h, const char* who, const fmx_rank_opts* opts, uint32_t* link);
void rankq_empty(fmx_eval_rank* out, const fmx_rank_opts* opts, uint32_t n_queries, double* dcg_q, double* hits_q);
int rankq_scores(fmx_handle h, const Slot& s, const float* score, int add_w0, uint32_t link, const fmx_rank_opts* opts,
                 fmx_eval_rank* out, double* dcg_q, double* hits_q);
// fmx_post.hip: the posterior accumulator of a slot (include/fmx.h "fmx_post_*").  The *_impl functions are the entry points after
// the handle-kind check, for the first shard of a group too (fmx_comm.hip); post_accum_scores takes scores that are on h's device.
struct PostAcc {
  double*  sum_all = nullptr;      // [n_rows] pred_sum_all
  double*  sum_late = nullptr;     // [n_rows] pred_sum_all_but5
  float*   last = nullptr;         // [n_rows] the last draw's raw y-hat
  uint32_t burn_in = 5, eval_rows = 0;
  uint64_t draws = 0, late_draws = 0;
};
void free_post(Slot& s);
int post_check(fmx_handle h, const char* who, int slot, bool need_begin);
int post_begin_impl(fmx_handle h, const char* who, int slot, const fmx_post_opts* opts);
int post_accum_scores(fmx_handle h, Slot& s, const float* score, int add_w0, fmx_post_stats* out);
int post_evaluate_impl(fmx_handle h, const char* who, int slot, uint32_t which, fmx_eval_ex* out);
int post_get_impl(fmx_handle h, const char* who, int slot, uint32_t which, double* out, uint64_t* draws);
int post_end_impl(fmx_handle h, const char* who, int slot);
int scan_error_check(fmx_handle h);                                      // fmx_sgd.hip: the device's error word after k_scan_pit launches (streams drained)
uint32_t multi_group_size(const Slot& s, int KP);                        // fmx_sgd.hip: examples per wavefront of the short-row kernels (0: rows are long)
bool streams_concurrent(fmx_handle h);                                   // fmx_sgd.hip: probed once per handle
void sgda_free(fmx_handle h);                                            // fmx_sgd.hip
// which owner a pair epoch ends in (fmx_pair.hip, fmx_pairneg.hip; launch_pair_owner, fmx_pair_rule_kernels.h): the plain batch rule,
// or the rule of the open fmx_adapt / fmx_ftrl session on the session's own tables
enum PairRule { PAIR_PLAIN = 0, PAIR_ADAGRAD = 1, PAIR_FTRL = 2 };
// fmx_pair.hip, what the rule epochs refuse beyond their plain counterparts: the schedules without a rule form (before the plain
// checks: their own message), then the session (after them)
int pair_rule_check_mode(fmx_handle h, PairRule r, int mode, const char* what);
int pair_rule_check_session(fmx_handle h, PairRule r, const char* what);
void adapt_free(fmx_handle h);                                           // fmx_sgd.hip
void ftrl_free(fmx_handle h);                                            // fmx_sgd.hip
// fmx_sgd.hip, shared by fmx_adapt_begin / fmx_ftrl_begin and fmx_checkpoint_load (fmx_ckpt.hip): the session's tables (allocated
// where they are not there yet; on failure the session is closed) and its start state from the constants ALREADY in h->adapt /
// h->ftrl -- every accumulator = init_acc, and for FTRL z derived from the current parameters (k_ftrl_init).  Launches on h->stream;
// the caller synchronises.
int adapt_tables(fmx_handle h, const char* who);
int adapt_start_state(fmx_handle h);
int ftrl_tables(fmx_handle h, const char* who);
int ftrl_start_state(fmx_handle h);
// fmx_sgd.hip, for the group forms fmx_group_adapt_* / fmx_group_ftrl_* / fmx_group_param_sparsity (fmx_comm.hip).  The *_impl functions
// are the per-handle entry points with in_group = true: the call comes from the group the handle is a member of, so the refusal of
// feature shards and group members is left out and everything else -- codes, messages, work -- is the entry point's own.  *_begin_check
// is every refusal of a begin (no device work), *_begin_open the tables and the start state: a group checks all members before it opens any.
int adapt_begin_check(fmx_handle h, const fmx_adapt_opts* opts, bool in_group, float* init_acc_out);
int adapt_begin_open(fmx_handle h, const fmx_adapt_opts* opts, float init_acc);
int adapt_epoch_impl(fmx_handle h, bool in_group, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats);
int adapt_state_rows_impl(fmx_handle h, bool in_group, const uint32_t* ids, uint32_t count, double* nw_out, double* nv_out);
int adapt_end_impl(fmx_handle h, bool in_group);
int ftrl_begin_check(fmx_handle h, const fmx_ftrl_opts* opts, bool in_group, FtrlState* out);
int ftrl_begin_open(fmx_handle h, const FtrlState& constants);
int ftrl_epoch_impl(fmx_handle h, bool in_group, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats);
int ftrl_state_rows_impl(fmx_handle h, bool in_group, const uint32_t* ids, uint32_t count, double* zw, double* zv, double* nw, double* nv);
int ftrl_end_impl(fmx_handle h, bool in_group);
int param_sparsity_impl(fmx_handle h, bool in_group, fmx_sparsity* out);
// one shard's share of a stateful epoch over feature shards: what stateful_epoch does in front of its loop, and steps 3 - 6 of a batch
// from the exchanged sums (rest_e, the bias recurrence, the shard's segments, the owner kernel of `rule`) on the shard's own stream
enum StatefulRule { STATEFUL_ADAGRAD = 1, STATEFUL_FTRL = 2 };
int stateful_shard_prepare(fmx_handle h, int slot, uint32_t B);
int stateful_shard_step(fmx_handle h, int slot, StatefulRule rule, uint64_t row0, uint32_t nb, uint32_t B, uint32_t chunk, const float* d_sum);
void als_free(fmx_handle h);                                             // fmx_als.hip
enum { GROUP_SINGLE = 0, GROUP_LOOPBACK = 1, GROUP_RCCL = 2 };
struct fmx_group_s {                      // fmx_comm.hip
  std::vector<fmx_handle> hs;
  int kind = GROUP_SINGLE;
  std::vector<void*> comms;               // GROUP_RCCL: one ncclComm_t per handle
  bool owns_comms = false;                // created by fmx_group_create (not borrowed from fmx_comm_init_rank)
  std::vector<hipEvent_t> ev_part;        // loopback: the buffer of shard i is ready
  hipEvent_t ev_sum = nullptr;            // loopback: the sum is ready
  std::string err;
};
int group_allreduce_f64(fmx_group_s* g, const std::vector<double*>& bufs, size_t count);   // fmx_comm.hip: in place, on the shards' streams
void comm_free(fmx_handle h);                                            // fmx_comm.hip: communicator, group membership, exchange buffers
int comm_sgd_epoch(fmx_handle h, int slot, const fmx_sgd_opts* opts, fmx_epoch_stats* stats);   // fmx_comm.hip
int comm_sum_double(fmx_handle h, double* v);                            // fmx_comm.hip

// Device allocations of the library go through fmx_dev_alloc / fmx_dev_free (fmx_mem.hip), never through hipMalloc directly:
//   * one classified arena per device outlives its handle (fmx_mem.hip, "arena cache") and can hold tens of GB that nothing uses; an
//     allocation that runs out of memory gives that cache back and tries once more (round-4 advisor);
//   * allocations of 768 MiB and more are built from <= 1 GiB physical chunks through the virtual-memory API (hipMemCreate + hipMemMap):
//     once a process has taken and returned a pool of chunks (what the table placement of fmx_create does), a plain hipMalloc of more
//     than 1 GiB takes 0.5 - 1.6 SECONDS on this part (scripts/ubench/alloc_cost.hip, profiles/r06_alloc_cost.txt: 4 GiB 1566 ms, through
//     the virtual-memory API 0.05 ms) -- that was 96 % of the 1.3 - 2.5 s of one-time slot preparation the round-5 verdict found.
// fmx_dev_free takes either kind (and nullptr).
void arena_cache_drop(int device);                                       // fmx_mem.hip
hipError_t fmx_dev_alloc_bytes(void** p, size_t bytes);                  // fmx_mem.hip
hipError_t fmx_dev_free(void* p);                                        // fmx_mem.hip
void mark_device_used(int dev);                                          // fmx_mem.hip: fmx_create has opened a handle on it
int place_tables(fmx_handle h);                                          // fmx_mem.hip: h->tb.V, h->w_sep and the placement report
void free_tables(fmx_handle h);                                          // fmx_mem.hip
template <class T> inline hipError_t fmx_dev_alloc(T** p, size_t bytes) { return fmx_dev_alloc_bytes(reinterpret_cast<void**>(p), bytes); }
// one plain allocation of any size, never a chunked range (freed by fmx_dev_free like the others).  For memory that is taken again right
// after memory of the same size went back, as a serving snapshot that replaces another is: see fmx_compact_begin
hipError_t fmx_dev_alloc_plain_bytes(void** p, size_t bytes);            // fmx_mem.hip
template <class T> inline hipError_t fmx_dev_alloc_plain(T** p, size_t bytes) { return fmx_dev_alloc_plain_bytes(reinterpret_cast<void**>(p), bytes); }

// everything a call of the exact metrics (fmx_eval.hip, fmx_evalq.hip) takes from the device, freed on every path out of the call:
// each function allocates the members it uses and the others stay null
struct EvalScratch {
  void* part = nullptr;                     // block partials + results
  unsigned long long* keys0 = nullptr; unsigned long long* keys1 = nullptr;   // the keys and the sort's second buffer
  uint32_t* negbefore = nullptr; uint32_t* runhead = nullptr; uint32_t* qhead = nullptr;
  void* tmp = nullptr; size_t tmp_bytes = 0;   // the larger of the sort's and the scans' temporaries
  void* perq = nullptr;                     // [n_queries] num2 (8 bytes), then pos, neg (4 + 4)
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~EvalScratch() {
    fmx_dev_free(part); fmx_dev_free(keys0); fmx_dev_free(keys1); fmx_dev_free(negbefore); fmx_dev_free(runhead); fmx_dev_free(qhead);
    fmx_dev_free(tmp); fmx_dev_free(perq);
    for (auto e : ev) if (e) hipEventDestroy(e);
  }
};

#define HIPCHK(h, expr)                                                                        \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess)                                                                       \
      return fail((h), FMX_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

// The gather of rows by feature id (fmx_get_param_rows, the optimisers' state rows, fmx_compact_get_rows) from nt tables, one after the
// other: the ids go up once; launch(t, grid, d_ids, d_w, d_v) starts table t's k_fetch_rows on h->stream, and its w and v parts come back
// to outs[t] = {w_out, v_out}.  Checks nothing about the ids, returns with the stream drained, frees both device buffers on every path;
// count >= 1.
template <class Launch>
int gather_rows(fmx_handle h, const char* who, const uint32_t* ids, uint32_t count, int nt, double* const (*outs)[2], Launch launch) {
  const int k = h->cfg.num_factor;
  HIPCHK(h, hipSetDevice(h->device));
  uint32_t* d_ids = nullptr; double* d_out = nullptr;
  const size_t nout = (size_t)count * (size_t)(k + 1);
  HIPCHK(h, fmx_dev_alloc(&d_ids, (size_t)count * 4));
  hipError_t er = fmx_dev_alloc(&d_out, nout * sizeof(double));
  if (er == hipSuccess) er = hipMemcpyAsync(d_ids, ids, (size_t)count * 4, hipMemcpyHostToDevice, h->stream);
  for (int t = 0; t < nt && er == hipSuccess; t++) {
    launch(t, dim3((uint32_t)((nout + 255) / 256)), (const uint32_t*)d_ids, d_out, d_out + count);
    er = hipGetLastError();
    if (er == hipSuccess) er = hipMemcpyAsync(outs[t][0], d_out, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (er == hipSuccess && k > 0) er = hipMemcpyAsync(outs[t][1], d_out + count, (size_t)count * k * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  }
  fmx_dev_free(d_ids); fmx_dev_free(d_out);
  if (er != hipSuccess) return fail(h, FMX_E_HIP, "%s: %s", who, hipGetErrorString(er));
  return FMX_OK;
}

// wave-per-example grids: 4 waves per 256-thread block, capped so that the launch is >> 256 workgroups
// but grid-strides the rest (guide: memory-bound ops, 256 CUs x 8 blocks).
inline uint32_t wave_grid(uint64_t n_waves_wanted) {
  uint64_t blocks = (n_waves_wanted + 3) / 4;
  if (blocks < 1) blocks = 1;
  if (blocks > 256 * 8) blocks = 256 * 8;
  return (uint32_t)blocks;
}

#define FMX_LAUNCH_WAVES(kfn, waves, st, ...)                                                        \
  do { auto _k = kfn; hipLaunchKernelGGL(_k, dim3(resident_grid(h, (const void*)_k, (waves))), dim3(256), 0, st, __VA_ARGS__); } while (0)

#define KP_SWITCH(KPV, ...)                                            \
  switch (KPV) {                                                       \
    case 1:   { constexpr int KP = 1;   __VA_ARGS__; } break;          \
    case 2:   { constexpr int KP = 2;   __VA_ARGS__; } break;          \
    case 4:   { constexpr int KP = 4;   __VA_ARGS__; } break;          \
    case 8:   { constexpr int KP = 8;   __VA_ARGS__; } break;          \
    case 16:  { constexpr int KP = 16;  __VA_ARGS__; } break;          \
    case 32:  { constexpr int KP = 32;  __VA_ARGS__; } break;          \
    case 64:  { constexpr int KP = 64;  __VA_ARGS__; } break;          \
    case 128: { constexpr int KP = 128; __VA_ARGS__; } break;          \
    case 256: { constexpr int KP = 256; __VA_ARGS__; } break;          \
    case 512: { constexpr int KP = 512; __VA_ARGS__; } break;          \
    case 1024: { constexpr int KP = 1024; __VA_ARGS__; } break;        \
    default: return fail(h, FMX_E_UNSUPPORTED, "num_factor > 1024 is not supported");   \
  }

