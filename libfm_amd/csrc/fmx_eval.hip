// fmx_eval.hip -- fmx_evaluate_ex: exact, tie-aware AUC and log loss of a slot on the device.
// The scores come from launch_rest like fmx_evaluate's; the reduction is this unit's: block partials summed in a fixed order, one
// radix sort of 33-bit keys, two library scans and the rank-sum kernel (fmx_eval_kernels.h).
#include "fmx_internal.h"
#include "fmx_eval_kernels.h"

#include <limits>

namespace {

// the block partials of the call: freed on every path out of eval_ex_scores
struct EvalScratch {
  void* part = nullptr;                     // block partials + results
  unsigned long long* keys = nullptr;
  ~EvalScratch() { fmx_dev_free(part); fmx_dev_free(keys); }
};

// everything the rank pipeline takes from the device: freed on every path out of eval_ex_rank
struct RankScratch {
  unsigned long long* keys1 = nullptr;      // the sort's second buffer
  uint32_t* negbefore = nullptr; uint32_t* runhead = nullptr;
  void* tmp = nullptr;                      // the larger of the sort's and the scans' temporaries
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~RankScratch() {
    fmx_dev_free(keys1); fmx_dev_free(negbefore); fmx_dev_free(runhead); fmx_dev_free(tmp);
    for (auto e : ev) if (e) hipEventDestroy(e);
  }
};

}  // namespace

int eval_ex_check_opts(fmx_handle h, const char* who, const fmx_eval_opts* opts, uint32_t* link) {
  *link = FMX_LINK_LOGISTIC;
  if (!opts) return FMX_OK;
  if (opts->link != FMX_LINK_LOGISTIC && opts->link != FMX_LINK_PROBIT) return fail(h, FMX_E_ARG, "%s: unknown link %u", who, opts->link);
  if (opts->flags != 0) return fail(h, FMX_E_ARG, "%s: flags must be 0 (got %u)", who, opts->flags);
  *link = opts->link;
  return FMX_OK;
}

int eval_ex_check_slot(fmx_handle h, const char* who, int slot) {
  if (slot < 0 || slot >= FMX_MAX_SLOTS) return fail(h, FMX_E_ARG, "%s: slot %d out of range", who, slot);
  if (!h->slots[slot].used) return fail(h, FMX_E_STATE, "%s: slot %d holds no rows (call fmx_upload_rows first)", who, slot);
  if (!h->slots[slot].target) return fail(h, FMX_E_STATE, "%s: slot %d was uploaded without targets", who, slot);
  if (h->slots[slot].n_rows > 0x7FFFFFFFu) return fail(h, FMX_E_UNSUPPORTED, "%s: more than 2^31 - 1 rows", who);
  return FMX_OK;
}

void eval_ex_empty(fmx_eval_ex* out) {
  memset(out, 0, sizeof(*out));
  out->auc = out->logloss = std::numeric_limits<double>::quiet_NaN();
}

// The rank pipeline of the exact AUC: n keys of key_bits bits on h's device -- the label in bit 0, an order-preserving image of the
// score above it -- are sorted (one radix sort; `keys` is one of its two buffers and is overwritten), scanned twice and reduced by
// k_evalx_ranksum into *d_num2, a device word the caller has zeroed on h->stream.  Records h->ev1 after the last kernel and
// returns with the stream drained.  n >= 1.
int eval_ex_rank(fmx_handle h, unsigned long long* keys, uint32_t n, int key_bits, unsigned long long* d_num2, uint64_t* num2,
                 double* rank_seconds) {
  RankScratch sc;
  HIPCHK(h, fmx_dev_alloc(&sc.keys1, (size_t)n * 8));
  HIPCHK(h, fmx_dev_alloc(&sc.negbefore, (size_t)n * 4));
  HIPCHK(h, fmx_dev_alloc(&sc.runhead, (size_t)n * 4));
  for (auto& e : sc.ev) HIPCHK(h, hipEventCreate(&e));
  hipcub::DoubleBuffer<unsigned long long> db(keys, sc.keys1);
  typedef hipcub::TransformInputIterator<uint32_t, EvalxIsNeg, const unsigned long long*> NegIt;
  typedef hipcub::TransformInputIterator<uint32_t, EvalxHead, hipcub::CountingInputIterator<uint32_t>> HeadIt;
  size_t b_sort = 0, b_sum = 0, b_max = 0;
  HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(nullptr, b_sort, db, (int)n, 0, key_bits, h->stream));
  HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, b_sum, NegIt(keys, EvalxIsNeg()), sc.negbefore, (int)n, h->stream));
  HIPCHK(h, hipcub::DeviceScan::InclusiveScan(nullptr, b_max, HeadIt(hipcub::CountingInputIterator<uint32_t>(0), EvalxHead{keys}),
                                              sc.runhead, hipcub::Max(), (int)n, h->stream));
  size_t b_tmp = std::max(b_sort, std::max(b_sum, b_max));
  HIPCHK(h, fmx_dev_alloc(&sc.tmp, std::max<size_t>(b_tmp, 16)));
  HIPCHK(h, hipEventRecord(sc.ev[0], h->stream));
  HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(sc.tmp, b_tmp, db, (int)n, 0, key_bits, h->stream));
  const unsigned long long* ks = db.Current();
  HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(sc.tmp, b_tmp, NegIt(ks, EvalxIsNeg()), sc.negbefore, (int)n, h->stream));
  HIPCHK(h, hipcub::DeviceScan::InclusiveScan(sc.tmp, b_tmp, HeadIt(hipcub::CountingInputIterator<uint32_t>(0), EvalxHead{ks}),
                                              sc.runhead, hipcub::Max(), (int)n, h->stream));
  hipLaunchKernelGGL(k_evalx_ranksum, dim3(evalx_grid(n)), dim3(256), 0, h->stream, ks, (const uint32_t*)sc.negbefore, (const uint32_t*)sc.runhead, n, d_num2);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(sc.ev[1], h->stream));
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  unsigned long long got = 0;
  HIPCHK(h, hipMemcpyAsync(&got, d_num2, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float rms = 0;
  HIPCHK(h, hipEventElapsedTime(&rms, sc.ev[0], sc.ev[1]));
  *rank_seconds = rms * 1e-3;
  *num2 = got;
  return FMX_OK;
}

// The reduction over n = s.n_rows scores that are already on h's device, on h->stream: score[e] is `rest` (y-hat - w0, add_w0 = 1) or
// the finished y-hat (add_w0 = 0); the targets are the slot's.  The caller has recorded h->ev0 where the call's device work began
// and fills out->flags.  n >= 1.
int eval_ex_scores(fmx_handle h, const Slot& s, const float* score, int add_w0, uint32_t link, fmx_eval_ex* out) {
  const uint32_t n = s.n_rows;
  const bool cls = (h->cfg.task == FMX_TASK_CLASSIFICATION);
  const uint32_t nblk = evalx_grid(n);
  EvalScratch sc;
  // [nblk][3] doubles, [nblk][3] counts, then 3 doubles, 3 counts and the AUC numerator
  HIPCHK(h, fmx_dev_alloc(&sc.part, ((size_t)nblk * 6 + 7) * 8));
  double* dpart = (double*)sc.part;
  unsigned long long* cpart = (unsigned long long*)sc.part + (size_t)nblk * 3;
  double* dres = (double*)sc.part + (size_t)nblk * 6;
  unsigned long long* cres = (unsigned long long*)sc.part + (size_t)nblk * 6 + 3;
  if (cls) HIPCHK(h, fmx_dev_alloc(&sc.keys, (size_t)n * 8));
  hipLaunchKernelGGL(k_evalx_score, dim3(nblk), dim3(256), 0, h->stream, score, (const float*)s.target, n, make_hyper(h->cfg), add_w0,
                     (const double*)h->w0, link, dpart, cpart, sc.keys);
  hipLaunchKernelGGL(k_evalx_final, dim3(1), dim3(64), 0, h->stream, (const double*)dpart, (const unsigned long long*)cpart, nblk, dres, cres);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemsetAsync(cres + 3, 0, 8, h->stream));
  struct { double d[3]; unsigned long long c[4]; } res;
  HIPCHK(h, hipMemcpyAsync(&res, dres, sizeof(res), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));                        // the counts decide whether anything is sorted
  const uint64_t pos = res.c[0], nan_rows = res.c[1], correct = res.c[2];
  const double nan = std::numeric_limits<double>::quiet_NaN();
  out->rows = n;
  out->auc = out->logloss = nan;
  if (!cls) {
    out->rmse = std::sqrt(res.d[0] / n);                             // fm_learn.h:152
    out->mae = res.d[1] / n;                                         // fm_learn.h:148
  } else {
    out->pos = pos; out->neg = n - pos; out->nan_rows = nan_rows; out->correct = correct;
    out->accuracy = (double)correct / n;                             // fm_learn.h:129
    if (nan_rows == 0) out->logloss = res.d[2] / n;
  }
  if (cls && nan_rows == 0 && out->pos != 0 && out->neg != 0) {      // (one class only: the numerator is 0 and the AUC NaN without a sort)
    const int rc = eval_ex_rank(h, sc.keys, n, EVALX_KEY_BITS, cres + 3, &out->auc_num2, &out->rank_seconds);
    if (rc) return rc;
    out->auc = (double)out->auc_num2 / (2.0 * (double)out->pos * (double)out->neg);
  } else {
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev1));
  }
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  out->device_seconds = ms * 1e-3;
  return FMX_OK;
}

extern "C" {

int fmx_evaluate_ex(fmx_handle h, int slot, const fmx_eval_opts* opts, fmx_eval_ex* out) {
  static const char who[] = "fmx_evaluate_ex";
  if (!h) return FMX_E_ARG;
  if (!out) return fail(h, FMX_E_ARG, "%s: out is NULL", who);
  uint32_t link;
  int rc = eval_ex_check_opts(h, who, opts, &link);
  if (rc) return rc;
  rc = eval_ex_check_slot(h, who, slot);
  if (rc) return rc;
  if (h->cfg.shard_world > 1) return fail(h, FMX_E_UNSUPPORTED, "%s on a feature shard: use fmx_group_evaluate_ex", who);
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  eval_ex_empty(out);
  if (s.n_rows == 0) return FMX_OK;
  rc = ensure_scratch(h, 0, (size_t)s.n_rows * 2);
  if (rc) return rc;
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  rc = launch_rest(h, s, 0, s.n_rows, h->rest, h->stream);
  if (rc) return rc;
  if (s.wside && s.wside_version == h->w_version && s.blocks.empty()) out->flags |= FMX_EVAL_WSIDE;
  return eval_ex_scores(h, s, h->rest, 1, link, out);
}

}  // extern "C"
