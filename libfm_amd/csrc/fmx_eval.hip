// fmx_eval.hip -- fmx_evaluate_ex: exact, tie-aware AUC and log loss of a slot on the device.
// The scores come from slot_scores like fmx_evaluate's; the reduction is this unit's: block partials summed in a fixed order, one
// radix sort of 33-bit keys, two library scans and the rank-sum kernel (fmx_eval_kernels.h).  Three pieces serve other units too:
// rank_sort_scan (the sort and the two scans: fmx_evalq.hip), eval_ex_rank and eval_ex_finish (fmx_post.hip).
#include "fmx_internal.h"
#include "fmx_eval_kernels.h"

#include <limits>

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

// The head of every rank pipeline: n keys of key_bits bits on h's device -- the label in bit 0, an order-preserving image of the
// score above it, and whatever the caller puts above that -- are sorted (one radix sort between `keys` and sc.keys1; both are
// overwritten) and scanned twice over the sorted order: sc.negbefore (negatives before a position) and sc.runhead (where the run of
// equal keys begins).  Allocates keys1, both outputs, the two events and sc.tmp, the larger of its own temporaries and b_more bytes
// (a scan of the caller's), and records sc.ev[0] before the sort.  *sorted: the buffer that holds the sorted keys.
int rank_sort_scan(fmx_handle h, EvalScratch& sc, unsigned long long* keys, uint32_t n, int key_bits, size_t b_more,
                   const unsigned long long** sorted) {
  HIPCHK(h, fmx_dev_alloc(&sc.keys1, (size_t)n * 8));
  HIPCHK(h, fmx_dev_alloc(&sc.negbefore, (size_t)n * 4));
  HIPCHK(h, fmx_dev_alloc(&sc.runhead, (size_t)n * 4));
  for (auto& e : sc.ev) HIPCHK(h, hipEventCreate(&e));
  hipcub::DoubleBuffer<unsigned long long> db(keys, sc.keys1);
  typedef hipcub::TransformInputIterator<uint32_t, EvalxIsNeg, const unsigned long long*> NegIt;
  typedef hipcub::TransformInputIterator<uint32_t, EvalxHead, hipcub::CountingInputIterator<uint32_t>> HeadIt;
  const hipcub::CountingInputIterator<uint32_t> pos0(0);
  size_t b_sort = 0, b_sum = 0, b_max = 0;
  HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(nullptr, b_sort, db, (int)n, 0, key_bits, h->stream));
  HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, b_sum, NegIt(keys, EvalxIsNeg()), sc.negbefore, (int)n, h->stream));
  HIPCHK(h, hipcub::DeviceScan::InclusiveScan(nullptr, b_max, HeadIt(pos0, EvalxHead{keys}), sc.runhead, hipcub::Max(), (int)n, h->stream));
  sc.tmp_bytes = std::max(std::max(b_sort, b_sum), std::max(b_max, b_more));
  HIPCHK(h, fmx_dev_alloc(&sc.tmp, std::max<size_t>(sc.tmp_bytes, 16)));
  HIPCHK(h, hipEventRecord(sc.ev[0], h->stream));
  HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(sc.tmp, sc.tmp_bytes, db, (int)n, 0, key_bits, h->stream));
  const unsigned long long* ks = db.Current();
  HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(sc.tmp, sc.tmp_bytes, NegIt(ks, EvalxIsNeg()), sc.negbefore, (int)n, h->stream));
  HIPCHK(h, hipcub::DeviceScan::InclusiveScan(sc.tmp, sc.tmp_bytes, HeadIt(pos0, EvalxHead{ks}), sc.runhead, hipcub::Max(), (int)n, h->stream));
  *sorted = ks;
  return FMX_OK;
}

// The rank pipeline of the exact AUC over such keys: rank_sort_scan, then k_evalx_ranksum into *d_num2, a device word the caller has
// zeroed on h->stream.  Records h->ev1 after the last kernel and returns with the stream drained.  n >= 1.
int eval_ex_rank(fmx_handle h, unsigned long long* keys, uint32_t n, int key_bits, unsigned long long* d_num2, uint64_t* num2,
                 double* rank_seconds) {
  EvalScratch sc;
  const unsigned long long* ks;
  const int rc = rank_sort_scan(h, sc, keys, n, key_bits, 0, &ks);
  if (rc) return rc;
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

// The finish of an fmx_eval_ex from the reduced sums d[3] = {squared error, absolute error, log loss} and counts of n rows: the
// fields, the rank pipeline over `keys` only when both classes are present and no row is NaN, and the timing from h->ev0 (the
// caller's) to h->ev1.  The stream is drained when it is called and when it returns.
int eval_ex_finish(fmx_handle h, uint32_t n, const double* d, uint64_t pos, uint64_t nan_rows, uint64_t correct,
                   unsigned long long* keys, int key_bits, unsigned long long* d_num2, fmx_eval_ex* out) {
  const bool cls = (h->cfg.task == FMX_TASK_CLASSIFICATION);
  out->rows = n;
  out->auc = out->logloss = std::numeric_limits<double>::quiet_NaN();
  if (!cls) {
    out->rmse = std::sqrt(d[0] / n);                                 // fm_learn.h:152
    out->mae = d[1] / n;                                             // fm_learn.h:148
  } else {
    out->pos = pos; out->neg = n - pos; out->nan_rows = nan_rows; out->correct = correct;
    out->accuracy = (double)correct / n;                             // fm_learn.h:129
    if (nan_rows == 0) out->logloss = d[2] / n;
  }
  if (cls && nan_rows == 0 && out->pos != 0 && out->neg != 0) {      // (one class only: the numerator is 0 and the AUC NaN without a sort)
    const int rc = eval_ex_rank(h, keys, n, key_bits, d_num2, &out->auc_num2, &out->rank_seconds);
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
  if (cls) HIPCHK(h, fmx_dev_alloc(&sc.keys0, (size_t)n * 8));
  hipLaunchKernelGGL(k_evalx_score, dim3(nblk), dim3(256), 0, h->stream, score, (const float*)s.target, n, make_hyper(h->cfg), add_w0,
                     (const double*)h->w0, link, dpart, cpart, sc.keys0);
  hipLaunchKernelGGL(k_evalx_final, dim3(1), dim3(64), 0, h->stream, (const double*)dpart, (const unsigned long long*)cpart, nblk, dres, cres);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemsetAsync(cres + 3, 0, 8, h->stream));
  struct { double d[3]; unsigned long long c[4]; } res;
  HIPCHK(h, hipMemcpyAsync(&res, dres, sizeof(res), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));                        // the counts decide whether anything is sorted
  return eval_ex_finish(h, n, res.d, res.c[0], res.c[1], res.c[2], sc.keys0, EVALX_KEY_BITS, cres + 3, out);
}

extern "C" {

int fmx_evaluate_ex(fmx_handle h, int slot, const fmx_eval_opts* opts, fmx_eval_ex* out) {
  static const char who[] = "fmx_evaluate_ex";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_evaluate_ex"); if (_sr) return _sr; }
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
  const float* rest;
  rc = slot_scores(h, s, nullptr, false, &rest);
  if (rc) return rc;
  if (s.wside && s.wside_version == h->w_version && s.blocks.empty()) out->flags |= FMX_EVAL_WSIDE;
  return eval_ex_scores(h, s, rest, 1, link, out);
}

}  // extern "C"
