// fmx_evalq.hip -- fmx_set_row_queries / fmx_evaluate_by_query: the exact AUC inside every query of a slot (GAUC) on the device
// (DESIGN.md section 16).  The scores come from slot_scores and the pooled metrics from eval_ex_scores, both fmx_evaluate_ex's
// (fmx_eval.hip); the same scores then feed this unit's pipeline: 64-bit keys with the query id above the score, fmx_evaluate_ex's
// sort and two scans (rank_sort_scan), a third scan for the query heads, the segmented rank sum and the reduction over the queries
// (fmx_evalq_kernels.h).  fmx_evaluate_rank (fmx_rankq.hip) runs the same pipeline through evalq_scores_keep and reads its scratch.
// The group entry points are in fmx_comm.hip, next to fmx_group_evaluate_ex.
#include "fmx_internal.h"
#include "fmx_evalq_kernels.h"

#include <limits>

void evalq_zero_per_query(uint32_t n_queries, uint64_t* num2_q, uint32_t* pos_q, uint32_t* neg_q) {
  if (num2_q) memset(num2_q, 0, (size_t)n_queries * 8);
  if (pos_q) memset(pos_q, 0, (size_t)n_queries * 4);
  if (neg_q) memset(neg_q, 0, (size_t)n_queries * 4);
}

// pooled = the empty result, no query counted, the three means NaN
void evalq_empty(fmx_eval_query* out, uint32_t n_queries) {
  memset(out, 0, sizeof(*out));
  eval_ex_empty(&out->pooled);
  out->queries = n_queries;
  out->auc_within = out->gauc = out->auc_macro = std::numeric_limits<double>::quiet_NaN();
}

int evalq_check_slot(fmx_handle h, const char* who, int slot) {
  const int rc = eval_ex_check_slot(h, who, slot);
  if (rc) return rc;
  if (!h->slots[slot].n_queries) return fail(h, FMX_E_STATE, "%s: slot %d has no query ids (call fmx_set_row_queries first)", who, slot);
  return FMX_OK;
}

int set_row_queries_impl(fmx_handle h, const char* who, int slot, const uint32_t* qid, uint32_t n_queries) {
  if (slot < 0 || slot >= FMX_MAX_SLOTS) return fail(h, FMX_E_ARG, "%s: slot %d out of range", who, slot);
  Slot& s = h->slots[slot];
  if (!s.used) return fail(h, FMX_E_STATE, "%s: slot %d holds no rows (call fmx_upload_rows first)", who, slot);
  HIPCHK(h, hipSetDevice(h->device));
  if (!qid) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    fmx_dev_free(s.qid);
    s.qid = nullptr; s.n_queries = 0;
    return FMX_OK;
  }
  if (n_queries == 0 || n_queries > 0x7FFFFFFFu) return fail(h, FMX_E_ARG, "%s: n_queries must be in 1 .. 2^31 - 1 (got %u)", who, n_queries);
  for (uint32_t r = 0; r < s.n_rows; r++)
    if (qid[r] >= n_queries) return fail(h, FMX_E_ARG, "%s: row %u has query id %u, n_queries is %u", who, r, qid[r], n_queries);
  uint32_t* d = nullptr;
  if (s.n_rows) {
    HIPCHK(h, fmx_dev_alloc(&d, (size_t)s.n_rows * 4));
    const hipError_t er = hipMemcpy(d, qid, (size_t)s.n_rows * 4, hipMemcpyHostToDevice);
    if (er != hipSuccess) { fmx_dev_free(d); return fail(h, FMX_E_HIP, "%s: %s", who, hipGetErrorString(er)); }
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  fmx_dev_free(s.qid);
  s.qid = d; s.n_queries = n_queries;
  return FMX_OK;
}

// The whole reduction over n = s.n_rows scores that are already on h's device, on h->stream: score[e] is `rest` (add_w0 = 1) or the
// finished y-hat (add_w0 = 0), exactly as eval_ex_scores takes them -- which fills out->pooled first and leaves the scores as they
// are, so the rows are scored once.  The caller has recorded h->ev0 where the call's device work began, zeroed *out (evalq_empty)
// and set out->pooled.flags.  n >= 1, s.n_queries >= 1.
// The scratch is the caller's and outlives the call (fmx_evaluate_rank reduces the top of every query segment from it, fmx_rankq.hip):
// *sorted is the buffer that holds the sorted keys, or nullptr when nothing was sorted; sc.negbefore, sc.runhead and sc.qhead are
// the three scans over it and sc.perq holds num2 [n_queries] (8 bytes each), then pos and neg (4 + 4).  The stream is drained.
int evalq_scores_keep(fmx_handle h, const Slot& s, const float* score, int add_w0, uint32_t link, fmx_eval_query* out,
                      uint64_t* num2_q, uint32_t* pos_q, uint32_t* neg_q, EvalScratch& sc, const unsigned long long** sorted) {
  const uint32_t n = s.n_rows, nq = s.n_queries;
  *sorted = nullptr;
  int rc = eval_ex_scores(h, s, score, add_w0, link, &out->pooled);
  if (rc) return rc;
  out->device_seconds = out->pooled.device_seconds;
  if (h->cfg.task != FMX_TASK_CLASSIFICATION || out->pooled.nan_rows != 0) {   // nothing is sorted
    evalq_zero_per_query(nq, num2_q, pos_q, neg_q);
    return FMX_OK;
  }
  int id_bits = 0;
  while ((1ull << id_bits) < nq) id_bits++;                                    // ceil(log2(n_queries)): 0 .. 31
  const int key_bits = EVALQ_QID_SHIFT + id_bits;
  const uint32_t qblk = evalx_grid(nq);
  HIPCHK(h, fmx_dev_alloc(&sc.keys0, (size_t)n * 8));
  HIPCHK(h, fmx_dev_alloc(&sc.qhead, (size_t)n * 4));
  HIPCHK(h, fmx_dev_alloc(&sc.perq, (size_t)nq * 16));
  HIPCHK(h, fmx_dev_alloc(&sc.part, ((size_t)qblk * 8 + 8) * 8));            // [qblk][2] doubles, [qblk][6] counts, then 2 doubles and 6 counts
  unsigned long long* d_num2 = (unsigned long long*)sc.perq;
  uint32_t* d_pos = (uint32_t*)(d_num2 + nq);
  uint32_t* d_neg = d_pos + nq;
  double* dpart = (double*)sc.part;
  unsigned long long* cpart = (unsigned long long*)sc.part + (size_t)qblk * 2;
  double* dres = (double*)sc.part + (size_t)qblk * 8;
  unsigned long long* cres = (unsigned long long*)sc.part + (size_t)qblk * 8 + 2;

  typedef hipcub::TransformInputIterator<uint32_t, EvalqQHead, hipcub::CountingInputIterator<uint32_t>> QHeadIt;
  const hipcub::CountingInputIterator<uint32_t> pos0(0);
  size_t b_qmax = 0;
  HIPCHK(h, hipcub::DeviceScan::InclusiveScan(nullptr, b_qmax, QHeadIt(pos0, EvalqQHead{sc.keys0}), sc.qhead, hipcub::Max(), (int)n, h->stream));
  hipLaunchKernelGGL(k_evalq_keys, dim3(evalx_grid(n)), dim3(256), 0, h->stream, score, (const float*)s.target, (const uint32_t*)s.qid, n,
                     make_hyper(h->cfg), add_w0, (const double*)h->w0, sc.keys0);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemsetAsync(sc.perq, 0, (size_t)nq * 16, h->stream));
  const unsigned long long* ks;
  rc = rank_sort_scan(h, sc, sc.keys0, n, key_bits, b_qmax, &ks);            // (rank_seconds starts at its sort, as fmx_evaluate_ex's does)
  if (rc) return rc;
  HIPCHK(h, hipcub::DeviceScan::InclusiveScan(sc.tmp, sc.tmp_bytes, QHeadIt(pos0, EvalqQHead{ks}), sc.qhead, hipcub::Max(), (int)n, h->stream));
  hipLaunchKernelGGL(k_evalq_ranksum, dim3(evalx_grid(n)), dim3(256), 0, h->stream, ks, (const uint32_t*)sc.negbefore, (const uint32_t*)sc.runhead,
                     (const uint32_t*)sc.qhead, n, d_num2, d_pos, d_neg);
  hipLaunchKernelGGL(k_evalq_final, dim3(qblk), dim3(256), 0, h->stream, (const unsigned long long*)d_num2, (const uint32_t*)d_pos,
                     (const uint32_t*)d_neg, nq, dpart, cpart);
  hipLaunchKernelGGL(k_evalq_final2, dim3(1), dim3(64), 0, h->stream, (const double*)dpart, (const unsigned long long*)cpart, qblk, dres, cres);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(sc.ev[1], h->stream));
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  struct { double d[2]; unsigned long long c[6]; } res;
  HIPCHK(h, hipMemcpyAsync(&res, dres, sizeof(res), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (num2_q) HIPCHK(h, hipMemcpy(num2_q, d_num2, (size_t)nq * 8, hipMemcpyDeviceToHost));
  if (pos_q) HIPCHK(h, hipMemcpy(pos_q, d_pos, (size_t)nq * 4, hipMemcpyDeviceToHost));
  if (neg_q) HIPCHK(h, hipMemcpy(neg_q, d_neg, (size_t)nq * 4, hipMemcpyDeviceToHost));
  float ms = 0, rms = 0;
  HIPCHK(h, hipEventElapsedTime(&rms, sc.ev[0], sc.ev[1]));
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  out->rank_seconds = rms * 1e-3;
  out->device_seconds = ms * 1e-3;
  out->valid_queries = res.c[0]; out->one_class_queries = res.c[1]; out->empty_queries = res.c[2];
  out->valid_rows = res.c[3]; out->num2_within = res.c[4]; out->den2_within = res.c[5];
  if (out->valid_queries) {
    out->auc_within = (double)out->num2_within / (double)out->den2_within;
    out->gauc = res.d[0] / (double)out->valid_rows;
    out->auc_macro = res.d[1] / (double)out->valid_queries;
  }
  *sorted = ks;
  return FMX_OK;
}

int evalq_scores(fmx_handle h, const Slot& s, const float* score, int add_w0, uint32_t link, fmx_eval_query* out,
                 uint64_t* num2_q, uint32_t* pos_q, uint32_t* neg_q) {
  EvalScratch sc;
  const unsigned long long* ks;
  return evalq_scores_keep(h, s, score, add_w0, link, out, num2_q, pos_q, neg_q, sc, &ks);
}

extern "C" {

int fmx_set_row_queries(fmx_handle h, int slot, const uint32_t* qid, uint32_t n_queries) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_set_row_queries"); if (_sr) return _sr; }
  return set_row_queries_impl(h, "fmx_set_row_queries", slot, qid, n_queries);
}

int fmx_evaluate_by_query(fmx_handle h, int slot, const fmx_eval_opts* opts, fmx_eval_query* out,
                          uint64_t* num2_q, uint32_t* pos_q, uint32_t* neg_q) {
  static const char who[] = "fmx_evaluate_by_query";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_evaluate_by_query"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "%s: out is NULL", who);
  uint32_t link;
  int rc = eval_ex_check_opts(h, who, opts, &link);
  if (rc) return rc;
  rc = evalq_check_slot(h, who, slot);
  if (rc) return rc;
  if (h->cfg.shard_world > 1) return fail(h, FMX_E_UNSUPPORTED, "%s on a feature shard: use fmx_group_evaluate_by_query", who);
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  evalq_empty(out, s.n_queries);
  if (s.n_rows == 0) {
    out->empty_queries = s.n_queries;
    evalq_zero_per_query(s.n_queries, num2_q, pos_q, neg_q);
    return FMX_OK;
  }
  const float* rest;
  rc = slot_scores(h, s, nullptr, false, &rest);
  if (rc) return rc;
  const uint32_t flags = (s.wside && s.wside_version == h->w_version && s.blocks.empty()) ? FMX_EVAL_WSIDE : 0u;
  out->pooled.flags = flags;
  return evalq_scores(h, s, rest, 1, link, out, num2_q, pos_q, neg_q);
}

}  // extern "C"
