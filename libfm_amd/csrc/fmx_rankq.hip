// fmx_rankq.hip -- fmx_rank_discounts / fmx_evaluate_rank: exact tie-averaged NDCG, recall and precision at K inside every query of a
// slot, on the device.  The call is fmx_evaluate_by_query's (evalq_scores_keep, fmx_evalq.hip: one scoring pass,
// one sort, three scans, the per-query counts) with its scratch kept alive, then one more reduction over the top of every query
// segment of the same sorted keys (fmx_rankq_kernels.h).
// The group entry point is in fmx_comm.hip, next to fmx_group_evaluate_by_query.
#include "fmx_internal.h"
#include "fmx_rankq_kernels.h"

#include <limits>

namespace {

// D[r + 1] = D[r] + 1.0 / log2((double)r + 2.0), sequentially: the one place the table is computed, for the caller and the device
void rank_discounts(uint32_t k_max, double* out) {
  out[0] = 0.0;
  for (uint32_t r = 0; r < k_max; r++) out[r + 1] = out[r] + 1.0 / std::log2((double)r + 2.0);
}

struct RankScratch {                        // what the top-K reduction takes from the device beyond EvalScratch
  uint32_t* qend = nullptr;                 // [n_queries] end of the query's segment of the sorted keys
  double* table = nullptr;                  // [k_max + 1] discounts
  double* dcg_q = nullptr; double* hits_q = nullptr;   // [n_queries][n_cutoffs], only when asked for
  void* part = nullptr;                     // block partials + results
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~RankScratch() {
    fmx_dev_free(qend); fmx_dev_free(table); fmx_dev_free(dcg_q); fmx_dev_free(hits_q); fmx_dev_free(part);
    for (auto e : ev) if (e) hipEventDestroy(e);
  }
};

}  // namespace

int rankq_check_opts(fmx_handle h, const char* who, const fmx_rank_opts* opts, uint32_t* link) {
  if (!opts) return fail(h, FMX_E_ARG, "%s: opts is NULL", who);
  const fmx_eval_opts eo = {opts->link, opts->flags};
  const int rc = eval_ex_check_opts(h, who, &eo, link);
  if (rc) return rc;
  if (opts->n_cutoffs < 1 || opts->n_cutoffs > FMX_RANK_MAX_CUTOFFS)
    return fail(h, FMX_E_ARG, "%s: n_cutoffs must be in 1 .. %d (got %u)", who, FMX_RANK_MAX_CUTOFFS, opts->n_cutoffs);
  for (uint32_t j = 0; j < opts->n_cutoffs; j++) {
    if (opts->k[j] < 1 || opts->k[j] > FMX_RANK_MAX_K)
      return fail(h, FMX_E_ARG, "%s: cutoff %u must be in 1 .. %u (got %u)", who, j, FMX_RANK_MAX_K, opts->k[j]);
    if (j && opts->k[j] <= opts->k[j - 1])
      return fail(h, FMX_E_ARG, "%s: the cutoffs must be strictly ascending (%u after %u)", who, opts->k[j], opts->k[j - 1]);
  }
  return FMX_OK;
}

// by_query = the empty result, no query relevant, every mean NaN, the arrays zero-filled
void rankq_empty(fmx_eval_rank* out, const fmx_rank_opts* opts, uint32_t n_queries, double* dcg_q, double* hits_q) {
  memset(out, 0, sizeof(*out));
  evalq_empty(&out->by_query, n_queries);
  out->n_cutoffs = opts->n_cutoffs;
  for (uint32_t j = 0; j < opts->n_cutoffs; j++) {
    out->at[j].k = opts->k[j];
    out->at[j].ndcg = out->at[j].recall = out->at[j].precision = std::numeric_limits<double>::quiet_NaN();
  }
  const size_t cells = (size_t)n_queries * opts->n_cutoffs;
  if (dcg_q) memset(dcg_q, 0, cells * sizeof(double));
  if (hits_q) memset(hits_q, 0, cells * sizeof(double));
}

// The whole reduction over n = s.n_rows scores that are on h's device, as evalq_scores takes them.  The caller has recorded h->ev0
// where the call's device work began, prepared *out (rankq_empty) and set out->by_query.pooled.flags.  n >= 1, s.n_queries >= 1.
int rankq_scores(fmx_handle h, const Slot& s, const float* score, int add_w0, uint32_t link, const fmx_rank_opts* opts,
                 fmx_eval_rank* out, double* dcg_q, double* hits_q) {
  const uint32_t n = s.n_rows, nq = s.n_queries, nc = opts->n_cutoffs, k_max = opts->k[nc - 1];
  EvalScratch sc;
  const unsigned long long* ks;
  int rc = evalq_scores_keep(h, s, score, add_w0, link, &out->by_query, nullptr, nullptr, nullptr, sc, &ks);
  if (rc) return rc;
  out->device_seconds = out->by_query.device_seconds;
  if (!ks) return FMX_OK;                                                      // nothing was sorted: the empty figures stand
  const uint32_t* d_pos = (const uint32_t*)((const unsigned long long*)sc.perq + nq);
  const uint32_t* d_neg = d_pos + nq;
  const uint32_t qblk = rankq_grid(nq);
  const size_t cells = (size_t)nq * nc;
  RankScratch rs;
  HIPCHK(h, fmx_dev_alloc(&rs.qend, (size_t)nq * 4));
  HIPCHK(h, fmx_dev_alloc(&rs.table, ((size_t)k_max + 1) * 8));
  if (dcg_q) HIPCHK(h, fmx_dev_alloc(&rs.dcg_q, cells * 8));
  if (hits_q) HIPCHK(h, fmx_dev_alloc(&rs.hits_q, cells * 8));
  HIPCHK(h, fmx_dev_alloc(&rs.part, ((size_t)qblk + 1) * (RANKQ_ND + RANKQ_NC) * 8));   // [qblk][ND] doubles, [qblk][NC] counts, then ND doubles and NC counts
  for (auto& e : rs.ev) HIPCHK(h, hipEventCreate(&e));
  double* dpart = (double*)rs.part;
  unsigned long long* cpart = (unsigned long long*)rs.part + (size_t)qblk * RANKQ_ND;
  double* dres = (double*)rs.part + (size_t)qblk * (RANKQ_ND + RANKQ_NC);
  unsigned long long* cres = (unsigned long long*)dres + RANKQ_ND;
  std::vector<double> table((size_t)k_max + 1);
  rank_discounts(k_max, table.data());
  HIPCHK(h, hipMemcpy(rs.table, table.data(), table.size() * 8, hipMemcpyHostToDevice));   // synchronous: the vector may go on any path out
  RankqCut cut;
  cut.n = nc;
  for (int j = 0; j < RANKQ_MAX_CUT; j++) cut.k[j] = (uint32_t)j < nc ? opts->k[j] : 0u;
  HIPCHK(h, hipEventRecord(rs.ev[0], h->stream));
  hipLaunchKernelGGL(k_rankq_bounds, dim3(evalx_grid(n)), dim3(256), 0, h->stream, ks, n, rs.qend);
  hipLaunchKernelGGL(k_rankq_top, dim3(qblk), dim3(256), 0, h->stream, ks, (const uint32_t*)sc.negbefore, (const uint32_t*)sc.runhead,
                     (const uint32_t*)rs.qend, d_pos, d_neg, nq, cut, (const double*)rs.table, rs.dcg_q, rs.hits_q, dpart, cpart);
  hipLaunchKernelGGL(k_rankq_final2, dim3(1), dim3(64), 0, h->stream, (const double*)dpart, (const unsigned long long*)cpart, qblk, dres, cres);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(rs.ev[1], h->stream));
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  struct { double d[RANKQ_ND]; unsigned long long c[RANKQ_NC]; } res;
  HIPCHK(h, hipMemcpyAsync(&res, dres, sizeof(res), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (dcg_q) HIPCHK(h, hipMemcpy(dcg_q, rs.dcg_q, cells * 8, hipMemcpyDeviceToHost));
  if (hits_q) HIPCHK(h, hipMemcpy(hits_q, rs.hits_q, cells * 8, hipMemcpyDeviceToHost));
  float ms = 0, tms = 0;
  HIPCHK(h, hipEventElapsedTime(&tms, rs.ev[0], rs.ev[1]));
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  out->topk_seconds = tms * 1e-3;
  out->device_seconds = ms * 1e-3;
  out->relevant_queries = res.c[RANKQ_MAX_CUT];
  for (uint32_t j = 0; j < nc; j++) {
    fmx_rank_at& at = out->at[j];
    if (!out->relevant_queries) continue;                                      // the means stay NaN, hits and tied_queries 0
    at.tied_queries = res.c[j];
    at.hits = res.d[4 * j + 0];
    at.ndcg = res.d[4 * j + 1] / (double)out->relevant_queries;
    at.recall = res.d[4 * j + 2] / (double)out->relevant_queries;
    at.precision = res.d[4 * j + 3] / (double)out->relevant_queries;
  }
  return FMX_OK;
}

extern "C" {

int fmx_rank_discounts(uint32_t k_max, double* out) {
  if (!out) return fail(nullptr, FMX_E_ARG, "fmx_rank_discounts: out is NULL");
  if (k_max > FMX_RANK_MAX_K) return fail(nullptr, FMX_E_ARG, "fmx_rank_discounts: k_max must be at most %u (got %u)", FMX_RANK_MAX_K, k_max);
  rank_discounts(k_max, out);
  return FMX_OK;
}

int fmx_evaluate_rank(fmx_handle h, int slot, const fmx_rank_opts* opts, fmx_eval_rank* out, double* dcg_q, double* hits_q) {
  static const char who[] = "fmx_evaluate_rank";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_evaluate_rank"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "%s: out is NULL", who);
  uint32_t link;
  int rc = rankq_check_opts(h, who, opts, &link);
  if (rc) return rc;
  rc = evalq_check_slot(h, who, slot);
  if (rc) return rc;
  if (h->cfg.shard_world > 1) return fail(h, FMX_E_UNSUPPORTED, "%s on a feature shard: use fmx_group_evaluate_rank", who);
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  rankq_empty(out, opts, s.n_queries, dcg_q, hits_q);
  if (s.n_rows == 0) {
    out->by_query.empty_queries = s.n_queries;
    return FMX_OK;
  }
  const float* rest;
  rc = slot_scores(h, s, nullptr, false, &rest);
  if (rc) return rc;
  out->by_query.pooled.flags = (s.wside && s.wside_version == h->w_version && s.blocks.empty()) ? FMX_EVAL_WSIDE : 0u;
  return rankq_scores(h, s, rest, 1, link, opts, out, dcg_q, hits_q);
}

}  // extern "C"
