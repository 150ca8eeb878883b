// fmx_topk.hip -- C-ABI (include/fmx.h): top-K retrieval of candidate rows per query row without materialising the joined rows
// (DESIGN.md section 11).  Factor sums of both row sets (sgd_partial_rows + k_topk_prep), then per chunk of queries the
// score-and-select kernel over every candidate split, a tree of pairwise merges of the splits' lists and the padded output.
// Kernels: fmx_topk_kernels.h.
#include "fmx_internal.h"
#include "fmx_topk_kernels.h"

namespace {

constexpr size_t TOPK_LIST_BYTES = size_t(1) << 30;     // per query chunk: both halves of the split lists

struct DevBufs {                                        // the call's device scratch, freed on every return
  std::vector<void*> p;
  template <class T> hipError_t alloc(T** out, size_t bytes) {
    hipError_t e = fmx_dev_alloc(out, std::max<size_t>(bytes, 256));
    if (e == hipSuccess) p.push_back((void*)*out);
    return e;
  }
  ~DevBufs() { for (void* x : p) fmx_dev_free(x); }
};
struct Events {
  hipEvent_t e[4] = {};
  ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

size_t score_lds_bytes(int buf) {
  return (size_t)(TOPK_QB + 4) * buf * sizeof(TopkEnt) + TOPK_QB * sizeof(TopkEnt) + (3 * TOPK_QB + 4) * sizeof(uint32_t);
}

}  // namespace

// factor sums of rows [row0, row0 + n) of a slot -> S_out [n][KM] (zero-padded), scal[n] = (k0 w0) + c + 1/2 |S|^2; raw: scratch of
// raw_rows * (KP + 1) floats (fmx_internal.h: shared with the hardest-of-M sampler of fmx_pairneg.hip)
int prep_rows(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n, int k0, float* raw, size_t raw_rows, int KM,
              float* S_out, float* scal, hipStream_t st, const CompactState* snap) {
  const int KP = h->KP;
  for (uint32_t r = 0; r < n; r += (uint32_t)raw_rows) {
    const uint32_t nr = (uint32_t)std::min<uint64_t>(raw_rows, n - r);
    float* S = raw;
    float* c = raw + (size_t)nr * KP;
    int rc = sgd_partial_rows(h, s, row0 + r, nr, S, c, st, snap);
    if (rc) return rc;
    hipLaunchKernelGGL(k_topk_prep, dim3(wave_grid(nr)), dim3(256), 0, st, (const float*)S, (const float*)c, nr, KP,
                       h->cfg.num_factor, KM, k0, (const double*)(snap ? snap->w0 : h->w0), S_out + (size_t)r * KM, scal + r);
    HIPCHK(h, hipGetLastError());
  }
  return FMX_OK;
}

int topk_impl(fmx_handle h, const char* who, int query_slot, int cand_slot, const fmx_topk_opts* opts, uint32_t* idx_out, double* score_out,
              fmx_topk_stats* stats, const CompactState* snap) {
  if (stats) memset(stats, 0, sizeof(*stats));
  int rc = check_slot(h, query_slot, false);
  if (rc) return rc;
  rc = check_slot(h, cand_slot, false);
  if (rc) return rc;
  if (h->cfg.shard_world > 1 || h->comm)
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", who);
  const Slot& qs = h->slots[query_slot];
  const Slot& cs = h->slots[cand_slot];
  if (!qs.blocks.empty() || !cs.blocks.empty())
    return fail(h, FMX_E_UNSUPPORTED, "%s: slots with kept `-relation` blocks are not supported", who);
  if (!opts) return fail(h, FMX_E_ARG, "%s: opts is NULL", who);
  if (!idx_out || !score_out) return fail(h, FMX_E_ARG, "%s: idx_out / score_out is NULL", who);
  const uint32_t K = opts->topk;
  if (K == 0 || K > FMX_TOPK_MAX) return fail(h, FMX_E_ARG, "%s: topk = %u (1 .. %u)", who, K, FMX_TOPK_MAX);
  if (opts->flags != 0) return fail(h, FMX_E_ARG, "%s: unknown flags 0x%x", who, opts->flags);
  const uint64_t row0 = opts->query_row0;
  const uint32_t NQ = opts->n_query;
  if (row0 > qs.n_rows || NQ > qs.n_rows - row0)
    return fail(h, FMX_E_ARG, "%s: query rows [%llu,+%u) outside the slot (%u rows)", who, (unsigned long long)row0, NQ, qs.n_rows);
  const uint32_t NC = cs.n_rows;
  // exclusion lists: validated (nothing is written on a bad index), then sorted and made unique per query
  std::vector<uint64_t> ex_ptr;
  std::vector<uint32_t> ex_idx;
  if (opts->exclude_ptr) {
    const uint64_t* p = opts->exclude_ptr;
    for (uint32_t i = 0; i < NQ; i++)
      if (p[i + 1] < p[i]) return fail(h, FMX_E_ARG, "%s: exclude_ptr decreases at query %u", who, i);
    if (p[NQ] > p[0] && !opts->exclude_idx) return fail(h, FMX_E_ARG, "%s: exclude_idx is NULL", who);
    for (uint64_t t = p[0]; t < p[NQ]; t++)
      if (opts->exclude_idx[t] >= NC)
        return fail(h, FMX_E_ARG, "%s: excluded candidate %u >= %u candidate rows", who, opts->exclude_idx[t], NC);
    ex_ptr.resize((size_t)NQ + 1);
    ex_ptr[0] = 0;
    ex_idx.reserve(p[NQ] - p[0]);
    for (uint32_t i = 0; i < NQ; i++) {
      const size_t b = ex_idx.size();
      ex_idx.insert(ex_idx.end(), opts->exclude_idx + p[i], opts->exclude_idx + p[i + 1]);
      std::sort(ex_idx.begin() + b, ex_idx.end());
      ex_idx.erase(std::unique(ex_idx.begin() + b, ex_idx.end()), ex_idx.end());
      ex_ptr[i + 1] = ex_idx.size();
    }
  }
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  if (stats) stats->scores = (uint64_t)NQ * NC;
  if (NQ == 0) return FMX_OK;
  if (NC == 0) {                                              // nothing to rank: every list is padding
    for (size_t t = 0; t < (size_t)NQ * K; t++) { idx_out[t] = TOPK_NONE; score_out[t] = -INFINITY; }
    return FMX_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const int KP = h->KP;
  const int KM = std::max(KP, 16);
  const int BUF = K >= 256 ? 256 : 128;
  const uint64_t C_pad = ((uint64_t)NC + TOPK_CT - 1) / TOPK_CT * TOPK_CT;
  const uint32_t tiles = (uint32_t)(C_pad / TOPK_CT);

  // candidate splits: enough workgroups for every CU (twice over), unless FMX_TOPK_SPLITS forces the count
  const uint64_t qblocks_all = ((uint64_t)NQ + TOPK_QB - 1) / TOPK_QB;
  uint32_t S;
  if (h->topk_splits) S = h->topk_splits;
  else S = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(512, tiles), std::max<uint64_t>(1, (2ull * h->num_cu + qblocks_all - 1) / qblocks_all));
  const uint32_t split_len = (uint32_t)((((uint64_t)NC + S - 1) / S + TOPK_CT - 1) / TOPK_CT * TOPK_CT);
  // queries per chunk: both halves of the lists within TOPK_LIST_BYTES
  uint64_t nq_chunk = TOPK_LIST_BYTES / (2ull * S * K * sizeof(TopkEnt)) / TOPK_QB * TOPK_QB;
  nq_chunk = std::max<uint64_t>(nq_chunk, TOPK_QB);
  nq_chunk = std::min<uint64_t>(nq_chunk, qblocks_all * TOPK_QB);
  const uint32_t nq_pad = (uint32_t)nq_chunk;
  if (stats) stats->splits = S;

  DevBufs db;
  Events ev;
  for (hipEvent_t& e : ev.e) HIPCHK(h, hipEventCreate(&e));
  float *Sc = nullptr, *bc = nullptr, *Sq = nullptr, *aq = nullptr, *raw = nullptr, *d_score = nullptr;
  TopkEnt* lists = nullptr;
  uint32_t *lens = nullptr, *d_idx = nullptr;
  uint64_t* d_ex_ptr = nullptr;
  uint32_t* d_ex_idx = nullptr;
  const size_t raw_rows = std::max<size_t>(TOPK_QB, PREP_RAW_FLOATS / (size_t)(KP + 1));
  HIPCHK(h, db.alloc(&Sc, (size_t)C_pad * KM * sizeof(float)));
  HIPCHK(h, db.alloc(&bc, (size_t)C_pad * sizeof(float)));
  HIPCHK(h, db.alloc(&Sq, (size_t)nq_pad * KM * sizeof(float)));
  HIPCHK(h, db.alloc(&aq, (size_t)nq_pad * sizeof(float)));
  HIPCHK(h, db.alloc(&raw, raw_rows * (size_t)(KP + 1) * sizeof(float)));
  HIPCHK(h, db.alloc(&lists, 2ull * S * nq_pad * K * sizeof(TopkEnt)));
  HIPCHK(h, db.alloc(&lens, 2ull * S * nq_pad * sizeof(uint32_t)));
  HIPCHK(h, db.alloc(&d_idx, (size_t)nq_pad * K * sizeof(uint32_t)));
  HIPCHK(h, db.alloc(&d_score, (size_t)nq_pad * K * sizeof(float)));
  if (!ex_ptr.empty()) {
    HIPCHK(h, db.alloc(&d_ex_ptr, ex_ptr.size() * sizeof(uint64_t)));
    HIPCHK(h, db.alloc(&d_ex_idx, std::max<size_t>(ex_idx.size(), 1) * sizeof(uint32_t)));
    HIPCHK(h, hipMemcpyAsync(d_ex_ptr, ex_ptr.data(), ex_ptr.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (!ex_idx.empty()) HIPCHK(h, hipMemcpyAsync(d_ex_idx, ex_idx.data(), ex_idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }

  HIPCHK(h, hipEventRecord(ev.e[0], st));
  HIPCHK(h, hipMemsetAsync(Sc + (size_t)NC * KM, 0, (size_t)(C_pad - NC) * KM * sizeof(float), st));
  HIPCHK(h, hipMemsetAsync(bc + NC, 0, (size_t)(C_pad - NC) * sizeof(float), st));
  rc = prep_rows(h, cs, 0, NC, 0, raw, raw_rows, KM, Sc, bc, st, snap);
  if (rc) return rc;

  // the score kernel of this (KM, BUF)
  const void* kfn = nullptr;
#define TOPK_KFN(KMV) do { if (KM == KMV) kfn = BUF == 256 ? (const void*)k_topk_score<KMV, 256> : (const void*)k_topk_score<KMV, 128>; } while (0)
  TOPK_KFN(16); TOPK_KFN(32); TOPK_KFN(64); TOPK_KFN(128); TOPK_KFN(256); TOPK_KFN(512); TOPK_KFN(1024);
#undef TOPK_KFN
  if (!kfn) return fail(h, FMX_E_UNSUPPORTED, "num_factor > 1024 is not supported");
  const size_t lds = score_lds_bytes(BUF);
  if (!h->lds_raised.count(kfn)) {
    HIPCHK(h, hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    h->lds_raised.insert(kfn);
  }

  std::vector<uint32_t> h_idx;
  std::vector<float> h_score;
  double score_s = 0.0;
  for (uint64_t qoff = 0; qoff < NQ; qoff += nq_chunk) {
    const uint32_t nqc = (uint32_t)std::min<uint64_t>(nq_chunk, NQ - qoff);
    const uint32_t qblocks = (nqc + TOPK_QB - 1) / TOPK_QB;
    HIPCHK(h, hipMemsetAsync(Sq, 0, (size_t)nq_pad * KM * sizeof(float), st));
    HIPCHK(h, hipMemsetAsync(aq, 0, (size_t)nq_pad * sizeof(float), st));
    rc = prep_rows(h, qs, row0 + qoff, nqc, h->cfg.k0, raw, raw_rows, KM, Sq, aq, st, snap);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(ev.e[2], st));
    const uint64_t* xp = d_ex_ptr ? d_ex_ptr + qoff : nullptr;
    void* args[] = {(void*)&Sq, (void*)&aq, (void*)&nqc, (void*)&nq_pad, (void*)&Sc, (void*)&bc, (void*)&NC, (void*)&split_len,
                    (void*)&S, (void*)&xp, (void*)&d_ex_idx, (void*)&K, (void*)&lists, (void*)&lens};
    HIPCHK(h, hipLaunchKernel(kfn, dim3(qblocks, S), dim3(256), args, lds, st));
    // merge rounds: splits 2p, 2p + 1 -> p, alternating between the two halves of `lists` (and of `lens`)
    TopkEnt* cur = lists;
    TopkEnt* nxt = lists + (size_t)S * nq_pad * K;
    uint32_t* lcur = lens;
    uint32_t* lnxt = lens + (size_t)S * nq_pad;
    for (uint32_t s_in = S; s_in > 1; s_in = (s_in + 1) / 2) {
      const uint64_t work = (uint64_t)nqc * ((s_in + 1) / 2);
      hipLaunchKernelGGL(k_topk_merge2, dim3(wave_grid(work)), dim3(256), 0, st, (const TopkEnt*)cur, (const uint32_t*)lcur, s_in, nqc,
                         nq_pad, K, nxt, lnxt);
      std::swap(cur, nxt);
      std::swap(lcur, lnxt);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(ev.e[3], st));
    hipLaunchKernelGGL(k_topk_emit, dim3(std::min<uint64_t>(((uint64_t)nqc * K + 255) / 256, 4096)), dim3(256), 0, st,
                       (const TopkEnt*)cur, (const uint32_t*)lcur, nqc, K, d_idx, d_score);
    HIPCHK(h, hipGetLastError());
    h_idx.resize((size_t)nqc * K);
    h_score.resize((size_t)nqc * K);
    HIPCHK(h, hipMemcpyAsync(h_idx.data(), d_idx, h_idx.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(h_score.data(), d_score, h_score.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipEventRecord(ev.e[1], st));
    HIPCHK(h, hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
    score_s += ms * 1e-3;
    const size_t o = (size_t)qoff * K;
    for (size_t t = 0; t < h_idx.size(); t++) { idx_out[o + t] = h_idx[t]; score_out[o + t] = (double)h_score[t]; }
  }
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  if (stats) { stats->device_seconds = ms * 1e-3; stats->score_seconds = score_s; }
  return FMX_OK;
}

extern "C" {

int fmx_topk(fmx_handle h, int query_slot, int cand_slot, const fmx_topk_opts* opts, uint32_t* idx_out, double* score_out,
             fmx_topk_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_topk"); if (_sr) return _sr; }
  return topk_impl(h, "fmx_topk", query_slot, cand_slot, opts, idx_out, score_out, stats, nullptr);
}

}  // extern "C"
