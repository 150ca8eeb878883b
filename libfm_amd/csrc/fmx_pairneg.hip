// fmx_pairneg.hip -- C-ABI (include/fmx.h): BPR on (query row, candidate row) interactions with the negatives drawn on the device
// (DESIGN.md sections 12 and 13).  Per epoch: k_neg_sample (FMX_NEG_HARDEST: the row tables of fmx_topk, then k_neg_pick), then FMX_SGD_SEQUENTIAL (k_pair_seq over the joined rows) or FMX_SGD_MINIBATCH
// (the pairs' entries -- the query's once -- bucketed by (batch, feature), sums + multipliers, owner apply).  Kernels:
// fmx_pairneg_kernels.h.  fmx_adapt_pair_epoch_sampled / fmx_ftrl_pair_epoch_sampled: the same epoch with the open session's rule in
// the owner (fmx_pair_rule_kernels.h).
#include "fmx_internal.h"
#include "fmx_pairneg_kernels.h"
#include "fmx_pair_rule_kernels.h"

static_assert(FMX_NEG_ATTEMPTS == NEG_ATTEMPTS, "include/fmx.h and fmx_pairneg_kernels.h disagree");

// the interactions of a query slot.  The three scratch blocks are kept between epochs (grown, never shrunk): by_pairs holds what is
// sized by the pairs P = n * n_neg (20 P bytes + the scan's temporary), by_entries what is sized by the expanded entries
// N = sum over the pairs of |x_q| + |x_c+| + |x_c-| (40 N bytes + the sort's temporary), by_rows (FMX_NEG_HARDEST only) the factor
// sums of the Q query and C candidate rows, (Q + C)(KM + 1) * 4 bytes + one piece of raw sums; nothing is sized by Q x C.
struct PairNeg {
  int       cand = -1;
  uint64_t  n = 0;
  uint32_t* q = nullptr;            // device [n]
  uint32_t* c = nullptr;
  uint64_t* ex_ptr = nullptr;       // device [Q + 1] / ex_idx: sorted, unique per query; nullptr: no exclusion lists
  uint32_t* ex_idx = nullptr;
  char*     by_pairs = nullptr;   size_t by_pairs_bytes = 0;
  char*     by_entries = nullptr; size_t by_entries_bytes = 0;
  char*     by_rows = nullptr;    size_t by_rows_bytes = 0;
};

extern "C++" void free_interactions(Slot& s) {
  PairNeg* pn = s.pneg;
  if (!pn) return;
  for (void* p : {(void*)pn->q, (void*)pn->c, (void*)pn->ex_ptr, (void*)pn->ex_idx, (void*)pn->by_pairs, (void*)pn->by_entries,
                  (void*)pn->by_rows})
    if (p) fmx_dev_free(p);
  delete pn;
  s.pneg = nullptr;
}

extern "C++" void drop_interactions(fmx_handle h, int slot) {
  for (int i = 0; i < FMX_MAX_SLOTS; i++) {
    Slot& s = h->slots[i];
    if (s.pneg && (i == slot || s.pneg->cand == slot)) free_interactions(s);
  }
}

namespace {

hipError_t grow(char** buf, size_t* have, size_t want) {
  if (*buf && *have >= want) return hipSuccess;
  if (*buf) fmx_dev_free(*buf);
  *buf = nullptr; *have = 0;
  const size_t bytes = want + want / 16;                      // (the entries of an epoch vary with its negatives)
  hipError_t e = fmx_dev_alloc(buf, bytes);
  if (e == hipSuccess) *have = bytes;
  return e;
}
size_t al256(size_t x) { return (x + 255) / 256 * 256; }

struct SetupClock {                                           // host seconds into h->setup_acc
  fmx_handle h; std::chrono::steady_clock::time_point t0;
  ~SetupClock() { h->setup_acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

uint32_t neg_draws(const fmx_pairneg_opts* o) { return (o->flags >> 8) & 0xFFu; }
// (one draw is the uniform sampler itself: k_neg_sample, no tables)
bool neg_hardest(const fmx_pairneg_opts* o) { return (o->flags & FMX_NEG_HARDEST) && neg_draws(o) > 1; }

// what every entry point that uses the interactions refuses (the handle stays usable)
int pairneg_check(fmx_handle h, int slot, const fmx_pairneg_opts* o, const char* what) {
  if (!h) return FMX_E_ARG;
  if (!o) return fail(h, FMX_E_ARG, "%s: opts is NULL", what);
  if (o->flags & ~(FMX_NEG_HARDEST | FMX_NEG_DRAWS(0xFFu))) return fail(h, FMX_E_ARG, "%s: unknown flags 0x%x", what, o->flags);
  const uint32_t draws = neg_draws(o);
  if (!(o->flags & FMX_NEG_HARDEST) && draws) return fail(h, FMX_E_ARG, "%s: FMX_NEG_DRAWS without FMX_NEG_HARDEST", what);
  if ((o->flags & FMX_NEG_HARDEST) && (draws == 0 || draws > FMX_NEG_ATTEMPTS))
    return fail(h, FMX_E_ARG, "%s: FMX_NEG_HARDEST with %u draws (1 .. %u)", what, draws, FMX_NEG_ATTEMPTS);
  if (o->n_neg == 0) return fail(h, FMX_E_ARG, "%s: n_neg = 0 (at least one negative per interaction)", what);
  if (o->mode == FMX_SGD_HOGWILD) return fail(h, FMX_E_UNSUPPORTED, "%s: FMX_SGD_HOGWILD is not supported for pairs", what);
  if (o->mode != FMX_SGD_SEQUENTIAL && o->mode != FMX_SGD_MINIBATCH) return fail(h, FMX_E_ARG, "%s: unknown mode %d", what, o->mode);
  int rc = check_slot(h, slot, false);
  if (rc) return rc;
  if (h->cfg.shard_world > 1 || h->comm)
    return fail(h, FMX_E_UNSUPPORTED, "%s: interactions are not supported on feature shards / communicator ranks", what);
  const Slot& qs = h->slots[slot];
  if (!qs.pneg) return fail(h, FMX_E_STATE, "%s: slot %d holds no interactions (call fmx_upload_interactions first)", what, slot);
  const int cand = qs.pneg->cand;
  rc = check_slot(h, cand, false);
  if (rc) return rc;
  if (!qs.blocks.empty() || !h->slots[cand].blocks.empty())
    return fail(h, FMX_E_UNSUPPORTED, "%s: relations are not supported with pairwise SGD", what);
  rc = slot_in_session(h, slot, what);
  if (rc) return rc;
  rc = slot_in_session(h, cand, what);
  if (rc) return rc;
  if (h->sgda.reg) return fail(h, FMX_E_STATE, "%s: an SGDA session is open (call fmx_sgda_end first)", what);
  if (qs.pneg->n && h->slots[cand].n_rows == 0) return fail(h, FMX_E_ARG, "%s: the candidate slot is empty", what);
  if (qs.pneg->n > ((1ull << 31) - 2) / o->n_neg)
    return fail(h, FMX_E_UNSUPPORTED, "%s: more than 2^31 - 2 pairs (n * n_neg: split the interactions)", what);
  return FMX_OK;
}

JoinSrc join_src(const Slot& qs, const Slot& cs, const PairNeg& pn, const uint32_t* neg, uint32_t n_neg) {
  return JoinSrc{qs.ent, qs.row_ptr, cs.ent, cs.row_ptr, pn.q, pn.c, neg, n_neg};
}

// the negatives of (seed, epoch) into by_pairs: neg [P] at offset 0; the forced count comes back in *forced.  Layout of by_pairs:
// neg [P] u32 | off [P + 1] u64 | len [P] u64 | forced partials | forced sum | scan temporary
// FMX_NEG_HARDEST with more than one draw: the tables S_q [Q][KM], S_c [C][KM], b_c [C] of the parameters as they are NOW
// (prep_rows, k0 = 0) into by_rows -- once when the query slot is the candidate slot -- and k_neg_pick instead of k_neg_sample.
struct PairsLayout { size_t o_neg, o_off, o_len, o_part, o_sum, o_tmp, tmp_bytes, bytes; };
int pairs_layout(fmx_handle h, uint64_t P, PairsLayout* L) {
  size_t tmp = 0;
  HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, (int)std::min<uint64_t>(P + 1, INT32_MAX), h->stream));
  size_t off = 0;
  L->o_neg = off; off += al256(P * 4);
  L->o_off = off; off += al256((P + 1) * 8);
  L->o_len = off; off += al256((P + 1) * 8);
  L->o_part = off; off += al256(std::max(NEG_MAX_BLOCKS, 4 * NEG_PICK_MAX_BLOCKS) * 4);
  L->o_sum = off; off += 256;
  L->o_tmp = off; L->tmp_bytes = std::max<size_t>(tmp, 256); off += al256(L->tmp_bytes);
  L->bytes = off;
  return FMX_OK;
}

int hard_tables(fmx_handle h, const Slot& qs, const Slot& cs, PairNeg& pn, int KM, NegTabs* out) {
  const bool same = &qs == &cs;
  const size_t Q = same ? 0 : qs.n_rows, NC = cs.n_rows;
  const size_t raw_rows = std::min<size_t>(std::max<size_t>(std::max(Q, NC), 1), std::max<size_t>(1, PREP_RAW_FLOATS / (size_t)(h->KP + 1)));
  size_t off = 0;
  const size_t o_sc = off; off += al256(NC * KM * sizeof(float));
  const size_t o_bc = off; off += al256(NC * sizeof(float));
  const size_t o_sq = off; off += al256(Q * KM * sizeof(float));
  const size_t o_aq = off; off += al256(Q * sizeof(float));
  const size_t o_raw = off; off += al256(raw_rows * (size_t)(h->KP + 1) * sizeof(float));
  HIPCHK(h, grow(&pn.by_rows, &pn.by_rows_bytes, off));
  char* sc = pn.by_rows;
  float* raw = (float*)(sc + o_raw);
  int rc = prep_rows(h, cs, 0, (uint32_t)NC, 0, raw, raw_rows, KM, (float*)(sc + o_sc), (float*)(sc + o_bc), h->stream);
  if (rc) return rc;
  if (!same) {
    rc = prep_rows(h, qs, 0, (uint32_t)Q, 0, raw, raw_rows, KM, (float*)(sc + o_sq), (float*)(sc + o_aq), h->stream);
    if (rc) return rc;
  }
  out->Sc = (const float*)(sc + o_sc);
  out->bc = (const float*)(sc + o_bc);
  out->Sq = same ? out->Sc : (const float*)(sc + o_sq);
  return FMX_OK;
}

int sample(fmx_handle h, const Slot& qs, const Slot& cs, PairNeg& pn, const fmx_pairneg_opts* o, const PairsLayout& L, uint64_t* forced) {
  const uint64_t P = pn.n * o->n_neg;
  hipStream_t st = h->stream;
  HIPCHK(h, grow(&pn.by_pairs, &pn.by_pairs_bytes, L.bytes));
  uint32_t* neg = (uint32_t*)(pn.by_pairs + L.o_neg);
  uint32_t* part = (uint32_t*)(pn.by_pairs + L.o_part);
  uint64_t* sum = (uint64_t*)(pn.by_pairs + L.o_sum);
  const NegSrc in{pn.q, pn.c, pn.ex_ptr, pn.ex_idx, pn.n, cs.n_rows};
  uint32_t nparts = 0;
  if (neg_hardest(o)) {
    const int KM = std::max(h->KP, 16);
    NegTabs tabs;
    int rc = hard_tables(h, qs, cs, pn, KM, &tabs);
    if (rc) return rc;
    const uint32_t nblk = (uint32_t)std::min<uint64_t>((P + 3) / 4, NEG_PICK_MAX_BLOCKS);
    nparts = 4 * nblk;
    switch (KM) {
#define PICK_CASE(KMV) case KMV: hipLaunchKernelGGL((k_neg_pick<KMV>), dim3(nblk), dim3(256), 0, st, in, tabs, o->n_neg, neg_draws(o), o->seed, o->epoch, neg, part); break;
      PICK_CASE(16) PICK_CASE(32) PICK_CASE(64) PICK_CASE(128) PICK_CASE(256) PICK_CASE(512) PICK_CASE(1024)
#undef PICK_CASE
      default: return fail(h, FMX_E_UNSUPPORTED, "num_factor > 1024 is not supported");
    }
  } else {
    nparts = (uint32_t)std::min<uint64_t>((P + 255) / 256, NEG_MAX_BLOCKS);
    hipLaunchKernelGGL(k_neg_sample, dim3(nparts), dim3(256), 0, st, in, o->n_neg, o->seed, o->epoch, neg, part);
  }
  hipLaunchKernelGGL(k_neg_forced_sum, dim3(1), dim3(64), 0, st, (const uint32_t*)part, nparts, sum);
  HIPCHK(h, hipGetLastError());
  if (forced) {
    HIPCHK(h, hipMemcpyAsync(forced, sum, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
  }
  return FMX_OK;
}

// the (batch, feature) bucketing of one epoch's pairs
struct Buckets {
  const TEntry* t_ent = nullptr; const uint32_t* seg_head = nullptr; const uint32_t* seg_feat = nullptr;
  uint32_t nseg = 0, max_seg = 0;
  std::vector<uint32_t> batch_seg;
};

int bucket(fmx_handle h, const JoinSrc& js, PairNeg& pn, uint64_t P, uint32_t B, const PairsLayout& L, Buckets* out) {
  hipStream_t st = h->stream;
  uint64_t* off = (uint64_t*)(pn.by_pairs + L.o_off);
  uint64_t* len = (uint64_t*)(pn.by_pairs + L.o_len);
  const uint32_t grid = (uint32_t)std::min<uint64_t>((P + 255) / 256, 2048);
  hipLaunchKernelGGL(k_pn_len, dim3(grid), dim3(256), 0, st, js, P, len);
  HIPCHK(h, hipMemsetAsync(len + P, 0, 8, st));
  size_t tb_ = L.tmp_bytes;
  HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(pn.by_pairs + L.o_tmp, tb_, len, off, (int)(P + 1), st));
  uint64_t N = 0;
  HIPCHK(h, hipMemcpyAsync(&N, off + P, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (N >= (1ull << 31) - 1)
    return fail(h, FMX_E_UNSUPPORTED, "fmx_pair_epoch_sampled: %llu expanded entries (2^31 - 1 at most: split the interactions)", (unsigned long long)N);
  const uint32_t n_batches = (uint32_t)((P + B - 1) / B);
  out->batch_seg.assign((size_t)n_batches + 1, 0u);
  if (N == 0) return FMX_OK;
  uint32_t fbits = 1; while (fbits < 32 && (1ull << fbits) < std::max<uint64_t>(h->n_local, 2)) fbits++;
  int bits_batch = 1; while ((1ull << bits_batch) < n_batches) bits_batch++;
  size_t tmp_sort = 0, tmp_scan = 0;
  HIPCHK(h, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                               (int)N, 0, (int)fbits + bits_batch, st));
  HIPCHK(h, hipcub::DeviceScan::InclusiveSum(nullptr, tmp_scan, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)N, st));
  const size_t tmp_bytes = std::max<size_t>(std::max(tmp_sort, tmp_scan), 256);
  const size_t cnt = (size_t)N;
  size_t o = 0;
  const size_t o_ka = o; o += al256(cnt * 8);                 // keys; after the sort: head [nseg + 1]
  const size_t o_kb = o; o += al256(cnt * 8);
  const size_t o_va = o; o += al256(cnt * 8);
  const size_t o_te = o; o += al256(cnt * 8);
  const size_t o_fl = o; o += al256(std::max<size_t>(cnt, (size_t)n_batches + 1) * 4);
  const size_t o_po = o; o += al256(cnt * 4);
  const size_t o_ct = o; o += 256;
  const size_t o_tmp = o; o += al256(tmp_bytes);
  HIPCHK(h, grow(&pn.by_entries, &pn.by_entries_bytes, o));
  char* sc = pn.by_entries;
  uint64_t* keys_a = (uint64_t*)(sc + o_ka); uint64_t* keys_b = (uint64_t*)(sc + o_kb); uint64_t* vals_a = (uint64_t*)(sc + o_va);
  TEntry* t_ent = (TEntry*)(sc + o_te);
  uint32_t* flags = (uint32_t*)(sc + o_fl); uint32_t* pos = (uint32_t*)(sc + o_po);
  uint32_t* d_counts = (uint32_t*)(sc + o_ct);                // {segments, -, longest segment, -}
  void* tmp = sc + o_tmp;
  HIPCHK(h, hipMemsetAsync(d_counts, 0, 16, st));
  hipLaunchKernelGGL(k_pn_keys, dim3(wave_grid(P)), dim3(256), 0, st, js, (const uint64_t*)off, P, B, fbits, keys_a, vals_a);
  size_t tb2 = tmp_bytes;
  HIPCHK(h, hipcub::DeviceRadixSort::SortPairs(tmp, tb2, keys_a, keys_b, vals_a, reinterpret_cast<uint64_t*>(t_ent), (int)N, 0,
                                               (int)fbits + bits_batch, st));
  hipLaunchKernelGGL(k_seg_heads, dim3(2048), dim3(256), 0, st, keys_b, N, flags);
  tb2 = tmp_bytes;
  HIPCHK(h, hipcub::DeviceScan::InclusiveSum(tmp, tb2, flags, pos, (int)N, st));
  uint32_t* head = reinterpret_cast<uint32_t*>(keys_a);
  hipLaunchKernelGGL(k_seg_head_pos, dim3(2048), dim3(256), 0, st, flags, pos, N, head);
  hipLaunchKernelGGL(k_seg_max_count, dim3(2048), dim3(256), 0, st, head, pos, N, d_counts + 2);
  HIPCHK(h, hipMemcpyAsync(d_counts, pos + (N - 1), 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(h, hipGetLastError());
  uint32_t counts[4] = {0, 0, 0, 0};
  HIPCHK(h, hipMemcpyAsync(counts, d_counts, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  out->nseg = counts[0]; out->max_seg = counts[2];
  uint32_t* feat = reinterpret_cast<uint32_t*>(vals_a);       // (free after the sort, like keys_a)
  hipLaunchKernelGGL(k_pair_seg_feat, dim3(2048), dim3(256), 0, st, keys_b, head, out->nseg, fbits, feat);
  hipLaunchKernelGGL(k_pair_batch_seg, dim3((n_batches + 256) / 256), dim3(256), 0, st, keys_b, head, out->nseg, fbits, n_batches, flags);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(out->batch_seg.data(), flags, ((size_t)n_batches + 1) * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  out->t_ent = t_ent; out->seg_head = head; out->seg_feat = feat;
  return FMX_OK;
}

}  // namespace

extern "C" {

int fmx_upload_interactions(fmx_handle h, int query_slot, int cand_slot, const uint32_t* q_row, const uint32_t* c_row, uint64_t n,
                            const uint64_t* exclude_ptr, const uint32_t* exclude_idx) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_upload_interactions"); if (_sr) return _sr; }
  int rc = check_slot(h, query_slot, false);
  if (rc) return rc;
  rc = check_slot(h, cand_slot, false);
  if (rc) return rc;
  if (n && (!q_row || !c_row)) return fail(h, FMX_E_ARG, "fmx_upload_interactions: q_row / c_row is NULL");
  Slot& qs = h->slots[query_slot];
  const uint32_t Q = qs.n_rows, NC = h->slots[cand_slot].n_rows;
  for (uint64_t t = 0; t < n; t++)
    if (q_row[t] >= Q || c_row[t] >= NC)
      return fail(h, FMX_E_ARG, "fmx_upload_interactions: interaction %llu = (%u, %u) names a row outside its slot (%u query, %u candidate rows)",
                  (unsigned long long)t, q_row[t], c_row[t], Q, NC);
  // exclusion lists: validated, then sorted and made unique per query (the device binary-searches them)
  std::vector<uint64_t> ex_ptr;
  std::vector<uint32_t> ex_idx;
  if (exclude_ptr) {
    const uint64_t* p = exclude_ptr;
    for (uint32_t i = 0; i < Q; i++)
      if (p[i + 1] < p[i]) return fail(h, FMX_E_ARG, "fmx_upload_interactions: exclude_ptr decreases at query %u", i);
    if (p[Q] > p[0] && !exclude_idx) return fail(h, FMX_E_ARG, "fmx_upload_interactions: exclude_idx is NULL");
    for (uint64_t t = p[0]; t < p[Q]; t++)
      if (exclude_idx[t] >= NC)
        return fail(h, FMX_E_ARG, "fmx_upload_interactions: excluded candidate %u >= %u candidate rows", exclude_idx[t], NC);
    ex_ptr.resize((size_t)Q + 1);
    ex_ptr[0] = 0;
    ex_idx.reserve(p[Q] - p[0]);
    for (uint32_t i = 0; i < Q; i++) {
      const size_t b = ex_idx.size();
      ex_idx.insert(ex_idx.end(), exclude_idx + p[i], exclude_idx + p[i + 1]);
      std::sort(ex_idx.begin() + b, ex_idx.end());
      ex_idx.erase(std::unique(ex_idx.begin() + b, ex_idx.end()), ex_idx.end());
      ex_ptr[i + 1] = ex_idx.size();
    }
  }
  HIPCHK(h, hipSetDevice(h->device));
  Slot tmp;                                                    // (only its pneg is used: free_interactions on every early return)
  tmp.pneg = new PairNeg();
  PairNeg& pn = *tmp.pneg;
  pn.cand = cand_slot; pn.n = n;
  const size_t np = (size_t)std::max<uint64_t>(n, 1);
  hipError_t er = fmx_dev_alloc(&pn.q, np * 4);
  if (er == hipSuccess) er = fmx_dev_alloc(&pn.c, np * 4);
  if (er == hipSuccess && n) er = hipMemcpy(pn.q, q_row, n * 4, hipMemcpyHostToDevice);
  if (er == hipSuccess && n) er = hipMemcpy(pn.c, c_row, n * 4, hipMemcpyHostToDevice);
  if (er == hipSuccess && !ex_ptr.empty()) {
    er = fmx_dev_alloc(&pn.ex_ptr, ex_ptr.size() * 8);
    if (er == hipSuccess) er = fmx_dev_alloc(&pn.ex_idx, std::max<size_t>(ex_idx.size(), 1) * 4);
    if (er == hipSuccess) er = hipMemcpy(pn.ex_ptr, ex_ptr.data(), ex_ptr.size() * 8, hipMemcpyHostToDevice);
    if (er == hipSuccess && !ex_idx.empty()) er = hipMemcpy(pn.ex_idx, ex_idx.data(), ex_idx.size() * 4, hipMemcpyHostToDevice);
  }
  if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  if (er != hipSuccess) {                                     // the previous interactions stay as they were
    free_interactions(tmp);
    return fail(h, FMX_E_HIP, "fmx_upload_interactions: %s", hipGetErrorString(er));
  }
  free_interactions(qs);
  qs.pneg = tmp.pneg;
  tmp.pneg = nullptr;
  return FMX_OK;
}

int fmx_interactions_info(fmx_handle h, int query_slot, int* cand_slot, uint64_t* n) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_interactions_info"); if (_sr) return _sr; }
  int rc = check_slot(h, query_slot, false);
  if (rc) return rc;
  const PairNeg* pn = h->slots[query_slot].pneg;
  if (!pn) return fail(h, FMX_E_STATE, "fmx_interactions_info: slot %d holds no interactions (call fmx_upload_interactions first)", query_slot);
  if (cand_slot) *cand_slot = pn->cand;
  if (n) *n = pn->n;
  return FMX_OK;
}

int fmx_pair_sample(fmx_handle h, int query_slot, const fmx_pairneg_opts* o, uint32_t* neg_out, uint64_t* forced_out) {
  if (forced_out) *forced_out = 0;
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_pair_sample"); if (_sr) return _sr; }
  int rc = pairneg_check(h, query_slot, o, "fmx_pair_sample");
  if (rc) return rc;
  PairNeg& pn = *h->slots[query_slot].pneg;
  const uint64_t P = pn.n * o->n_neg;
  if (P == 0) return FMX_OK;
  if (!neg_out) return fail(h, FMX_E_ARG, "fmx_pair_sample: neg_out is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  PairsLayout L;
  rc = pairs_layout(h, P, &L);
  if (rc) return rc;
  uint64_t forced = 0;
  if (neg_hardest(o)) { int _rc = lag_flush(h); if (_rc) return _rc; }   // (the scores read the parameters)
  rc = sample(h, h->slots[query_slot], h->slots[pn.cand], pn, o, L, &forced);
  if (rc) return rc;
  HIPCHK(h, hipMemcpy(neg_out, pn.by_pairs + L.o_neg, P * 4, hipMemcpyDeviceToHost));
  if (forced_out) *forced_out = forced;
  return FMX_OK;
}

// one epoch over the interactions of a query slot for `what` (fmx_pair_epoch_sampled and the rule epochs): they differ in their
// refusals and in the owner launch of a batch (launch_pair_owner), nothing else
static int pairneg_epoch_run(fmx_handle h, int query_slot, const fmx_pairneg_opts* o, fmx_epoch_stats* stats, uint64_t* forced_out,
                             const char* what, PairRule rule) {
  if (stats) memset(stats, 0, sizeof(*stats));
  if (forced_out) *forced_out = 0;
  int rc = (h && o) ? pair_rule_check_mode(h, rule, o->mode, what) : FMX_OK;
  if (rc) return rc;
  rc = pairneg_check(h, query_slot, o, what);
  if (rc) return rc;
  rc = pair_rule_check_session(h, rule, what);
  if (rc) return rc;
  uint32_t B = 1;
  if (o->mode == FMX_SGD_MINIBATCH) {
    B = o->batch ? o->batch : FMX_PAIR_DEFAULT_BATCH;
    if (B >= (1u << 30)) return fail(h, FMX_E_ARG, "%s: batch %u (2^30 - 1 at most)", what, B);
  }
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& qs = h->slots[query_slot];
  PairNeg& pn = *qs.pneg;
  const Slot& cs = h->slots[pn.cand];
  const Hyper hy = make_hyper(h->cfg);
  const int k = h->cfg.num_factor;
  h->setup_acc = 0.0;
  const uint64_t P = pn.n * o->n_neg;
  if (P == 0) return FMX_OK;
  touch_w(h);                                                 // (a slot's weight side stream is stale from here on)
  hipStream_t st = h->stream;
  uint64_t forced = 0, batches = 0;
  uint32_t max_seg = 0;
  PairsLayout L;
  Buckets bk;
  {
    SetupClock clk{h, std::chrono::steady_clock::now()};
    rc = pairs_layout(h, P, &L);
    if (rc) return rc;
    rc = sample(h, qs, cs, pn, o, L, &forced);
    if (rc) return rc;
  }
  const JoinSrc js = join_src(qs, cs, pn, (const uint32_t*)(pn.by_pairs + L.o_neg), o->n_neg);
  if (o->mode == FMX_SGD_SEQUENTIAL) {
    // an upper bound of the longest pair (2 |x_q| + |x_c+| + |x_c-|) picks the staging buffer; both give the same result
    const uint64_t max_len = 2ull * qs.max_row + 2ull * cs.max_row;
    if (max_len > 0xFFFFFFFFull) return fail(h, FMX_E_UNSUPPORTED, "fmx_pair_epoch_sampled: rows too long");
    const bool use_lds = max_len <= PAIR_SEQ_LDS_ENT;
    PairEnt* gbuf = nullptr;
    if (!use_lds) HIPCHK(h, fmx_dev_alloc(&gbuf, (size_t)max_len * sizeof(PairEnt)));
    HIPCHK(h, hipEventRecord(h->ev0, st));
    hipLaunchKernelGGL(k_pair_seq<JoinSrc>, dim3(1), dim3(PAIR_SEQ_THREADS), 0, st, js, P, h->tb, hy, k, h->w0, gbuf, (uint32_t)(use_lds ? 1u : 0u));
    hipError_t le = hipGetLastError();
    HIPCHK(h, hipEventRecord(h->ev1, st));
    hipError_t se = hipStreamSynchronize(st);
    if (gbuf) fmx_dev_free(gbuf);
    HIPCHK(h, le);
    HIPCHK(h, se);
    batches = P;
  } else {
    const uint32_t nbc = (uint32_t)std::min<uint64_t>(B, P);
    char* scr = nullptr;
    const size_t s_bytes = al256((size_t)nbc * 3 * (size_t)h->KP * sizeof(float));
    {
      SetupClock clk{h, std::chrono::steady_clock::now()};
      rc = bucket(h, js, pn, P, B, L, &bk);
      if (rc) return rc;
      HIPCHK(h, fmx_dev_alloc(&scr, s_bytes + (size_t)nbc * sizeof(double)));
    }
    max_seg = bk.max_seg;
    float* S = reinterpret_cast<float*>(scr);
    double* mult = reinterpret_cast<double*>(scr + s_bytes);
    double w0 = 0.0;
    hipError_t er = hipMemcpy(&w0, h->w0, sizeof(double), hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipEventRecord(h->ev0, st);
    for (uint64_t p0 = 0; er == hipSuccess && p0 < P; p0 += B) {
      const uint32_t nb = (uint32_t)std::min<uint64_t>(B, P - p0);
      const uint64_t b = p0 / B;
      const uint32_t s0 = bk.batch_seg[b], s1 = bk.batch_seg[b + 1];
      KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_pn_sums<KP>), nb, st, js, p0, nb, h->tb, k, h->cfg.k1, S, mult));
      if (s1 > s0) launch_pair_owner<3>(h, rule, bk.t_ent, bk.seg_head, bk.seg_feat, s0, s1, S, mult, hy, st);
      er = hipGetLastError();
      batches++;
    }
    if (er == hipSuccess) er = hipEventRecord(h->ev1, st);
    if (er == hipSuccess) er = hipStreamSynchronize(st);
    if (er == hipSuccess && hy.k0) {                            // fm_sgd.h:56 once per pair, fp64, in order
      for (uint64_t t = 0; t < P; t++) w0 -= h->cfg.reg0 * w0;
      er = hipMemcpy(h->w0, &w0, sizeof(double), hipMemcpyHostToDevice);
    }
    fmx_dev_free(scr);
    HIPCHK(h, er);
  }
  if (forced_out) *forced_out = forced;
  if (stats) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    stats->rows = P;
    stats->batches = batches;
    stats->batch_used = B;
    stats->device_seconds = ms * 1e-3;
    stats->main_kernel_seconds = stats->device_seconds;
    stats->main_kernel_launches = (o->mode == FMX_SGD_SEQUENTIAL) ? 1 : 2 * batches;
    stats->max_feature_count = max_seg;
    stats->setup_seconds = h->setup_acc;
  }
  return FMX_OK;
}

int fmx_pair_epoch_sampled(fmx_handle h, int query_slot, const fmx_pairneg_opts* o, fmx_epoch_stats* stats, uint64_t* forced_out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_pair_epoch_sampled"); if (_sr) return _sr; }
  return pairneg_epoch_run(h, query_slot, o, stats, forced_out, "fmx_pair_epoch_sampled", PAIR_PLAIN);
}
int fmx_adapt_pair_epoch_sampled(fmx_handle h, int query_slot, const fmx_pairneg_opts* o, fmx_epoch_stats* stats, uint64_t* forced_out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_adapt_pair_epoch_sampled"); if (_sr) return _sr; }
  return pairneg_epoch_run(h, query_slot, o, stats, forced_out, "fmx_adapt_pair_epoch_sampled", PAIR_ADAGRAD);
}
int fmx_ftrl_pair_epoch_sampled(fmx_handle h, int query_slot, const fmx_pairneg_opts* o, fmx_epoch_stats* stats, uint64_t* forced_out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_ftrl_pair_epoch_sampled"); if (_sr) return _sr; }
  return pairneg_epoch_run(h, query_slot, o, stats, forced_out, "fmx_ftrl_pair_epoch_sampled", PAIR_FTRL);
}

int fmx_pair_evaluate_sampled(fmx_handle h, int query_slot, const fmx_pairneg_opts* o, fmx_pair_eval* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_pair_evaluate_sampled"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_pair_evaluate_sampled: out is NULL");
  memset(out, 0, sizeof(*out));
  int rc = pairneg_check(h, query_slot, o, "fmx_pair_evaluate_sampled");
  if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& qs = h->slots[query_slot];
  PairNeg& pn = *qs.pneg;
  const Slot& cs = h->slots[pn.cand];
  const uint64_t P = pn.n * o->n_neg;
  out->pairs = P;
  if (P == 0) return FMX_OK;
  hipStream_t st = h->stream;
  PairsLayout L;
  rc = pairs_layout(h, P, &L);
  if (rc) return rc;
  rc = sample(h, qs, cs, pn, o, L, nullptr);
  if (rc) return rc;
  const JoinSrc js = join_src(qs, cs, pn, (const uint32_t*)(pn.by_pairs + L.o_neg), o->n_neg);
  const uint32_t nblk = (uint32_t)std::min<uint64_t>((P + 3) / 4, PAIR_EVAL_BLOCKS);
  double* part = nullptr;
  HIPCHK(h, fmx_dev_alloc(&part, ((size_t)nblk * 2 + 2) * sizeof(double)));
  hipError_t er = hipEventRecord(h->ev0, st);
  if (er == hipSuccess) {
    const int k = h->cfg.num_factor;
    switch (h->KP) {
#define PN_EVAL_CASE(KPV) case KPV: hipLaunchKernelGGL((k_pn_eval<KPV>), dim3(nblk), dim3(256), 0, st, js, P, h->tb, k, h->cfg.k1, part); break;
      PN_EVAL_CASE(1) PN_EVAL_CASE(2) PN_EVAL_CASE(4) PN_EVAL_CASE(8) PN_EVAL_CASE(16) PN_EVAL_CASE(32) PN_EVAL_CASE(64)
      PN_EVAL_CASE(128) PN_EVAL_CASE(256) PN_EVAL_CASE(512) PN_EVAL_CASE(1024)
#undef PN_EVAL_CASE
      default: fmx_dev_free(part); return fail(h, FMX_E_UNSUPPORTED, "num_factor > 1024 is not supported");
    }
    hipLaunchKernelGGL(k_pair_eval_final, dim3(1), dim3(64), 0, st, (const double*)part, nblk, part + 2 * nblk);
    er = hipGetLastError();
  }
  if (er == hipSuccess) er = hipEventRecord(h->ev1, st);
  double res[2] = {0.0, 0.0};
  if (er == hipSuccess) er = hipMemcpyAsync(res, part + 2 * nblk, sizeof(res), hipMemcpyDeviceToHost, st);
  if (er == hipSuccess) er = hipStreamSynchronize(st);
  fmx_dev_free(part);
  HIPCHK(h, er);
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  out->accuracy = res[0] / (double)P;
  out->loss = res[1] / (double)P;
  out->device_seconds = ms * 1e-3;
  return FMX_OK;
}

}  // extern "C"
