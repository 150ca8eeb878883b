// fmx_pair.hip -- C-ABI (include/fmx.h): pairwise ranking (BPR) around fm_pairSGD -- the pairs of a slot, one epoch in order
// (FMX_SGD_SEQUENTIAL) or by the batch rule (FMX_SGD_MINIBATCH: the (batch, feature) bucketing of the pair-expanded entries,
// sums + multipliers, owner apply), the same epoch stepped by an open fmx_adapt / fmx_ftrl session's rule (fmx_adapt_pair_epoch,
// fmx_ftrl_pair_epoch), and the pair metrics.  Kernels: fmx_pair_kernels.h, fmx_pair_rule_kernels.h.
#include "fmx_internal.h"
#include "fmx_pair_kernels.h"
#include "fmx_pair_rule_kernels.h"

static void free_pair_segments(Slot& s) {
  if (s.pair_t_ent) fmx_dev_free(s.pair_t_ent);
  if (s.pair_seg_head) fmx_dev_free(s.pair_seg_head);
  if (s.pair_seg_feat) fmx_dev_free(s.pair_seg_feat);
  s.pair_t_ent = nullptr; s.pair_seg_head = nullptr; s.pair_seg_feat = nullptr;
  s.pair_seg_B = 0; s.pair_nseg = 0; s.pair_max_seg = 0;
  s.pair_batch_seg.clear();
}

extern "C++" void free_pairs(Slot& s) {
  free_pair_segments(s);
  if (s.pair_a) fmx_dev_free(s.pair_a);
  if (s.pair_b) fmx_dev_free(s.pair_b);
  if (s.pair_off) fmx_dev_free(s.pair_off);
  s.pair_a = nullptr; s.pair_b = nullptr; s.pair_off = nullptr;
  s.pairs_set = false; s.n_pairs = 0; s.pair_nnz = 0; s.pair_max_len = 0;
}

// what every pair entry point refuses (the handle stays usable)
static int pair_check(fmx_handle h, int slot, const char* what) {
  int rc = check_slot(h, slot, false);
  if (rc) return rc;
  if (h->cfg.shard_world > 1 || h->comm)
    return fail(h, FMX_E_UNSUPPORTED, "%s: pairs are not supported on feature shards / communicator ranks", what);
  const Slot& s = h->slots[slot];
  if (!s.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "%s: relations are not supported with pairwise SGD", what);   // as fm_learn_sgd.h:61-63
  rc = slot_in_session(h, slot, what);
  if (rc) return rc;
  if (h->sgda.reg) return fail(h, FMX_E_STATE, "%s: an SGDA session is open (call fmx_sgda_end first)", what);
  if (!s.pairs_set) return fail(h, FMX_E_STATE, "%s: slot %d holds no pairs (call fmx_upload_pairs first)", what, slot);
  return FMX_OK;
}

extern "C++" int pair_rule_check_mode(fmx_handle h, PairRule r, int mode, const char* what) {
  if (r != PAIR_PLAIN && (mode == FMX_SGD_SEQUENTIAL || mode == FMX_SGD_HOGWILD))
    return fail(h, FMX_E_UNSUPPORTED, "%s: a per-coordinate rule runs on FMX_SGD_MINIBATCH only (batch = 1 gives the per-pair rule); "
                "FMX_SGD_SEQUENTIAL and FMX_SGD_HOGWILD have no such form", what);
  return FMX_OK;
}
extern "C++" int pair_rule_check_session(fmx_handle h, PairRule r, const char* what) {
  if (r == PAIR_ADAGRAD && !h->adapt.nv) return fail(h, FMX_E_STATE, "%s before fmx_adapt_begin", what);
  if (r == PAIR_FTRL && !h->ftrl.nv) return fail(h, FMX_E_STATE, "%s before fmx_ftrl_begin", what);
  if (r == PAIR_FTRL && h->adapt.nv) return fail(h, FMX_E_STATE, "%s: an fmx_adapt session is open", what);
  return FMX_OK;
}

// the (batch, feature) bucketing of the pair-expanded entries (like ensure_segments: device radix sort, stable; once per
// (slot, pairs, B))
static int ensure_pair_segments(fmx_handle h, Slot& s, uint32_t B) {
  if (s.pair_seg_B == B && s.pair_t_ent) return FMX_OK;
  free_pair_segments(s);
  const auto t0 = std::chrono::steady_clock::now();
  struct Acc { fmx_handle h; std::chrono::steady_clock::time_point t0;
               ~Acc() { h->setup_acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } } acc_{h, t0};
  const uint64_t N = s.pair_nnz;
  if (N >= (1ull << 31) - 1)
    return fail(h, FMX_E_UNSUPPORTED, "fmx_pair_epoch: %llu pair-expanded entries (2^31 at most: split the pairs)", (unsigned long long)N);
  const uint32_t n_batches = (uint32_t)((s.n_pairs + B - 1) / B);
  uint32_t fbits = 1; while (fbits < 32 && (1ull << fbits) < std::max<uint64_t>(h->n_local, 2)) fbits++;
  int bits_batch = 1; while ((1ull << bits_batch) < n_batches) bits_batch++;
  hipStream_t st = h->stream;
  const size_t cnt = (size_t)std::max<uint64_t>(N, 1);
  char* scratch = nullptr;
  int rc = FMX_OK;
#define PSEG_CHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
    rc = fail(h, FMX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); goto done; } } while (0)
  {
    size_t tmp_sort = 0, tmp_scan = 0;
    PSEG_CHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                                (int)cnt, 0, (int)fbits + bits_batch, st));
    PSEG_CHK(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_scan, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)cnt, st));
    const size_t tmp_bytes = std::max<size_t>(std::max(tmp_sort, tmp_scan), 256);
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t off = 0;
    const size_t o_ka = off; off += al(cnt * 8);
    const size_t o_kb = off; off += al(cnt * 8);
    const size_t o_va = off; off += al(cnt * 8);
    const size_t o_fl = off; off += al(std::max<size_t>(cnt, (size_t)n_batches + 1) * 4);   // (also the per-batch table at the end)
    const size_t o_po = off; off += al(cnt * 4);
    const size_t o_ct = off; off += 256;
    const size_t o_tmp = off; off += al(tmp_bytes);
    PSEG_CHK(fmx_dev_alloc(&scratch, off));
    uint64_t* keys_a = (uint64_t*)(scratch + o_ka); uint64_t* keys_b = (uint64_t*)(scratch + o_kb); uint64_t* vals_a = (uint64_t*)(scratch + o_va);
    uint32_t* flags = (uint32_t*)(scratch + o_fl); uint32_t* pos = (uint32_t*)(scratch + o_po);
    uint32_t* d_counts = (uint32_t*)(scratch + o_ct);           // {segments, -, longest segment, -}
    void* tmp = scratch + o_tmp;
    PSEG_CHK(fmx_dev_alloc(&s.pair_t_ent, cnt * 8));
    PSEG_CHK(hipMemsetAsync(d_counts, 0, 16, st));
    uint32_t counts[4] = {0, 0, 0, 0};
    if (N) {
      hipLaunchKernelGGL(k_pair_keys, dim3(wave_grid(s.n_pairs)), dim3(256), 0, st, s.ent, s.row_ptr, s.pair_a, s.pair_b, s.pair_off,
                         s.n_pairs, B, fbits, keys_a, vals_a);
      size_t tb_ = tmp_bytes;
      PSEG_CHK(hipcub::DeviceRadixSort::SortPairs(tmp, tb_, keys_a, keys_b, vals_a, reinterpret_cast<uint64_t*>(s.pair_t_ent), (int)N, 0,
                                                  (int)fbits + bits_batch, st));
      hipLaunchKernelGGL(k_seg_heads, dim3(2048), dim3(256), 0, st, keys_b, N, flags);
      tb_ = tmp_bytes;
      PSEG_CHK(hipcub::DeviceScan::InclusiveSum(tmp, tb_, flags, pos, (int)N, st));
      uint32_t* head = reinterpret_cast<uint32_t*>(keys_a);      // keys_a is free after the sort: head[nseg + 1] <= 8 bytes per entry
      hipLaunchKernelGGL(k_seg_head_pos, dim3(2048), dim3(256), 0, st, flags, pos, N, head);
      hipLaunchKernelGGL(k_seg_max_count, dim3(2048), dim3(256), 0, st, head, pos, N, d_counts + 2);
      PSEG_CHK(hipMemcpyAsync(d_counts, pos + (N - 1), 4, hipMemcpyDeviceToDevice, st));
      PSEG_CHK(hipGetLastError());
      PSEG_CHK(hipMemcpyAsync(counts, d_counts, 16, hipMemcpyDeviceToHost, st));
      PSEG_CHK(hipStreamSynchronize(st));
      s.pair_nseg = counts[0]; s.pair_max_seg = counts[2];
      PSEG_CHK(fmx_dev_alloc(&s.pair_seg_head, ((size_t)s.pair_nseg + 1) * 4));
      PSEG_CHK(fmx_dev_alloc(&s.pair_seg_feat, (size_t)std::max<uint32_t>(s.pair_nseg, 1) * 4));
      PSEG_CHK(hipMemcpyAsync(s.pair_seg_head, head, ((size_t)s.pair_nseg + 1) * 4, hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(k_pair_seg_feat, dim3(2048), dim3(256), 0, st, keys_b, head, s.pair_nseg, fbits, s.pair_seg_feat);
      hipLaunchKernelGGL(k_pair_batch_seg, dim3((n_batches + 256) / 256), dim3(256), 0, st, keys_b, head, s.pair_nseg, fbits, n_batches, flags);
      PSEG_CHK(hipGetLastError());
      s.pair_batch_seg.resize((size_t)n_batches + 1);
      PSEG_CHK(hipMemcpyAsync(s.pair_batch_seg.data(), flags, ((size_t)n_batches + 1) * 4, hipMemcpyDeviceToHost, st));
      PSEG_CHK(hipStreamSynchronize(st));
    } else {
      s.pair_nseg = 0; s.pair_max_seg = 0;
      PSEG_CHK(fmx_dev_alloc(&s.pair_seg_head, 4));
      PSEG_CHK(fmx_dev_alloc(&s.pair_seg_feat, 4));
      s.pair_batch_seg.assign((size_t)n_batches + 1, 0u);
    }
    s.pair_seg_B = B;
  }
done:
#undef PSEG_CHK
  if (scratch) fmx_dev_free(scratch);
  if (rc) free_pair_segments(s);
  return rc;
}

extern "C" {

int fmx_upload_pairs(fmx_handle h, int slot, const uint32_t* row_a, const uint32_t* row_b, uint64_t n_pairs) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_upload_pairs"); if (_sr) return _sr; }
  int rc = check_slot(h, slot, false);
  if (rc) return rc;
  if (n_pairs && (!row_a || !row_b)) return fail(h, FMX_E_ARG, "fmx_upload_pairs: row_a / row_b is NULL");
  Slot& s = h->slots[slot];
  for (uint64_t t = 0; t < n_pairs; t++)
    if (row_a[t] >= s.n_rows || row_b[t] >= s.n_rows)
      return fail(h, FMX_E_ARG, "fmx_upload_pairs: pair %llu = (%u, %u) names a row outside the slot (%u rows)", (unsigned long long)t,
                  row_a[t], row_b[t], s.n_rows);
  HIPCHK(h, hipSetDevice(h->device));
  // the pair-expanded entry stream: pair t's x_a then x_b start at off[t]
  std::vector<uint64_t> rp((size_t)s.n_rows + 1);
  HIPCHK(h, hipMemcpy(rp.data(), s.row_ptr, rp.size() * 8, hipMemcpyDeviceToHost));
  std::vector<uint64_t> off((size_t)n_pairs + 1);
  uint64_t tot = 0;
  uint32_t max_len = 0;
  for (uint64_t t = 0; t < n_pairs; t++) {
    off[t] = tot;
    const uint64_t len = (rp[row_a[t] + 1] - rp[row_a[t]]) + (rp[row_b[t] + 1] - rp[row_b[t]]);
    tot += len;
    max_len = std::max<uint32_t>(max_len, (uint32_t)std::min<uint64_t>(len, 0xFFFFFFFFull));
  }
  off[n_pairs] = tot;
  uint32_t *pa = nullptr, *pb = nullptr;
  uint64_t* po = nullptr;
  const size_t np = (size_t)std::max<uint64_t>(n_pairs, 1);
  hipError_t er = fmx_dev_alloc(&pa, np * 4);
  if (er == hipSuccess) er = fmx_dev_alloc(&pb, np * 4);
  if (er == hipSuccess) er = fmx_dev_alloc(&po, (np + 1) * 8);
  if (er == hipSuccess && n_pairs) er = hipMemcpy(pa, row_a, n_pairs * 4, hipMemcpyHostToDevice);
  if (er == hipSuccess && n_pairs) er = hipMemcpy(pb, row_b, n_pairs * 4, hipMemcpyHostToDevice);
  if (er == hipSuccess) er = hipMemcpy(po, off.data(), off.size() * 8, hipMemcpyHostToDevice);
  if (er != hipSuccess) {                                     // the previous pairs stay as they were
    if (pa) fmx_dev_free(pa);
    if (pb) fmx_dev_free(pb);
    if (po) fmx_dev_free(po);
    return fail(h, FMX_E_HIP, "fmx_upload_pairs: %s", hipGetErrorString(er));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  free_pairs(s);
  s.pair_a = pa; s.pair_b = pb; s.pair_off = po;
  s.n_pairs = n_pairs; s.pair_nnz = tot; s.pair_max_len = max_len; s.pairs_set = true;
  return FMX_OK;
}

// one epoch over the pairs of a slot for `what` (fmx_pair_epoch and the rule epochs): they differ in their refusals and in the
// owner launch of a batch (launch_pair_owner), nothing else
static int pair_epoch_run(fmx_handle h, int slot, const fmx_pair_opts* opts, fmx_epoch_stats* stats, const char* what, PairRule rule) {
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!h) return FMX_E_ARG;
  if (!opts) return fail(h, FMX_E_ARG, "%s: opts is NULL", what);
  int rc = pair_rule_check_mode(h, rule, opts->mode, what);
  if (rc) return rc;
  if (opts->mode == FMX_SGD_HOGWILD) return fail(h, FMX_E_UNSUPPORTED, "%s: FMX_SGD_HOGWILD is not supported for pairs", what);
  if (opts->mode != FMX_SGD_SEQUENTIAL && opts->mode != FMX_SGD_MINIBATCH) return fail(h, FMX_E_ARG, "%s: unknown mode %d", what, opts->mode);
  rc = pair_check(h, slot, what);
  if (rc) return rc;
  rc = pair_rule_check_session(h, rule, what);
  if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[slot];
  const Hyper hy = make_hyper(h->cfg);
  const int k = h->cfg.num_factor;
  h->setup_acc = 0.0;
  touch_w(h);                                                 // (a slot's weight side stream is stale from here on)
  const uint64_t P = s.n_pairs;
  uint64_t batches = 0;
  uint32_t B = 1;
  if (P == 0) return FMX_OK;
  if (opts->mode == FMX_SGD_SEQUENTIAL) {
    const bool use_lds = s.pair_max_len <= PAIR_SEQ_LDS_ENT;
    PairEnt* gbuf = nullptr;
    if (!use_lds) HIPCHK(h, fmx_dev_alloc(&gbuf, (size_t)s.pair_max_len * sizeof(PairEnt)));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(k_pair_seq<PairSlotSrc>, dim3(1), dim3(PAIR_SEQ_THREADS), 0, h->stream, PairSlotSrc{s.ent, s.row_ptr, s.pair_a, s.pair_b}, P,
                       h->tb, hy, k, h->w0, gbuf, (uint32_t)(use_lds ? 1u : 0u));
    hipError_t le = hipGetLastError();
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    hipError_t se = hipStreamSynchronize(h->stream);
    if (gbuf) fmx_dev_free(gbuf);
    HIPCHK(h, le);
    HIPCHK(h, se);
    batches = P;
  } else {
    B = opts->batch ? opts->batch : FMX_PAIR_DEFAULT_BATCH;
    if (B >= (1u << 31)) return fail(h, FMX_E_ARG, "%s: batch %u (2^31 - 1 at most)", what, B);
    rc = ensure_pair_segments(h, s, B);
    if (rc) return rc;
    const uint32_t nbc = (uint32_t)std::min<uint64_t>(B, P);
    char* scr = nullptr;
    const size_t s_bytes = ((size_t)nbc * 2 * (size_t)h->KP * sizeof(float) + 255) / 256 * 256;
    HIPCHK(h, fmx_dev_alloc(&scr, s_bytes + (size_t)nbc * sizeof(double)));
    float* S = reinterpret_cast<float*>(scr);
    double* mult = reinterpret_cast<double*>(scr + s_bytes);
    double w0 = 0.0;
    hipError_t er = hipMemcpy(&w0, h->w0, sizeof(double), hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipEventRecord(h->ev0, h->stream);
    for (uint64_t t0 = 0; er == hipSuccess && t0 < P; t0 += B) {
      const uint32_t nb = (uint32_t)std::min<uint64_t>(B, P - t0);
      const uint64_t b = t0 / B;
      const uint32_t s0 = s.pair_batch_seg[b], s1 = s.pair_batch_seg[b + 1];
      KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_pair_sums<KP>), nb, h->stream, s.ent, s.row_ptr, s.pair_a, s.pair_b, t0, nb, h->tb, k, h->cfg.k1, S, mult));
      if (s1 > s0) launch_pair_owner<2>(h, rule, s.pair_t_ent, s.pair_seg_head, s.pair_seg_feat, s0, s1, S, mult, hy, h->stream);
      er = hipGetLastError();
      batches++;
    }
    if (er == hipSuccess) er = hipEventRecord(h->ev1, h->stream);
    if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
    if (er == hipSuccess && hy.k0) {                            // fm_sgd.h:56 once per pair, fp64, in order
      for (uint64_t t = 0; t < P; t++) w0 -= h->cfg.reg0 * w0;
      er = hipMemcpy(h->w0, &w0, sizeof(double), hipMemcpyHostToDevice);
    }
    fmx_dev_free(scr);
    HIPCHK(h, er);
  }
  if (stats) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    stats->rows = P;
    stats->batches = batches;
    stats->batch_used = B;
    stats->device_seconds = ms * 1e-3;
    stats->main_kernel_seconds = stats->device_seconds;
    stats->main_kernel_launches = (opts->mode == FMX_SGD_SEQUENTIAL) ? 1 : 2 * batches;
    if (opts->mode == FMX_SGD_MINIBATCH) stats->max_feature_count = s.pair_max_seg;
    stats->setup_seconds = h->setup_acc;
  }
  return FMX_OK;
}

int fmx_pair_epoch(fmx_handle h, int slot, const fmx_pair_opts* opts, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_pair_epoch"); if (_sr) return _sr; }
  return pair_epoch_run(h, slot, opts, stats, "fmx_pair_epoch", PAIR_PLAIN);
}
int fmx_adapt_pair_epoch(fmx_handle h, int slot, const fmx_pair_opts* opts, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_adapt_pair_epoch"); if (_sr) return _sr; }
  return pair_epoch_run(h, slot, opts, stats, "fmx_adapt_pair_epoch", PAIR_ADAGRAD);
}
int fmx_ftrl_pair_epoch(fmx_handle h, int slot, const fmx_pair_opts* opts, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_ftrl_pair_epoch"); if (_sr) return _sr; }
  return pair_epoch_run(h, slot, opts, stats, "fmx_ftrl_pair_epoch", PAIR_FTRL);
}

int fmx_pair_evaluate(fmx_handle h, int slot, fmx_pair_eval* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_pair_evaluate"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_pair_evaluate: out is NULL");
  memset(out, 0, sizeof(*out));
  int rc = pair_check(h, slot, "fmx_pair_evaluate");
  if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  out->pairs = s.n_pairs;
  if (s.n_pairs == 0) return FMX_OK;
  const uint32_t nblk = (uint32_t)std::min<uint64_t>((s.n_pairs + 3) / 4, PAIR_EVAL_BLOCKS);
  double* part = nullptr;
  HIPCHK(h, fmx_dev_alloc(&part, ((size_t)nblk * 2 + 2) * sizeof(double)));
  hipError_t er = hipEventRecord(h->ev0, h->stream);
  if (er == hipSuccess) {
    const int k = h->cfg.num_factor;
    switch (h->KP) {
#define PAIR_EVAL_CASE(KPV) case KPV: hipLaunchKernelGGL((k_pair_eval<KPV>), dim3(nblk), dim3(256), 0, h->stream, s.ent, s.row_ptr, s.pair_a, s.pair_b, \
                                                      s.n_pairs, h->tb, k, h->cfg.k1, part); break;
      PAIR_EVAL_CASE(1) PAIR_EVAL_CASE(2) PAIR_EVAL_CASE(4) PAIR_EVAL_CASE(8) PAIR_EVAL_CASE(16) PAIR_EVAL_CASE(32) PAIR_EVAL_CASE(64)
      PAIR_EVAL_CASE(128) PAIR_EVAL_CASE(256) PAIR_EVAL_CASE(512) PAIR_EVAL_CASE(1024)
#undef PAIR_EVAL_CASE
      default: fmx_dev_free(part); return fail(h, FMX_E_UNSUPPORTED, "num_factor > 1024 is not supported");
    }
    hipLaunchKernelGGL(k_pair_eval_final, dim3(1), dim3(64), 0, h->stream, part, nblk, part + 2 * nblk);
    er = hipGetLastError();
  }
  if (er == hipSuccess) er = hipEventRecord(h->ev1, h->stream);
  double res[2] = {0.0, 0.0};
  if (er == hipSuccess) er = hipMemcpyAsync(res, part + 2 * nblk, sizeof(res), hipMemcpyDeviceToHost, h->stream);
  if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  fmx_dev_free(part);
  HIPCHK(h, er);
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  out->accuracy = res[0] / (double)s.n_pairs;
  out->loss = res[1] / (double)s.n_pairs;
  out->device_seconds = ms * 1e-3;
  return FMX_OK;
}

}  // extern "C"
