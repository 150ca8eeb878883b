// fmx_sgd.hip -- C-ABI (include/fmx.h): the SGD family -- sequential / minibatch / hogwild epochs, the split step of
// the multi-GPU driver, the bias-lag bookkeeping, the (batch, feature) segment build, SGDA, and AdaGrad on
// the minibatch rule (fmx_adapt_*), FTRL-proximal with L1 on the same rule (fmx_ftrl_*) and the zero count of the tables.
#include "fmx_internal.h"
#include "fmx_online_kernels.h"
#include "fmx_seq_kernels.h"
#include "fmx_small_kernels.h"
#include "fmx_adapt_kernels.h"
#include "fmx_ftrl_kernels.h"
#include "fmx_weighted_kernels.h"

namespace {
// default micro-chunk of the bias recurrence.  The reference moves w0 after EVERY example (fm_sgd.h:34-37); summing the
// multipliers of a chunk and applying them at once is a batch step of size lr * chunk on a coordinate whose curvature is
// up to 1 (regression) or 1/4 (logistic) PER EXAMPLE, so lr * chunk * curvature must stay below 2 or the bias
// oscillates with growing amplitude (observed: classification, lr = 0.02, chunk = 1024 -> w0 = +-3..6, accuracy 0.50).
// Default: the largest power of two with lr * chunk * curvature <= 1, capped at FMX_W0_CHUNK_CAP.  The cap is what sets how
// closely the batch rule follows the reference's bias PATH (and through it the reference's predictions): at the bench shape the
// rule's bias ends 0.025 from the online loop's at chunk 256 and 0.0014 at chunk 32, so the cap went from
// 256 to 32 in round 5 -- the recurrence is solved parallel in time (k_scan_pit) at 40-80 us per 262 144 examples whatever the chunk; as a
// one-wavefront chain (k_scan1's sub-piece form, FMX_SCAN=serial) such chunks cost ~60 ns each.  An explicit w0_chunk is honoured.
uint32_t default_w0_chunk(const fmx_config& c) { return fmx_default_w0_chunk(c.learn_rate, c.task); }

// row slots (ZR) of the k_fused instance used for a slot: the smallest instance whose registers hold the longest row
template <int KP> constexpr bool fused_zr_ok(int zr) { return Map<KP>::VEC * zr <= 128; }
template <int KP> int fused_zr_select(uint32_t max_row) {
  constexpr int EPI = Map<KP>::EPI;
  const uint32_t need = (max_row + EPI - 1) / EPI;         // row slots per lane to keep a whole row in registers
  for (int zr : {8, 16, 32, 40, 64})                       // 40: Criteo-shaped rows (39 fields)
    if (fused_zr_ok<KP>(zr) && need <= (uint32_t)zr) return zr;
  return 8;                                                // rows too long for the register file: the kernel's two-pass branch
}
// longest row the selected instance keeps in registers (longer rows take its two-pass branch; FUSED_EXACT defers them)
template <int KP> uint32_t fused_row_cap_kp(uint32_t max_row) {
  return std::min<uint32_t>(64u, (uint32_t)fused_zr_select<KP>(max_row) * (uint32_t)Map<KP>::EPI);
}

template <int KP, int VAR>
int launch_fused_zr(fmx_handle h, const Slot& s, const Hyper& hy, uint64_t row0, uint32_t n_rows, hipStream_t st,
                    const double* w0_in, float* rest_out, const uint64_t* cmask = nullptr, float* S_out = nullptr,
                    float* mult_out = nullptr, uint32_t* handoff_err = nullptr, bool keep_wside = false, const WTrain wt = WTrain()) {
#define FMX_LAUNCH_ZR(ZRV)                                                                                  \
  if constexpr (fused_zr_ok<KP>(ZRV)) {                                                                     \
    FMX_LAUNCH_WAVES((k_fused<KP, ZRV, VAR>), n_rows, st, s.ent, s.row_ptr, s.target, row0,                 \
                     n_rows, h->tb, hy, w0_in, rest_out, cmask, S_out, mult_out, s.fixed_nnz, handoff_err,                  \
                     (const uint64_t*)(keep_wside ? s.lmask : nullptr), keep_wside ? s.wside : (float*)nullptr,             \
                     (const uint32_t*)s.ids, wt); }
  switch (fused_zr_select<KP>(s.max_row)) {
    case 8:  FMX_LAUNCH_ZR(8);  break;
    case 16: FMX_LAUNCH_ZR(16); break;
    case 32: FMX_LAUNCH_ZR(32); break;
    case 40: FMX_LAUNCH_ZR(40); break;
    case 64: FMX_LAUNCH_ZR(64); break;
  }
#undef FMX_LAUNCH_ZR
  return FMX_OK;
}

}  // namespace

// SHORT rows (a feature shard of P GPUs sees nnz / P entries per example): examples per wavefront of k_rowsums_multi / k_apply_multi --
// about 24 entries per 32-slot round (mean + 1.7 sigma of a shard's binomial row lengths stays inside one round); 0 = rows are long enough
// for the one-example-per-wavefront kernels (or KP < 64: several rows per wave-wide load, not built)
extern "C++" uint32_t multi_group_size(const Slot& s, int KP) {
  if (KP < 64 || KP > 256 || s.n_rows == 0) return 0;          // (beyond 256 factors the sums of a group of examples do not fit the LDS)
  const double avg = (double)s.nnz / (double)s.n_rows;
  if (avg > 12.0) return 0;
  static const double fill = []() { const char* e = getenv("FMX_MULTI_FILL"); const double f = e ? atof(e) : 0.0; return (f >= 8.0 && f <= 32.0) ? f : 24.0; }();
  const double g = avg > 0.0 ? fill / avg : (double)MULTI_GMAX;   // (FMX_MULTI_FILL: A/B knob for the probe, 8 .. 32)
  return (uint32_t)std::max(2.0, std::min((double)MULTI_GMAX, std::floor(g)));
}

extern "C" {

// ---------------------------------------------------------------------------------------------
// SGD
// ---------------------------------------------------------------------------------------------
uint32_t fmx_default_w0_chunk(double learn_rate, int task) {
  const double curv = (task == FMX_TASK_REGRESSION) ? 1.0 : 0.25;
  const double lim = (learn_rate > 0) ? 1.0 / (learn_rate * curv) : (double)FMX_W0_CHUNK_CAP;
  uint32_t chunk = 1;
  while (chunk < (uint32_t)FMX_W0_CHUNK_CAP && (double)(chunk * 2) <= lim) chunk *= 2;
  return chunk;
}
int fmx_partial_floats(fmx_handle h, uint32_t batch, uint64_t* n_floats) {
  if (!h || !n_floats) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_partial_floats"); if (_sr) return _sr; }
  *n_floats = (uint64_t)batch * (uint64_t)(h->KP + 1);
  return FMX_OK;
}

// partial buffer layout: [n_rows][KP] factor sums, then [n_rows] scalars
int fmx_sgd_partial(fmx_handle h, int slot, uint64_t row0, uint32_t n_rows, float* d_partial, void* stream) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_sgd_partial"); if (_sr) return _sr; }
  int rc = check_slot(h, slot, false);
  if (rc) return rc;
  rc = refuse_weighted(h, slot, "fmx_sgd_partial"); if (rc) return rc;
  const Slot& s = h->slots[slot];
  if (row0 + n_rows > s.n_rows) return fail(h, FMX_E_ARG, "fmx_sgd_partial: rows [%llu,+%u) outside slot (%u rows)",
                                            (unsigned long long)row0, n_rows, s.n_rows);
  if (!s.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "relations are not supported with SGD");   // fm_learn_sgd.h:61-63
  if (!d_partial) return fail(h, FMX_E_ARG, "fmx_sgd_partial: d_partial is NULL");
  if (n_rows == 0) return FMX_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  float* S = d_partial;
  float* c = d_partial + (size_t)n_rows * h->KP;
  return sgd_partial_rows(h, s, row0, n_rows, S, c, st);
}

// a run of rows of a batch into the batch's partial buffer (S: [batch rows][KP], c: [batch rows]) -- the chunked exchange of
// fmx_group_sgd_epoch enqueues the all-reduce of one run while the next one is being summed
extern "C++" int sgd_partial_rows(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n_rows, float* S, float* c, hipStream_t st,
                                  const CompactState* snap) {
  if (n_rows == 0) return FMX_OK;
  if (snap) {
    if (snap->dir && snap->format == FMX_COMPACT_INT8) { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, true, false, RowsI8P>), n_rows, st, s.ent, s.row_ptr, row0, n_rows, compact_rows8_p(*snap), h->cfg.k1, S, c)); }
    else if (snap->dir) { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, true, false, RowsBf16P>), n_rows, st, s.ent, s.row_ptr, row0, n_rows, compact_rows_p(h, *snap), h->cfg.k1, S, c)); }
    else if (snap->format == FMX_COMPACT_INT8) { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, true, false, RowsI8>), n_rows, st, s.ent, s.row_ptr, row0, n_rows, compact_rows8(*snap), h->cfg.k1, S, c)); }
    else { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, true, false, RowsBf16>), n_rows, st, s.ent, s.row_ptr, row0, n_rows, compact_rows(h, *snap), h->cfg.k1, S, c)); }
    HIPCHK(h, hipGetLastError());
    return FMX_OK;
  }
  if (const uint32_t G = multi_group_size(s, h->KP)) {          // short rows: several examples per wavefront
    KP_SWITCH(h->KP, { if constexpr (KP >= 64 && KP <= 256) { FMX_LAUNCH_WAVES((k_rowsums_multi<KP, true, false>), ((uint64_t)n_rows + G - 1) / G, st,
                                                                  s.ent, s.row_ptr, row0, n_rows, h->tb, h->cfg.k1, S, c, G); } });
    HIPCHK(h, hipGetLastError());
    return FMX_OK;
  }
  KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, true, false>), n_rows, st, s.ent, s.row_ptr, row0, n_rows, RowsF32{h->tb}, h->cfg.k1, S, c));
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// the batch an epoch of the MINIBATCH rule runs with on this slot (fmx_sgd_opts::batch): the rows' collision mass -- summed over
// the feature shards when the handle is one -- and the stability cut of the default
extern "C++" int sgd_resolve_batch(fmx_handle h, Slot& s, const fmx_sgd_opts* opts, fmx_batch_info* bi) {
  const int slot = (int)(&s - h->slots);
  double C = 0.0;
  if (h->group && !h->owns_group && h->group->hs.size() > 1) {          // one process, several shards: their shares add up
    for (fmx_handle m : h->group->hs) {
      if (!m) return fail(h, FMX_E_STATE, "a member of the group was destroyed");
      int rc = ensure_coll_mass(m, m->slots[slot]);
      if (rc) { h->err = m->err; return rc; }
      C += m->slots[slot].coll_mass;
    }
  } else {
    int rc = ensure_coll_mass(h, s);
    if (rc) return rc;
    C = s.coll_mass;
    if (h->comm && h->cfg.shard_world > 1) {                 // one process per GPU: a collective on EVERY call (include/fmx.h) -- a per-rank
      rc = comm_sum_double(h, &C);                            // cache made the decision to enter it per-rank too: a rank that re-uploaded its
      if (rc) return rc;                                      // slot entered alone and the job hung (round-4 advisor).  8 bytes per epoch.
      s.coll_mass_world = C;
    }
  }
  resolve_batch(h->cfg, C, opts ? opts->batch : 0u, FMX_DEFAULT_BATCH, 1.0, bi);
  return FMX_OK;
}

int fmx_sgd_batch_info(fmx_handle h, int slot, const fmx_sgd_opts* opts, fmx_batch_info* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_sgd_batch_info"); if (_sr) return _sr; }
  int rc = check_slot(h, slot, false);
  if (rc) return rc;
  if (!out) return fail(h, FMX_E_ARG, "fmx_sgd_batch_info: out is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  return sgd_resolve_batch(h, h->slots[slot], opts, out);
}

// builds the (batch, feature) segments of a slot for batch size B (device radix sort; once per data set).
// Round 6: ONE scratch allocation (fmx_dev_alloc: built from <= 1 GiB chunks, see fmx_internal.h -- ten plain allocations of > 1 GiB were 2.4 s
// of a 2.46 s preparation), the temporary-storage sizes of the three hipCUB calls asked for once, the counts read back ONCE, every per-batch
// table (first segment / first deferred segment / first entry of a batch) computed on the device and read back together: two host
// synchronisations instead of seven, no copy of row_ptr to the host.  FMX_TRACE_SETUP=1 prints where the time goes.
extern "C++" int ensure_segments(fmx_handle h, Slot& s, uint32_t B) {
  if (s.seg_B == B && s.t_ent) return FMX_OK;
  if (&s >= h->slots && &s < h->slots + FMX_MAX_SLOTS) {          // (the rows of a kept `-relation` block are bucketed by their own session)
    int _rc = slot_in_session(h, (int)(&s - h->slots), "re-bucketing the rows for another batch size"); if (_rc) return _rc;
  }
  free_segments(s);
  const auto t_setup0 = std::chrono::steady_clock::now();
  static const bool trace = getenv("FMX_TRACE_SETUP") != nullptr;
  auto tp = [&](const char* what) { if (trace) { (void)hipStreamSynchronize(h->stream); fprintf(stderr, "[fmx setup] segments %-22s %8.3f ms\n", what,
                                     1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_setup0).count()); } };
  struct Acc { fmx_handle h; std::chrono::steady_clock::time_point t0;
               ~Acc() { h->setup_acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } } acc_{h, t_setup0};
  const uint64_t nnz = s.nnz;
  const uint32_t n_batches = (s.n_rows + B - 1) / B;
  if (nnz >= (1ull << 31)) return fail(h, FMX_E_UNSUPPORTED, "segmented apply: nnz >= 2^31 in one slot (split the data set)");
  hipStream_t st = h->stream;
  uint32_t cap = 64;
  KP_SWITCH(h->KP, cap = fused_row_cap_kp<KP>(s.max_row));
  uint32_t fbits = 1; while (fbits < 32 && (1ull << fbits) < std::max<uint64_t>(h->n_local, 2)) fbits++;   // bits of a local feature id
  int bits_batch = 1; while ((1ull << bits_batch) < n_batches) bits_batch++;
  char* scratch = nullptr;
  int rc = FMX_OK;
  const size_t cnt = (size_t)std::max<uint64_t>(nnz, 1);
  const size_t nb1 = (size_t)n_batches + 1;
#define SEG_CHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
    rc = fail(h, FMX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); goto done; } } while (0)
  {
    // temporary storage of the three hipCUB calls (a size query touches no memory)
    size_t tmp_sort = 0, tmp_scan = 0, tmp_xscan = 0;
    SEG_CHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                               (int)cnt, 0, (int)fbits + bits_batch, st));
    SEG_CHK(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_scan, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)cnt, st));
    SEG_CHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_xscan, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)cnt, st));
    const size_t tmp_bytes = std::max<size_t>(std::max(tmp_sort, std::max(tmp_scan, tmp_xscan)), 256);
    // scratch layout (256-byte aligned pieces): keys_a | keys_b | vals_a | flags | pos | cflag | cpos | counts | hipCUB temp
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t off = 0;
    const size_t o_ka = off; off += al(cnt * 8);
    const size_t o_kb = off; off += al(cnt * 8);
    const size_t o_va = off; off += al(cnt * 8);
    const size_t o_fl = off; off += al(cnt * 4);
    const size_t o_po = off; off += al(cnt * 4);
    const size_t o_cf = off; off += al(cnt * 4);
    const size_t o_cp = off; off += al(cnt * 4);
    const size_t o_ct = off; off += 256;
    const size_t o_tmp = off; off += al(tmp_bytes);
    SEG_CHK(fmx_dev_alloc(&scratch, off));
    uint64_t* keys_a = (uint64_t*)(scratch + o_ka); uint64_t* keys_b = (uint64_t*)(scratch + o_kb); uint64_t* vals_a = (uint64_t*)(scratch + o_va);
    uint32_t* flags = (uint32_t*)(scratch + o_fl); uint32_t* pos = (uint32_t*)(scratch + o_po);
    uint32_t* cflag = (uint32_t*)(scratch + o_cf); uint32_t* cpos = (uint32_t*)(scratch + o_cp);
    uint32_t* d_counts = (uint32_t*)(scratch + o_ct);            // {segments, deferred segments, longest segment, -}
    void* tmp = scratch + o_tmp;
    uint64_t* vals_b = nullptr;                                    // the sort's output payload IS t_ent (payload layout == TEntry): allocated on its own, kept
    SEG_CHK(fmx_dev_alloc(&vals_b, cnt * 8));
    s.t_ent = reinterpret_cast<TEntry*>(vals_b);
    SEG_CHK(fmx_dev_alloc(&s.cmask, (size_t)std::max<uint32_t>(s.n_rows, 1) * 8));
    SEG_CHK(fmx_dev_alloc(&s.d_batch_seg, nb1 * 4));
    SEG_CHK(fmx_dev_alloc(&s.d_cbatch, nb1 * 4));
    SEG_CHK(fmx_dev_alloc(&s.d_batch_base, nb1 * 8));
    tp("allocations");
    hipLaunchKernelGGL(k_seg_slow_rows, dim3(std::min<uint32_t>((s.n_rows + 255) / 256, 2048)), dim3(256), 0, st, s.row_ptr, s.n_rows, cap, s.cmask);
    s.fused_cap = cap;
    SEG_CHK(hipMemsetAsync(d_counts, 0, 16, st));
    if (nnz) {
      hipLaunchKernelGGL(k_seg_keys, dim3(wave_grid(s.n_rows)), dim3(256), 0, st, s.ent, s.row_ptr, s.n_rows, B, fbits, keys_a, vals_a, d_counts + 3);
      size_t tb_ = tmp_bytes;
      SEG_CHK(hipcub::DeviceRadixSort::SortPairs(tmp, tb_, keys_a, keys_b, vals_a, vals_b, (int)nnz, 0, (int)fbits + bits_batch, st));
      hipLaunchKernelGGL(k_seg_heads, dim3(2048), dim3(256), 0, st, keys_b, nnz, flags);
      tp("keys + sort + heads");
      tb_ = tmp_bytes;
      SEG_CHK(hipcub::DeviceScan::InclusiveSum(tmp, tb_, flags, pos, (int)nnz, st));
      // per-batch tables on the device (kept: the persistent small-batch kernel and the group driver's captured graphs read them there)
      hipLaunchKernelGGL(k_seg_batches, dim3((n_batches + 256) / 256), dim3(256), 0, st, pos, nnz, s.row_ptr, s.n_rows, B, n_batches, s.d_batch_seg, s.d_batch_base);
      // longest segment (fmx_epoch_stats::max_feature_count); keys_a is free after the sort: head[nseg + 1] <= 8 bytes per entry
      uint32_t* head = reinterpret_cast<uint32_t*>(keys_a);
      hipLaunchKernelGGL(k_seg_head_pos, dim3(2048), dim3(256), 0, st, flags, pos, nnz, head);
      hipLaunchKernelGGL(k_seg_max_count, dim3(2048), dim3(256), 0, st, head, pos, nnz, d_counts + 2);
      // what the one-pass kernel (FMX_APPLY_FUSED) must leave to k_apply_seg: features occurring more than once in their batch + rows too
      // long for its registers
      hipLaunchKernelGGL(k_seg_mark, dim3(2048), dim3(256), 0, st, keys_b, reinterpret_cast<const TEntry*>(vals_b), head, pos, nnz,
                         s.ent, s.row_ptr, B, fbits, cap, (uint32_t)(s.max_row > cap ? 1u : 0u), s.cmask, cflag);
      SEG_CHK(hipGetLastError());
      tb_ = tmp_bytes;
      SEG_CHK(hipcub::DeviceScan::ExclusiveSum(tmp, tb_, cflag, cpos, (int)nnz, st));   // (over nnz >= nseg elements: the tail is never read)
      hipLaunchKernelGGL(k_seg_counts, dim3(1), dim3(64), 0, st, pos, nnz, cpos, cflag, d_counts + 2, d_counts);
      uint32_t counts[4] = {0, 0, 0, 0};
      SEG_CHK(hipMemcpyAsync(counts, d_counts, 16, hipMemcpyDeviceToHost, st));
      SEG_CHK(hipStreamSynchronize(st));                         // host synchronisation 1 of 2: the sizes of the slot's arrays
      tp("scan + mark + counts");
      const uint32_t nseg = counts[0];
      s.nseg = nseg; s.ncseg = counts[1]; s.max_seg_count = counts[2]; s.all_ones = counts[3] == 0u;
      SEG_CHK(fmx_dev_alloc(&s.seg_feat, (size_t)std::max<uint32_t>(nseg, 1) * 4));
      SEG_CHK(fmx_dev_alloc(&s.seg_rel, (size_t)std::max<uint32_t>(nseg, 1) * 4));
      SEG_CHK(fmx_dev_alloc(&s.cseg, (size_t)std::max<uint32_t>(s.ncseg, 1) * 4));
      SEG_CHK(fmx_dev_alloc(&s.cdesc, (size_t)std::max<uint32_t>(s.ncseg, 1) * sizeof(CDesc)));
      hipLaunchKernelGGL(k_seg_fill, dim3(2048), dim3(256), 0, st, keys_b, flags, pos, nnz, s.row_ptr, B, fbits, s.seg_feat, s.seg_rel);
      hipLaunchKernelGGL(k_seg_compact, dim3(2048), dim3(256), 0, st, keys_b, head, cflag, cpos, nseg, s.d_batch_seg, s.cseg,
                         s.seg_feat, s.seg_rel, s.row_ptr, s.n_rows, B, fbits, s.cdesc, reinterpret_cast<const TEntry*>(vals_b));
      hipLaunchKernelGGL(k_seg_cbatch, dim3((n_batches + 256) / 256), dim3(256), 0, st, cpos, cflag, nseg, s.d_batch_seg, n_batches, s.d_cbatch);
      SEG_CHK(hipGetLastError());
    } else {
      s.nseg = 0; s.ncseg = 0; s.max_seg_count = 0; s.all_ones = false;
      SEG_CHK(hipMemsetAsync(s.d_batch_seg, 0, nb1 * 4, st));
      SEG_CHK(hipMemsetAsync(s.d_cbatch, 0, nb1 * 4, st));
      SEG_CHK(hipMemsetAsync(s.d_batch_base, 0, nb1 * 8, st));
      SEG_CHK(fmx_dev_alloc(&s.seg_feat, 4)); SEG_CHK(fmx_dev_alloc(&s.seg_rel, 4));
      SEG_CHK(fmx_dev_alloc(&s.cseg, 4));
      SEG_CHK(fmx_dev_alloc(&s.cdesc, sizeof(CDesc)));
    }
    s.batch_seg.resize(nb1); s.cbatch.resize(nb1); s.batch_base.resize(nb1);
    SEG_CHK(hipMemcpyAsync(s.batch_seg.data(), s.d_batch_seg, nb1 * 4, hipMemcpyDeviceToHost, st));
    SEG_CHK(hipMemcpyAsync(s.cbatch.data(), s.d_cbatch, nb1 * 4, hipMemcpyDeviceToHost, st));
    SEG_CHK(hipMemcpyAsync(s.batch_base.data(), s.d_batch_base, nb1 * 8, hipMemcpyDeviceToHost, st));
    SEG_CHK(hipStreamSynchronize(st));                           // host synchronisation 2 of 2: the per-batch tables
    tp("fill + compact + tables");
    s.seg_B = B;
  }
done:
#undef SEG_CHK
  if (scratch) fmx_dev_free(scratch);
  tp("frees");
  if (rc) free_segments(s);
  return rc;
}

// the device's error word (h->handoff_err), read with the streams drained: copies it to the host, clears the bits of `mask` on the device
// where one of them is set, and returns those
static int take_error_bits(fmx_handle h, uint32_t mask, uint32_t* bits) {
  uint32_t e = 0;
  HIPCHK(h, hipMemcpy(&e, h->handoff_err, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (e & mask) {
    const uint32_t rest_bits = e & ~mask;
    (void)hipMemcpy(h->handoff_err, &rest_bits, sizeof(uint32_t), hipMemcpyHostToDevice);
  }
  *bits = e & mask;
  return FMX_OK;
}
// ... after launches of k_scan_pit.  Bit 4 = a grid-wide exchange ran
// into its bound and one workgroup evaluated the batch's chain serially instead (fmx_kernels.h): the numbers are the rule's, so this is
// not a failure -- the epoch reports FMX_STAT_SCAN_FALLBACK and the handle takes the one-wavefront chain from now on.  Only bit 4 is
// cleared here (the hand-off's bits 1 and 2 belong to the epoch's own check).
extern "C++" int scan_error_check(fmx_handle h) {
  if (!h->pit_used) return FMX_OK;
  h->pit_used = false;
  uint32_t bits = 0;
  int rc = take_error_bits(h, 4u, &bits);
  if (rc) return rc;
  if (bits) {
    h->scan_pit = false;
    h->run_status |= FMX_STAT_SCAN_FALLBACK;
  }
  return FMX_OK;
}

// do the handle's two streams run concurrently?  (k_concurrency_probe, once per handle: ~50 us when they do, ~40 ms when they do not)
extern "C++" bool streams_concurrent(fmx_handle h) {
  if (h->concurrent >= 0) return h->concurrent != 0;
  h->concurrent = 0;
  if (!h->probe_flags && fmx_dev_alloc(&h->probe_flags, 4 * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); return false; }
  unsigned res[4] = {0, 0, 0, 0};
  hipError_t e = hipMemsetAsync(h->probe_flags, 0, 4 * sizeof(unsigned), h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream2);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_concurrency_probe, dim3(1), dim3(64), 0, h->stream2, h->probe_flags, 1u);
    hipLaunchKernelGGL(k_concurrency_probe, dim3(1), dim3(64), 0, h->stream, h->probe_flags, 0u);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream2);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = hipMemcpy(res, h->probe_flags, sizeof(res), hipMemcpyDeviceToHost);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  h->concurrent = (res[2] == 1u && res[3] == 1u) ? 1 : 0;
  return h->concurrent != 0;
}

// a kernel that asks for more dynamic LDS than the default limit: that limit is per-device state, raised once per handle and kernel
static int raise_lds(fmx_handle h, const void* kf, size_t bytes) {
  if (h->lds_raised.count(kf)) return FMX_OK;
  HIPCHK(h, hipFuncSetAttribute((const void*)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  h->lds_raised.insert(kf);
  return FMX_OK;
}
#define FMX_RAISE_LDS(kf, bytes) do { int _rc = raise_lds(h, (const void*)(kf), (bytes)); if (_rc) return _rc; } while (0)

// workgroups of k_scan_pit that must be resident TOGETHER on the handle's device: every shard of a loopback group runs the whole
// recurrence itself, on the same device (round-5 advisor: 16 loopback shards x 32 workgroups on 256 CUs waited for each other)
static uint32_t pit_concurrent_kernels(fmx_handle h) {
  uint32_t n = 1;
  if (h->group && h->group->hs.size() > 1) {
    n = 0;
    for (fmx_handle m : h->group->hs) if (m && m->device == h->device) n++;
    if (n == 0) n = 1;
  }
  return n;
}

static int launch_scan(fmx_handle h, const float* rest, const float* target, uint32_t n_rows, uint32_t chunk,
                       const Hyper& hy, float* mult, hipStream_t st, const double* w0_in = nullptr, double* w0_out = nullptr,
                       const Handoff hw = Handoff{nullptr, 0ull, nullptr}, bool short_pit = false) {
  if (hy.k0) {
    const double* wi = w0_in ? w0_in : h->w0;
    double* wo = w0_out ? w0_out : h->w0;
    // round 5: the recurrence solved parallel in time (k_scan_pit: Newton on the whole path, affine prefix scans; up to 64 workgroups) for
    // micro-chunks that are powers of two up to 1024 on batches of 4097 .. 262 144 examples -- every default.  Same result as the chain to
    // fp32 rounding; 40-80 us per 262 144 examples whatever the micro-chunk where the chain takes 0.18 ms (256) .. 0.5 ms (32).
    // (the arrival counters of its exchanges are zeroed on the launch's own stream, in front of it)
    if (h->scan_pit && (n_rows > 4096u || (short_pit && n_rows >= 256u)) && chunk <= PIT_MAX_CHUNK && (chunk & (chunk - 1u)) == 0u) {
      // every workgroup of the launch spins on a grid-wide arrival counter: all of them must fit the device TOGETHER -- next to the same
      // kernel of the other shards on this device.  112 KiB of LDS per workgroup = one per CU (asked once per handle).
      if (h->pit_occ < 0) {
        int per_cu = 0;
        auto kf = k_scan_pit<false, 1>;
        (void)hipFuncSetAttribute((const void*)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PIT_LDS_BYTES);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kf, 256, PIT_LDS_BYTES) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
        h->pit_occ = per_cu * h->num_cu;
      }
      const uint32_t piece_rows = PIT_MAX_ROWS;
      const uint32_t nwg_max = (std::min(n_rows, piece_rows) + pit_seg(chunk) - 1) / pit_seg(chunk);
      static const bool trace_pit = getenv("FMX_TRACE_PIT") != nullptr;
      if (trace_pit) fprintf(stderr, "[fmx pit] rows %u chunk %u: %u workgroups x %u kernels, device holds %d\n", n_rows, chunk, nwg_max, pit_concurrent_kernels(h), h->pit_occ);
      if ((uint64_t)nwg_max * pit_concurrent_kernels(h) <= (uint64_t)std::max(h->pit_occ, 0)) {
        // a batch longer than PIT_MAX_ROWS (an explicit batch, a HOGWILD macro-batch): pieces of PIT_MAX_ROWS examples, the bias handed from
        // piece to piece on the launch's stream (round-5 advisor: such batches silently took the one-wavefront chain, 8x the steps at the new
        // default micro-chunk); only the first piece waits for the hand-off counter, only the last one publishes
        const uint32_t n_pieces = (n_rows + piece_rows - 1) / piece_rows;
        if (n_pieces > 1 && !h->pit_tmp) HIPCHK(h, fmx_dev_alloc(&h->pit_tmp, 64 * sizeof(double)));
        if (n_pieces <= 64) {
          const PitSync ps{h->pit_ctr, h->pit_slots, h->handoff_err, h->pit_spins};   // (FMX_DEBUG_PIT_SPINS=0 at fmx_create: every exchange gives up at once -- the test of the fall-back)
          for (uint32_t pc = 0; pc < n_pieces; pc++) {
            const uint32_t r0 = pc * piece_rows, rn = std::min(piece_rows, n_rows - r0);
            const uint32_t nwg = (rn + pit_seg(chunk) - 1) / pit_seg(chunk);
            const double* pin = pc == 0 ? wi : h->pit_tmp + (pc - 1);
            double* pout = pc + 1 == n_pieces ? wo : h->pit_tmp + pc;
            Handoff ph{nullptr, 0ull, nullptr};                    // a piece in the middle: plain load, plain store, stream order
            if (hw.ctr) {
              if (pc == 0) ph = hw;                                // waits for the batch's rest[] (and stores with the hand-off store: harmless for pit_tmp)
              else if (pc + 1 == n_pieces) ph = Handoff{hw.ctr, 0ull, hw.err};   // publishes; nothing left to wait for
            }
            HIPCHK(h, hipMemsetAsync(h->pit_ctr, 0, (PIT_MAX_IT + 1) * sizeof(unsigned long long), st));
            float* mp = mult ? mult + r0 : nullptr;
#define FMX_PIT(WM, TK) do { auto kf = k_scan_pit<WM, TK>;                                                                       \
            FMX_RAISE_LDS(kf, PIT_LDS_BYTES);                                                                                      \
            hipLaunchKernelGGL(kf, dim3(nwg), dim3(256), PIT_LDS_BYTES, st, rest + r0, target + r0, rn, chunk, hy, pin, pout, mp, ph, ps); } while (0)
            if (hy.task == 0) { if (mult) FMX_PIT(true, 0); else FMX_PIT(false, 0); }
            else              { if (mult) FMX_PIT(true, 1); else FMX_PIT(false, 1); }
#undef FMX_PIT
          }
          h->pit_used = true;
          h->run_status |= FMX_STAT_SCAN_PIT;
          HIPCHK(h, hipGetLastError());
          return FMX_OK;
        }
      }
    }
    h->run_status |= FMX_STAT_SCAN_SERIAL;
    // micro-chunks that are multiples of 256 examples: k_scan1 (one wavefront on the chain, four contiguous examples per lane, a 128 KiB
    // tile pipeline fed by the workgroup's four wavefronts); else, and for
    // batches of a few thousand rows (the 128 KiB-LDS workgroup costs more to place than the recurrence takes): one plain wavefront
    // ... or, round 5, the sub-piece form of the same kernel for micro-chunks of 16 / 32 / 64 / 128 examples (the default is now below 256)
    const bool sub = chunk == 16u || chunk == 32u || chunk == 64u || chunk == 128u;
    const bool tiled = n_rows > 8192u && ((chunk % 256u) == 0 || sub);
#define FMX_SCAN1(WM, TK, C256) do { auto kf = k_scan1<WM, TK, C256>;                                                              \
      FMX_RAISE_LDS(kf, SCAN4_LDS_BYTES);                                                                                          \
      hipLaunchKernelGGL(kf, dim3(1), dim3(256), SCAN4_LDS_BYTES, st, rest, target, n_rows, chunk, hy, wi, wo, mult, hw); } while (0)
#define FMX_SCAN(WM, TK) do { \
      if (tiled && chunk == 256u) FMX_SCAN1(WM, TK, 256); \
      else if (tiled && chunk == 128u) FMX_SCAN1(WM, TK, 128); \
      else if (tiled && chunk == 64u)  FMX_SCAN1(WM, TK, 64); \
      else if (tiled && chunk == 32u)  FMX_SCAN1(WM, TK, 32); \
      else if (tiled && chunk == 16u)  FMX_SCAN1(WM, TK, 16); \
      else if (tiled)             FMX_SCAN1(WM, TK, 0); \
      else                        hipLaunchKernelGGL((k_scan<WM, TK>), dim3(1), dim3(64), 0, st, rest, target, n_rows, chunk, hy, wi, wo, mult, hw); } while (0)
    if (hy.task == 0) { if (mult) FMX_SCAN(true, 0); else FMX_SCAN(false, 0); }
    else              { if (mult) FMX_SCAN(true, 1); else FMX_SCAN(false, 1); }
#undef FMX_SCAN
#undef FMX_SCAN1
  } else if (mult) {
    hipLaunchKernelGGL(k_mult, dim3(std::min<uint32_t>((n_rows + 255) / 256, 2048)), dim3(256), 0, st, rest, target, n_rows, hy,
                       (const double*)nullptr, mult);
  }
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// ---- FMX_FLAG_BIAS_LAG (split step): the w0 recurrence of batch b runs on stream2 while the main stream goes on ----
// Depth d = opts->bias_lag (>= 1): the multipliers of batch b use the bias as it was after the recurrence of batch b - d.
// Ring of R = d + 1 bias slots: slot (b + 1) % R holds the bias after batch b (all slots start as the current bias);
// the recurrence of batch b reads slot b % R and writes slot (b + 1) % R; the multipliers of batch b read slot
// (b - d + 1) % R, which is rewritten next by the recurrence of batch b + 1 -- enqueued after them.  d + 1 rest buffers.
extern "C++" int lag_flush(fmx_handle h) {                      // make h->w0 the current bias again
  LagState& L = h->lag;
  if (!L.active) return FMX_OK;
  if (L.in_stream) { HIPCHK(h, hipStreamSynchronize(L.in_stream)); L.in_stream = nullptr; }
  HIPCHK(h, hipStreamSynchronize(h->stream2));
  // on the handle's OWN stream, then drained: the streams are non-blocking, so a device-to-device hipMemcpy (null stream; it may return before
  // the copy has run) is not ordered against what the next epoch enqueues on h->stream -- its ring of bias slots was then, once in a few
  // thousand epochs, initialised from the bias of BEFORE this epoch (round 6: tests/test_gpu_fuzz.py seed 16 ended at w0 = -0.0076 instead of
  // -0.0163: exactly the second epoch started from the first epoch's start value)
  HIPCHK(h, hipMemcpyAsync(h->w0, h->w0_pp + (L.step % (L.depth + 1)), sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  L.active = false; L.step = 0;
  return scan_error_check(h);                                 // (callers that drive fmx_sgd_partial / _finish themselves and then read parameters)
}
// ---- the plan of ONE step of the split rule: every route decision, made once (fmx_sgd_finish per step, epoch_split per epoch) and read,
// not derived again, by lag_prepare and sgd_finish_impl ----
struct StepPlan {
  bool     lag;         // FMX_FLAG_BIAS_LAG: multipliers from the bias of `depth` batches ago, the recurrence off the critical path
  bool     short_rows;  // short rows (a feature shard), library's choice of the update: k_apply_multi (example-major, several examples per wavefront) + the deferred list
  bool     from_sums;   // lag && short_rows on exchanged sums: rest_e and the multipliers come out of the update kernel (no k_rest_from_partial, no k_mult)
  bool     in_stream;   // ... of a small batch: the recurrence rides in the launch of the deferred features -- no side stream, no events
  int      apply;       // fmx_sgd_opts::apply as given
  int64_t  seg_batch;   // the rows are exactly this batch of the slot's segment structure; -1: per-example apply only
  uint32_t chunk, depth;
};
// has_rest: the caller computed rest[] itself (k_rowsums of an unsharded epoch leaves it); else it holds the sums of an exchange
static StepPlan step_plan(fmx_handle h, const Slot& s, const fmx_sgd_opts* opts, int64_t seg_batch, bool has_rest) {
  StepPlan p;
  p.apply = opts ? opts->apply : FMX_APPLY_DEFAULT; p.seg_batch = seg_batch;
  p.chunk = (opts && opts->w0_chunk) ? opts->w0_chunk : default_w0_chunk(h->cfg);
  p.depth = (opts && opts->bias_lag) ? opts->bias_lag : 1u;
  p.lag = opts && (opts->flags & FMX_FLAG_BIAS_LAG);
  p.short_rows = (p.apply == FMX_APPLY_DEFAULT || p.apply == FMX_APPLY_FUSED) && seg_batch >= 0 && s.cmask && !s.cbatch.empty() && multi_group_size(s, h->KP) != 0;
  p.from_sums = p.lag && p.short_rows && !has_rest;
  p.in_stream = p.from_sums && sgd_in_stream_batch(opts->batch, opts->flags);
  return p;
}
// call BEFORE producing the rest buffer of this step on `st`; returns which of the d + 1 rest buffers to use
static int lag_prepare(fmx_handle h, hipStream_t st, const StepPlan& plan, int* slot) {
  LagState& L = h->lag;
  const uint32_t depth = plan.depth;
  if (!L.ev_rest) {
    HIPCHK(h, hipEventCreateWithFlags(&L.ev_rest, hipEventDisableTiming));
    for (auto& e : L.ev_scan) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  if (L.active && L.depth != depth) { int rc = lag_flush(h); if (rc) return rc; }
  if (!L.active) {
    L.depth = depth;
    for (uint32_t r = 0; r <= depth; r++) HIPCHK(h, hipMemcpyAsync(h->w0_pp + r, h->w0, sizeof(double), hipMemcpyDeviceToDevice, st));
    L.active = true; L.step = 0;
  } else if (L.step > depth && !plan.in_stream) {
    HIPCHK(h, hipStreamWaitEvent(st, L.ev_scan[(L.step - depth - 1) % LagState::RING], 0));   // recurrence (step - d - 1) is done with this rest buffer
  }
  *slot = (int)(L.step % (depth + 1));
  return FMX_OK;
}
// call AFTER `rest` is complete on `st`: starts the recurrence on the side stream and leaves the multipliers of
// this batch (lagged bias) in h->mult on `st`
// the three pieces of a lagged step: `st` waits for the recurrence whose bias this batch's multipliers use; where that bias lives; the
// recurrence of THIS batch goes to the side stream behind whatever produced rest[] on `st`
static int lag_wait_bias(fmx_handle h, const Hyper& hy, hipStream_t st) {
  LagState& L = h->lag;
  if (hy.k0 && L.step >= L.depth) HIPCHK(h, hipStreamWaitEvent(st, L.ev_scan[(L.step - L.depth) % LagState::RING], 0));   // recurrence of batch b - d
  return FMX_OK;
}
static const double* lag_bias_slot(fmx_handle h) {
  const LagState& L = h->lag;
  const uint32_t R = L.depth + 1;
  return h->w0_pp + ((L.step + R - L.depth + 1) % R);
}
static int lag_start_scan(fmx_handle h, const float* rest, const float* target, uint32_t n_rows, uint32_t chunk, const Hyper& hy, hipStream_t st) {
  LagState& L = h->lag;
  const uint64_t b = L.step;
  const uint32_t R = L.depth + 1;
  if (hy.k0) {
    HIPCHK(h, hipEventRecord(L.ev_rest, st));
    HIPCHK(h, hipStreamWaitEvent(h->stream2, L.ev_rest, 0));
    int rc = launch_scan(h, rest, target, n_rows, chunk, hy, nullptr, h->stream2, h->w0_pp + (b % R), h->w0_pp + ((b + 1) % R)); if (rc) return rc;
    HIPCHK(h, hipEventRecord(L.ev_scan[b % LagState::RING], h->stream2));
  }
  return FMX_OK;
}
static int lag_step(fmx_handle h, const float* rest, const float* target, uint32_t n_rows, uint32_t chunk,
                    const Hyper& hy, hipStream_t st) {
  int rc = lag_start_scan(h, rest, target, n_rows, chunk, hy, st); if (rc) return rc;
  rc = lag_wait_bias(h, hy, st); if (rc) return rc;
  hipLaunchKernelGGL(k_mult, dim3(std::min<uint32_t>((n_rows + 255) / 256, 2048)), dim3(256), 0, st, rest, target, n_rows, hy,
                     lag_bias_slot(h), h->mult);
  HIPCHK(h, hipGetLastError());
  h->lag.step++;
  return FMX_OK;
}

// the deferred features of batch b of the slot's segment structure (ensure_segments): those that occur more than once in the batch,
// finished by their owners (k_apply_seg, k_apply_seg_scan, k_small_one) from the examples' factor sums S and multipliers
static SegWork seg_work(fmx_handle, const Slot& s, size_t b, const float* S, const float* mult) {
  const uint32_t c0 = s.cbatch[b], c1 = s.cbatch[b + 1], s0 = s.batch_seg[b], s1 = s.batch_seg[b + 1];
  const uint64_t base = s.batch_base[b];
  return SegWork{s.t_ent + base, s.seg_feat + s0, s.seg_rel + s0, s.cseg + c0, c1 - c0, s1 - s0, (uint32_t)(s.batch_base[b + 1] - base), S, mult,
                 s.cdesc + c0, nullptr, 0ull};
}
// ... and EVERY feature of the batch, one owner each (the dense pass of FMX_APPLY_SEGMENTED and of SGDA's batch form)
static SegWork seg_work_dense(fmx_handle, const Slot& s, size_t b, const float* S, const float* mult) {
  const uint32_t s0 = s.batch_seg[b], nseg = s.batch_seg[b + 1] - s0;
  const uint64_t base = s.batch_base[b];
  return SegWork{s.t_ent + base, s.seg_feat + s0, s.seg_rel + s0, nullptr, nseg, nseg, (uint32_t)(s.batch_base[b + 1] - base), S, mult, nullptr, nullptr, 0ull};
}
// the split step's deferred-feature pass (the only place it launches k_apply_seg<KP, 8, 16>)
static int launch_deferred(fmx_handle h, const Slot& s, const Hyper& hy, const float* S, size_t b, hipStream_t st) {
  const SegWork sw = seg_work(h, s, b, S, h->mult);
  if (sw.nseg) { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_apply_seg<KP, 8, 16>), ((uint64_t)sw.nseg + 15) / 16, st, sw, h->tb, hy)); }
  return FMX_OK;
}
// the short-row update over the batch-unique features.  fused: it derives rest_e (left in `rest` for the recurrence) and the multipliers
// (left in h->mult for the deferred list) from the exchanged sums S and cpart itself, with the bias in `bias`; else the multipliers are there
static int launch_apply_multi(fmx_handle h, const Slot& s, const Hyper& hy, uint64_t row0, uint32_t n_rows, bool fused, const double* bias,
                              const float* S, const float* cpart, float* rest, hipStream_t st) {
  const uint32_t G = multi_group_size(s, h->KP);
  KP_SWITCH(h->KP, { if constexpr (KP >= 64 && KP <= 256) { FMX_LAUNCH_WAVES((fused ? k_apply_multi<KP, true> : k_apply_multi<KP, false>), ((uint64_t)n_rows + G - 1) / G, st,
                                                                s.ent, s.row_ptr, s.target, row0, n_rows, h->tb, hy, bias, S, cpart, rest, h->mult, (const uint64_t*)s.cmask, G); } });
  return FMX_OK;
}
// step 3 where the rows are long enough for one example per wavefront: the update in the form fmx_sgd_opts::apply names
static int launch_apply(fmx_handle h, const Slot& s, const Hyper& hy, uint64_t row0, uint32_t n_rows, const float* S, const StepPlan& p,
                        hipStream_t st, hipEvent_t ev_a) {
  int apply = p.apply, rc = FMX_OK;
  // split step, library's choice (DEFAULT / FUSED): the features that occur once in the batch are written back example-major
  // (k_fused<FUSED_APPLY>: the wavefront holds S_e, no gather per occurrence), the others by their owner (k_apply_seg over the
  // batch's cseg list) -- the second half of what k_fused<EXACT> + k_apply_seg do in one pass on an unsharded handle.
  // FMX_APPLY_SEGMENTED keeps the dense owner-per-feature pass.
  // ... where rows are long enough to fill a wavefront's gather: measured per rank of a P-way sharded step (scripts/gpu_shard_probe.py,
  // dense vs example-major second pass): 32 entries per row +5 %, 16 entries -4 %, 8 entries -18 %, 4 entries -17 %.
  const bool masked = (apply == FMX_APPLY_DEFAULT || apply == FMX_APPLY_FUSED) && s.cmask && !s.cbatch.empty() && s.nnz >= (uint64_t)24 * s.n_rows;
  if (apply == FMX_APPLY_DEFAULT || apply == FMX_APPLY_FUSED) apply = FMX_APPLY_SEGMENTED;   // split step: same rule, two passes
  if (apply == FMX_APPLY_SEGMENTED && p.seg_batch < 0) return fail(h, FMX_E_STATE, "segmented apply needs batch-aligned rows");
  if (ev_a) HIPCHK(h, hipEventRecord(ev_a, st));
  if (apply == FMX_APPLY_SEGMENTED && masked) {
    KP_SWITCH(h->KP, rc = (launch_fused_zr<KP, FUSED_APPLY>(h, s, hy, row0, n_rows, st, (const double*)h->w0, nullptr,
                                                               (const uint64_t*)s.cmask, const_cast<float*>(S), h->mult)));
    if (rc) return rc;
    return launch_deferred(h, s, hy, S, (size_t)p.seg_batch, st);
  } else if (apply == FMX_APPLY_SEGMENTED) {
    const SegWork sw = seg_work_dense(h, s, (size_t)p.seg_batch, S, h->mult);
    if (sw.nseg) { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_apply_seg<KP, 8, 64>), ((uint64_t)sw.nseg + 63) / 64, st, sw, h->tb, hy)); }
  } else if (apply == FMX_APPLY_ATOMIC || apply == FMX_APPLY_STORE) {
    const bool atomic = apply == FMX_APPLY_ATOMIC;
    KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((atomic ? k_apply<KP, true> : k_apply<KP, false>), n_rows, st, s.ent, s.row_ptr, row0, n_rows, h->tb, hy, S, h->mult));
  } else {
    return fail(h, FMX_E_ARG, "unknown apply mode %d", apply);
  }
  return FMX_OK;
}
// steps 2 and 3 of the minibatch rule for rows [row0,row0+n_rows), as the plan says.  p.from_sums: `rest` has NOT been computed -- the
// short-row update derives it (and the multipliers) from S and cpart itself
static int sgd_finish_impl(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n_rows, const float* S, float* rest, const float* cpart,
                           const StepPlan& p, hipStream_t st, hipEvent_t ev_a, hipEvent_t ev_b) {
  const Hyper hy = make_hyper(h->cfg);
  const float* target = s.target + row0;
  int rc = FMX_OK;
  if (p.in_stream) {
    // small batches (what the stability cut leaves of rows with frequent features: BASELINE configs[2] runs 512 rows per batch): a batch is a
    // few microseconds of work and every call the host makes for it costs as much again -- the recurrence leaves the side stream and rides
    // in the launch of the deferred features (k_apply_seg_scan, as on an unsharded handle), no events: TWO launches per shard and batch.
    // Same rule, same ring of bias slots: what a batch reads does not depend on which stream wrote it.
    const LagState& L = h->lag;
    const uint32_t R = L.depth + 1;
    if (ev_a) HIPCHK(h, hipEventRecord(ev_a, st));
    rc = launch_apply_multi(h, s, hy, row0, n_rows, true, lag_bias_slot(h), S, cpart, rest, st); if (rc) return rc;
    const SegWork sw = seg_work(h, s, (size_t)p.seg_batch, S, h->mult);
    const ScanSmall sc{rest, target, h->w0_pp + (L.step % R), h->w0_pp + ((L.step + 1) % R), n_rows, p.chunk};
    KP_SWITCH(h->KP, hipLaunchKernelGGL((k_apply_seg_scan<KP, 8, 1>), dim3((sw.nseg + 3) / 4 + 1), dim3(256), 0, st, sw, h->tb, hy, sc));
    h->lag.step++; h->lag.in_stream = st;
    h->run_status |= FMX_STAT_SCAN_SERIAL;
  } else if (p.from_sums) {
    // fused short-row step (bias-lag schedule on a feature shard): [wait for the bias of batch b - d] -> k_apply_multi<FUSED> (rest, multipliers,
    // update of the batch-unique features) -> the recurrence of this batch starts on the side stream -> the deferred features
    rc = lag_wait_bias(h, hy, st); if (rc) return rc;
    if (ev_a) HIPCHK(h, hipEventRecord(ev_a, st));
    rc = launch_apply_multi(h, s, hy, row0, n_rows, true, lag_bias_slot(h), S, cpart, rest, st); if (rc) return rc;
    HIPCHK(h, hipGetLastError());
    rc = lag_start_scan(h, rest, target, n_rows, p.chunk, hy, st); if (rc) return rc;
    h->lag.step++;
    rc = launch_deferred(h, s, hy, S, (size_t)p.seg_batch, st); if (rc) return rc;
  } else {
    rc = p.lag ? lag_step(h, rest, target, n_rows, p.chunk, hy, st) : launch_scan(h, rest, target, n_rows, p.chunk, hy, h->mult, st);
    if (rc) return rc;
    if (p.short_rows) {                                         // (exact chunk coupling: the multipliers came out of the recurrence)
      if (ev_a) HIPCHK(h, hipEventRecord(ev_a, st));
      rc = launch_apply_multi(h, s, hy, row0, n_rows, false, (const double*)h->w0, S, nullptr, nullptr, st); if (rc) return rc;
      HIPCHK(h, hipGetLastError());
      rc = launch_deferred(h, s, hy, S, (size_t)p.seg_batch, st); if (rc) return rc;
    } else {
      rc = launch_apply(h, s, hy, row0, n_rows, S, p, st, ev_a); if (rc) return rc;
    }
  }
  if (ev_b) HIPCHK(h, hipEventRecord(ev_b, st));
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

int fmx_sgd_finish(fmx_handle h, int slot, uint64_t row0, uint32_t n_rows, const float* d_partial,
                   const fmx_sgd_opts* opts, void* stream) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_sgd_finish"); if (_sr) return _sr; }
  touch_w(h);
  int rc = check_slot(h, slot, true); if (rc) return rc;
  rc = refuse_weighted(h, slot, "fmx_sgd_finish"); if (rc) return rc;
  Slot& s = h->slots[slot];
  if (row0 + n_rows > s.n_rows) return fail(h, FMX_E_ARG, "fmx_sgd_finish: rows outside slot");
  if (!s.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "relations are not supported with SGD");   // fm_learn_sgd.h:61-63
  if (!d_partial) return fail(h, FMX_E_ARG, "fmx_sgd_finish: d_partial is NULL");
  if (((uintptr_t)d_partial & 15u) != 0) return fail(h, FMX_E_ARG, "fmx_sgd_finish: d_partial must be 16-byte aligned");
  if (n_rows == 0) return FMX_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const uint32_t Bcap = (opts && opts->batch) ? std::max(opts->batch, n_rows) : n_rows;
  const uint32_t lag_depth = (opts && opts->bias_lag) ? opts->bias_lag : 1u;   // (ahead of the plan: it sizes the scratch)
  if (lag_depth > 4) return fail(h, FMX_E_ARG, "bias_lag %u: at most 4 batches", lag_depth);
  rc = ensure_scratch(h, n_rows, (size_t)Bcap * (lag_depth + 1)); if (rc) return rc;
  const float* S = d_partial;
  const float* c = d_partial + (size_t)n_rows * h->KP;
  int64_t seg_batch = -1;
  const int apply = opts ? opts->apply : FMX_APPLY_DEFAULT;
  if (apply == FMX_APPLY_DEFAULT || apply == FMX_APPLY_SEGMENTED || apply == FMX_APPLY_FUSED) {
    // the driver walks the slot in batches of opts->batch rows (the last one may be short)
    const uint32_t B = (opts && opts->batch) ? opts->batch : n_rows;
    if (row0 % B != 0 || n_rows > B || n_rows != std::min<uint64_t>(B, s.n_rows - row0))
      return fail(h, FMX_E_ARG, "fmx_sgd_finish: rows [%llu,+%u) are not batch %u of the slot", (unsigned long long)row0, n_rows, B);
    rc = ensure_segments(h, h->slots[slot], B); if (rc) return rc;
    seg_batch = (int64_t)(row0 / B);
  }
  const StepPlan plan = step_plan(h, s, opts, seg_batch, false);   // every route decision of this step (the segments are there: it reads them)
  int rslot = 0;
  if (plan.lag) { rc = lag_prepare(h, st, plan, &rslot); if (rc) return rc; }
  else { rc = lag_flush(h); if (rc) return rc; }
  float* rest_buf = h->rest + (size_t)rslot * Bcap;
  if (!plan.from_sums) {
    KP_SWITCH(h->KP, hipLaunchKernelGGL((k_rest_from_partial<KP>), dim3(wave_grid((n_rows + Map<KP>::EPI - 1) / Map<KP>::EPI)),
                                          dim3(256), 0, st, S, c, n_rows, rest_buf));
    HIPCHK(h, hipGetLastError());
  }
  return sgd_finish_impl(h, s, row0, n_rows, S, rest_buf, c, plan, st, nullptr, nullptr);
}

int fmx_predict_finish(fmx_handle h, uint32_t n_rows, const float* d_partial, float* d_yhat, void* stream) {
  if (!h || !d_partial || !d_yhat) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_predict_finish"); if (_sr) return _sr; }
  if (((uintptr_t)d_partial & 15u) != 0) return fail(h, FMX_E_ARG, "fmx_predict_finish: d_partial must be 16-byte aligned");
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  if (n_rows == 0) return FMX_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  int rc = ensure_scratch(h, 0, n_rows);
  if (rc) return rc;
  const float* S = d_partial;
  const float* c = d_partial + (size_t)n_rows * h->KP;
  KP_SWITCH(h->KP, hipLaunchKernelGGL((k_rest_from_partial<KP>), dim3(wave_grid((n_rows + Map<KP>::EPI - 1) / Map<KP>::EPI)),
                                        dim3(256), 0, st, S, c, n_rows, h->rest));
  hipLaunchKernelGGL(k_yhat, dim3(std::min<uint32_t>((n_rows + 255) / 256, 2048)), dim3(256), 0, st,
                     h->rest, n_rows, h->cfg.k0, h->w0, d_yhat);
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// what an epoch driver reports back to fmx_sgd_epoch
// wtrain_fresh (in): the slot's training-side weight stream held the current w when fmx_sgd_epoch was entered; kept_wtrain (out): every
// batch of the epoch went through the kernel that maintains it
struct EpochCounts { uint64_t batches = 0, launches = 0, deferred = 0; bool kept_wside = false, wtrain_fresh = false, kept_wtrain = false; };

// MINIBATCH rule, FMX_APPLY_FUSED: per batch ONE pass over the examples (k_fused<FUSED_EXACT>: gather, predict, multiplier,
// write-back of every feature that occurs once in the batch) + k_apply_seg over the features that occur more than once.
// The multipliers of batch b use the bias as it was after the recurrence of batch b - d (d = opts->bias_lag >= 1; oracle
// fmo_sgd_epoch_minibatch_ex with bias_lag = d): the recurrence of batch b (k_scan, one workgroup) runs on the side stream
// under the launches of batches b+1 .. b+d-1 and only the launch of batch b+d waits for it.
// Three schedules of a batch (fused_batch_*), over what they share:
struct FusedEpoch {
  fmx_handle h; Slot* s; Hyper hy;
  uint32_t B, Bc, d, chunk; uint64_t n_batch;   // batch, min(batch, rows), bias lag, micro-chunk of the recurrence, batches of the epoch
  bool keep, handoff;             // the slot's weight side stream is kept (FMX_FLAG_KEEP_WSIDE); side stream: device-side hand-off (else events)
  WTrain wt;                      // the slot's training-side weight stream (w == nullptr: none; read: it holds the current w)
  double* W; unsigned long long hbase;   // hand-off: bias slots W[0 .. n_batch], the completion counter's value before this epoch
  int szr, small_cap;             // one launch: row slots of the k_small_one instance; workgroups of it the device holds (0: not asked yet)
  unsigned long long* small_trace;
};
static uint32_t rows_of_batch(const FusedEpoch& E, uint64_t b) { return (uint32_t)std::min<uint64_t>(E.B, E.s->n_rows - b * E.B); }
// FMX_SMALL_TRACE=<file>: device time stamps of the epoch's middle batch (fmx_small_kernels.h SmallSync::trace), appended to the file
static const char* small_trace_file() { static const char* f = getenv("FMX_SMALL_TRACE"); return f; }
static int small_trace_arm(fmx_handle h, hipStream_t st, unsigned long long** trace) {
  if (!small_trace_file()) return FMX_OK;
  *trace = h->small_slots + (size_t)3 * SMALL_ONE_MAX;
  unsigned long long init[16];
  for (int i = 0; i < 16; i++) init[i] = (i == 0 || i == 5) ? ~0ull : 0ull;
  HIPCHK(h, hipMemcpyAsync(*trace, init, sizeof(init), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return FMX_OK;
}
static int small_trace_dump(fmx_handle h, hipStream_t st, const unsigned long long* trace, uint64_t n_batch) {
  unsigned long long tr[16];
  HIPCHK(h, hipMemcpyAsync(tr, trace, sizeof(tr), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (FILE* f = fopen(small_trace_file(), "a")) {
    const double t0 = (double)tr[0];
    fprintf(f, "batch %llu of %llu (ns after the first example started): last example started %.0f, rows gathered %.0f, multiplier published %.0f, example done %.0f | "
               "first owner started %.0f, last owner saw its tags %.0f, holds its S rows %.0f, done %.0f | recurrence done %.0f | last owner started %.0f, has its entry list %.0f\n",
            (unsigned long long)(n_batch / 2), (unsigned long long)n_batch, tr[1] - t0, tr[2] - t0, tr[3] - t0, tr[4] - t0, (double)tr[5] - t0, tr[6] - t0, tr[7] - t0, tr[8] - t0, tr[9] - t0, tr[10] - t0, tr[11] - t0);
    fclose(f);
  }
  return FMX_OK;
}
// small batches as ONE launch per batch across all dies (k_small_one, fmx_small_kernels.h; FMX_SMALL_ONE=0 at fmx_create: two launches)
static int fused_batch_one_launch(FusedEpoch& E, uint64_t b, EpochCounts* n) {
  fmx_handle h = E.h; const Slot& s = *E.s; const Hyper& hy = E.hy;
  const uint32_t B = E.B, d = E.d, chunk = E.chunk, nb = rows_of_batch(E, b);
  const uint64_t row0 = b * B, n_batch = E.n_batch;
  float* S = h->partial;                                        // [nb][KP] x {tag, value}: 8 bytes per element (the two batches' worth of the scratch)
  const SegWork sw = seg_work(h, s, (size_t)b, S, h->mult + (size_t)(b & 1) * E.Bc);
  n->deferred += sw.nseg;
  // the recurrence: at lag >= 2 one launch behind (k_small_one), the last launch catches up
  const bool defer = d >= 2u;
  const bool own = !defer || b + 1 == n_batch, prev = defer && b >= 1;
  const ScanSmall sc{nullptr, s.target + row0, h->w0_pp + (b % d), h->w0_pp + ((b + 1) % d), own ? nb : 0u, chunk};
  const ScanSmall sc_prev{nullptr, s.target + (prev ? row0 - B : 0), h->w0_pp + ((b + d - 1) % d), h->w0_pp + (b % d), prev ? B : 0u, chunk};
  unsigned long long* rs0 = h->small_slots + SMALL_ONE_MAX;
  const SmallSync sy{h->small_slots, rs0 + (size_t)(b & 1) * SMALL_ONE_MAX, rs0 + (size_t)((b + 1) & 1) * SMALL_ONE_MAX, (uint32_t)(b + 1), (uint32_t)b,
                     h->handoff_err, std::min<uint32_t>(h->pit_spins, 1u << 21), (E.small_trace && b == n_batch / 2) ? E.small_trace : nullptr};
  const uint32_t n_ex_wg = (nb + 3u) / 4u;
  bool launched = false;
#define FMX_SMALL1(KPV, ZRV) do { if (h->KP == KPV && E.szr == ZRV) {                                                                    \
    auto kf = k_small_one<KPV, ZRV>;                                                                                                       \
    if (!E.small_cap) {                                                                                                                    \
      int per_cu = 0;                                                                                                                      \
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kf, 256, 0) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; } \
      E.small_cap = std::max(1, per_cu * h->num_cu);                                                                                       \
    }                                                                                                                                      \
    const uint32_t room = (uint32_t)E.small_cap > n_ex_wg + 1u ? (uint32_t)E.small_cap - n_ex_wg - 1u : 1u;                                \
    const uint32_t own_wg = sw.nseg ? std::max(1u, std::min((sw.nseg + 3u) / 4u, room)) : 0u;                                              \
    hipLaunchKernelGGL(kf, dim3(n_ex_wg + own_wg + 1u), dim3(256), 0, h->stream, s.ent, s.row_ptr, s.target, row0, nb, h->tb, hy,          \
                       (const double*)(h->w0_pp + ((b + 1) % d)), (const uint64_t*)s.cmask, S, s.fixed_nnz, sw, sc_prev, sc, sy, n_ex_wg,  \
                       (const uint64_t*)(E.keep ? s.lmask : nullptr), E.keep ? s.wside : (float*)nullptr);                                 \
    launched = true; } } while (0)
  FMX_SMALL1(8, 8);    FMX_SMALL1(16, 16);  FMX_SMALL1(32, 32);
  FMX_SMALL1(64, 16);  FMX_SMALL1(64, 40);  FMX_SMALL1(64, 64);
  FMX_SMALL1(128, 16); FMX_SMALL1(128, 40); FMX_SMALL1(128, 64);
#undef FMX_SMALL1
  if (!launched) return fail(h, FMX_E_STATE, "no one-launch instance for %d factors and %d row slots", h->KP, E.szr);   // (every width the epoch admits has its instances)
  HIPCHK(h, hipGetLastError());
  h->small_one_used = true;
  h->run_status |= FMX_STAT_SMALL_ONE;
  return FMX_OK;
}
// the example pass of batch b (k_fused<FUSED_EXACT>) into the batch's half of the scratch; leaves the batch's deferred list in *sw
static int fused_examples(const FusedEpoch& E, uint64_t b, const double* w0_in, float* rest, SegWork* sw, EpochCounts* n) {
  fmx_handle h = E.h; const Slot& s = *E.s;
  float* S = h->partial + (size_t)(b & 1) * E.Bc * (size_t)(h->KP + 1);
  float* mult = h->mult + (size_t)(b & 1) * E.Bc;
  int rc = FMX_OK;
  KP_SWITCH(h->KP, { rc = launch_fused_zr<KP, FUSED_EXACT>(h, s, E.hy, b * E.B, rows_of_batch(E, b), h->stream, w0_in, rest, s.cmask, S, mult,
                                                             E.handoff ? h->handoff_err : nullptr, E.keep, E.wt); });
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  *sw = seg_work(h, s, (size_t)b, S, mult);
  n->deferred += sw->nseg;
  return FMX_OK;
}
// small batches (what the stability cut leaves of data with frequent features): a batch is a few microseconds of work, so
// the recurrence leaves the side stream and rides in the launch of the deferred features (k_apply_seg_scan) -- no events, two
// launches per batch.  Same rule, same ring of bias slots: what a batch reads does not depend on which stream wrote it.
static int fused_batch_in_stream(const FusedEpoch& E, uint64_t b, EpochCounts* n) {
  fmx_handle h = E.h; const Slot& s = *E.s;
  const uint32_t d = E.d;
  float* rest = h->rest + (size_t)(b % d) * E.Bc;
  SegWork sw;
  int rc = fused_examples(E, b, h->w0_pp + ((b + 1) % d), rest, &sw, n); if (rc) return rc;   // (the bias of batch b - d; the initial one for b < d)
  // deferred features and bias recurrence in ONE launch (one workgroup per four segments + one for the recurrence)
  const ScanSmall sc{rest, s.target + b * E.B, h->w0_pp + (b % d), h->w0_pp + ((b + 1) % d), rows_of_batch(E, b), E.chunk};
  KP_SWITCH(h->KP, hipLaunchKernelGGL((k_apply_seg_scan<KP, 8, 1>), dim3((sw.nseg + 3) / 4 + 1), dim3(256), 0, h->stream, sw, h->tb, E.hy, sc));
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}
// large batches: the recurrence runs on the side stream.  handoff (default; FMX_HANDOFF=0 at fmx_create goes back to events): the two
// streams are ordered by the DATA -- bias slots W[0 .. n_batch] that start as "pending", a counter the deferred-feature launch of a batch
// advances (fmx_kernels.h: "Device-side hand-off") -- instead of four event packets per batch; W[i] = the bias after the recurrence of batch
// i - 1, k_fused of batch b reads W[max(0, b - d + 1)], the recurrence of batch b reads W[b] and publishes W[b + 1].
static int fused_batch_side(const FusedEpoch& E, uint64_t b, EpochCounts* n) {
  fmx_handle h = E.h; const Slot& s = *E.s; const Hyper& hy = E.hy;
  hipStream_t st = h->stream;
  const uint32_t d = E.d, nb = rows_of_batch(E, b);
  const uint64_t row0 = b * E.B;
  const bool handoff = E.handoff;
  // rest buffers: with events the launch of batch b waits for the recurrence of batch b - d, which was the last reader of buffer b % d;
  // with the hand-off k_fused writes rest[] BEFORE it asks for that bias, so it takes a buffer whose reader (batch b - d - 1) is known
  // to be done: every wavefront of the previous launch has consumed its result
  float* rest = h->rest + (size_t)(handoff ? b % (d + 1) : b % d) * E.Bc;
  if (!handoff && b >= d) HIPCHK(h, hipStreamWaitEvent(st, h->ev_sync[2 * (b - d) + 1], 0));   // recurrence of batch b - d is done
  const double* w0_in = handoff ? E.W + (b + 1 >= d ? b + 1 - d : 0)
                                : h->w0_pp + ((b + 1) % d);    // written by the recurrence of batch b - d (initial bias for b < d)
  SegWork sw;
  int rc = fused_examples(E, b, w0_in, rest, &sw, n); if (rc) return rc;
  if (!handoff) HIPCHK(h, hipEventRecord(h->ev_sync[2 * b], st));
  if (handoff) { sw.done_ctr = h->handoff_ctr; sw.done_val = E.hbase + b + 1; }
  if (handoff && !sw.nseg) hipLaunchKernelGGL(k_handoff_signal, dim3(1), dim3(64), 0, st, h->handoff_ctr, E.hbase + b + 1);
  if (sw.nseg) {
    // segments per wavefront of the deferred-feature pass: 16 (measured best at the bench shape: 8 / 16 / 32 / 64 -> 244.5 / 245.0 /
    // 243.0 / 241.0 M examples/s), fewer when the list is short so that the pass still spreads over the chip
    // (rows in flight per round: 8; round 6 measured 4 / 8 / 16 at the bench shape: 274.7 / 274.3 / 267.2 M examples/s)
    if (sw.nseg >= 16u * 2048u)     { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_apply_seg<KP, 8, 16>), ((uint64_t)sw.nseg + 15) / 16, st, sw, h->tb, hy)); }
    else if (sw.nseg >= 4u * 2048u) { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_apply_seg<KP, 8, 4>), ((uint64_t)sw.nseg + 3) / 4, st, sw, h->tb, hy)); }
    else                            { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_apply_seg<KP, 8, 1>), (uint64_t)sw.nseg, st, sw, h->tb, hy)); }
    HIPCHK(h, hipGetLastError());
  }
  if (handoff)
    return launch_scan(h, rest, s.target + row0, nb, E.chunk, hy, nullptr, h->stream2, E.W + b, E.W + b + 1,
                       Handoff{h->handoff_ctr, E.hbase + b + 1, h->handoff_err});
  HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_sync[2 * b], 0));
  rc = launch_scan(h, rest, s.target + row0, nb, E.chunk, hy, nullptr, h->stream2, h->w0_pp + (b % d), h->w0_pp + ((b + 1) % d)); if (rc) return rc;
  HIPCHK(h, hipEventRecord(h->ev_sync[2 * b + 1], h->stream2));
  return FMX_OK;
}
static int sgd_epoch_fused(fmx_handle h, Slot& s, const fmx_sgd_opts* opts, const Hyper& hy, EpochCounts* n) {
  FusedEpoch E{h, &s, hy};
  const uint32_t B = E.B = opts->batch;                     // resolved by the caller (sgd_resolve_batch)
  const uint32_t d = E.d = opts->bias_lag ? opts->bias_lag : 1u;
  if (d > 4) return fail(h, FMX_E_ARG, "bias_lag %u: at most 4 batches", d);
  E.chunk = opts->w0_chunk ? opts->w0_chunk : default_w0_chunk(h->cfg);
  int rc = ensure_segments(h, s, B); if (rc) return rc;
  rc = ensure_ids(h, s); if (rc) return rc;                 // unit-valued fixed-length rows: k_fused streams the ids alone
  // FMX_FLAG_KEEP_WSIDE: this epoch keeps the slot's weight side stream current (for the evaluation passes that follow it)
  const bool keep_wside = (opts->flags & FMX_FLAG_KEEP_WSIDE) && hy.k1 && h->cfg.shard_world == 1 && s.blocks.empty();
  if (keep_wside) { rc = ensure_wside(h, s); if (rc) return rc; }
  n->kept_wside = E.keep = keep_wside && s.wside != nullptr;
  // the slot's training-side weight stream (WTrain): the linear weights of its once-only features, kept by this epoch whatever its flags
  const bool wtrain_ok = hy.k1 && !hy.sgda && h->cfg.shard_world == 1 && s.blocks.empty() && !s.weight;
  if (wtrain_ok) { rc = ensure_wtrain(h, s, s.fused_cap); if (rc) return rc; }
  const uint32_t Bc = E.Bc = std::min<uint32_t>(B, s.n_rows);
  rc = ensure_scratch(h, (size_t)Bc * 2, (size_t)Bc * (d + 1)); if (rc) return rc;   // S / mult of two consecutive batches, d (+ 1: hand-off) rest buffers
  const uint64_t n_batch = E.n_batch = ((uint64_t)s.n_rows + B - 1) / B;
  const bool side = B >= FMX_SIDE_STREAM_BATCH;             // (below: fused_batch_in_stream / fused_batch_one_launch)
  // the hand-off of fused_batch_side.  bias_lag 1 keeps the events: there every wavefront of k_fused WAITS for a slot the one-workgroup
  // recurrence of the previous batch publishes, and nothing guarantees that kernel a CU once k_fused has filled the chip -- round-4 advisor;
  // at lag >= 2 the slot is a batch old
  // ... and only where the two streams really run side by side (streams_concurrent: probed once per handle): under serialised dispatch the
  // waits of the hand-off are satisfied by LATER launches and every batch would run into its bound
  const bool handoff = E.handoff = side && h->handoff && hy.k0 && d >= 2 && !(opts->flags & FMX_FLAG_EVENT_SYNC) && streams_concurrent(h);
  if (side && hy.k0 && !handoff) h->run_status |= FMX_STAT_EVENT_SYNC;
  if (!side && hy.k0) h->run_status |= FMX_STAT_SCAN_SERIAL;
  if (handoff) {
    if (h->w0_slots_cap < n_batch + 1) {
      if (h->w0_slots) HIPCHK(h, fmx_dev_free(h->w0_slots));
      h->w0_slots = nullptr; h->w0_slots_cap = 0;
      HIPCHK(h, fmx_dev_alloc(&h->w0_slots, (size_t)(n_batch + 1) * sizeof(double)));
      h->w0_slots_cap = n_batch + 1;
    }
    E.W = h->w0_slots;
    E.hbase = h->handoff_seq; h->handoff_seq += n_batch + 1;         // the counter only grows: no reset to order against the side stream
  }
  if (side && !handoff) while (h->ev_sync.size() < 2 * n_batch + 1) { hipEvent_t e; HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->ev_sync.push_back(e); }
  hipStream_t st = h->stream;
  HIPCHK(h, hipEventRecord(h->ev0, st));                    // do not bill the one-time bucketing to the epoch
  for (uint32_t r = 0; r < d; r++) HIPCHK(h, hipMemcpyAsync(h->w0_pp + r, h->w0, sizeof(double), hipMemcpyDeviceToDevice, st));
  if (handoff) {
    hipLaunchKernelGGL(k_handoff_arm, dim3((unsigned)std::min<uint64_t>((n_batch + 255) / 256, 64)), dim3(256), 0, st, E.W, (uint32_t)n_batch);
    HIPCHK(h, hipMemcpyAsync(E.W, h->w0, sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  const bool small_one = !side && h->small_one && (h->KP == 8 || h->KP == 16 || h->KP == 32 || h->KP == 64 || h->KP == 128) && s.cdesc && Bc <= SMALL_ONE_MAX && !hy.sgda;
  // the singles' linear weights from their packed stream (k_fused<FUSED_EXACT> alone maintains it: not the one-launch form)
  if (wtrain_ok && !small_one && s.wtrain) {
    E.wt = WTrain{s.smask, s.soff, s.wtrain, n->wtrain_fresh ? 1u : 0u};
    n->kept_wtrain = true;
    if (E.wt.read) h->run_status |= FMX_STAT_WSTREAM;
  }
  if (small_one) {
    if (h->KP < 64) E.szr = h->KP;                                // (k <= 32: 64 / KP entries per row slot, KP slots hold any row of <= 64 entries)
    else {
      E.szr = (h->KP == 64) ? fused_zr_select<64>(s.max_row) : fused_zr_select<128>(s.max_row);
      if (E.szr == 8) E.szr = 16;                                 // (three instances per row width: 16, 40, 64 row slots)
      if (E.szr == 32) E.szr = 40;
    }
    if (!h->small_slots) HIPCHK(h, fmx_dev_alloc(&h->small_slots, ((size_t)3 * SMALL_ONE_MAX + 16) * sizeof(unsigned long long)));
    HIPCHK(h, hipMemsetAsync(h->small_slots, 0, (size_t)3 * SMALL_ONE_MAX * sizeof(unsigned long long), st));
    // ... and the tagged S_e elements (the scratch may hold anything, e.g. last epoch's elements under the same tags)
    HIPCHK(h, hipMemsetAsync(h->partial, 0, (size_t)Bc * (size_t)h->KP * sizeof(unsigned long long), st));
    rc = small_trace_arm(h, st, &E.small_trace); if (rc) return rc;
  }
  for (uint64_t b = 0; b < n_batch; b++) {
    rc = small_one ? fused_batch_one_launch(E, b, n) : side ? fused_batch_side(E, b, n) : fused_batch_in_stream(E, b, n); if (rc) return rc;
    n->batches++; n->launches++;
  }
  if (E.small_trace) { rc = small_trace_dump(h, st, E.small_trace, n_batch); if (rc) return rc; }
  if (handoff) {                                              // ONE event per epoch: the last recurrence, then the bias goes home
    if (h->ev_sync.empty()) { hipEvent_t e; HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->ev_sync.push_back(e); }
    HIPCHK(h, hipEventRecord(h->ev_sync[0], h->stream2));
    HIPCHK(h, hipStreamWaitEvent(st, h->ev_sync[0], 0));
    HIPCHK(h, hipMemcpyAsync(h->w0, E.W + n_batch, sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemcpyAsync(&h->handoff_err_host, h->handoff_err, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return FMX_OK;
  }
  if (side) HIPCHK(h, hipStreamWaitEvent(st, h->ev_sync[2 * (n_batch - 1) + 1], 0));
  if (hy.k0) HIPCHK(h, hipMemcpyAsync(h->w0, h->w0_pp + (n_batch % d), sizeof(double), hipMemcpyDeviceToDevice, st));
  return FMX_OK;
}

// ---- FMX_SGD_SEQUENTIAL as conflict-free runs (fmx_seq_kernels.h) ----
// cuts the slot into maximal runs of consecutive rows that share no feature (once per slot; host wall-clock goes to setup_seconds)
static int ensure_runs(fmx_handle h, Slot& s) {
  if (!s.run_start.empty()) return FMX_OK;
  struct Acc { fmx_handle h; std::chrono::steady_clock::time_point t0;
               ~Acc() { h->setup_acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } } acc_{h, std::chrono::steady_clock::now()};
  const uint32_t n = s.n_rows;
  if (n == 0 || n >= 0x7FFFFFFEu || s.nnz >= (1ull << 31)) { s.run_start = {0u, n}; s.run_single = {2u}; return FMX_OK; }   // (2: not cut -- the caller takes the kernel)
  hipStream_t st = h->stream;
  std::vector<uint32_t> prev(n, 0u);
  if (s.nnz) {
    uint32_t fbits = 1; while (fbits < 32 && (1ull << fbits) < std::max<uint64_t>(h->n_local, 2)) fbits++;
    size_t tmp_bytes = 0;
    HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (int)s.nnz, 0, 32 + (int)fbits, st));
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_a = 0, o_b = al(s.nnz * 8), o_p = o_b + al(s.nnz * 8), o_t = o_p + al((size_t)n * 4), total = o_t + al(std::max<size_t>(tmp_bytes, 256));
    char* scratch = nullptr;
    HIPCHK(h, fmx_dev_alloc(&scratch, total));
    uint64_t* ka = (uint64_t*)(scratch + o_a); uint64_t* kb = (uint64_t*)(scratch + o_b); uint32_t* d_prev = (uint32_t*)(scratch + o_p);
    hipError_t e = hipMemsetAsync(d_prev, 0, (size_t)n * 4, st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_run_keys, dim3(wave_grid(n)), dim3(256), 0, st, s.ent, s.row_ptr, n, ka);
      size_t tb_ = tmp_bytes;
      e = hipcub::DeviceRadixSort::SortKeys(scratch + o_t, tb_, ka, kb, (int)s.nnz, 0, 32 + (int)fbits, st);
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_run_prev, dim3(2048), dim3(256), 0, st, kb, s.nnz, d_prev);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(prev.data(), d_prev, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    fmx_dev_free(scratch);
    if (e != hipSuccess) return fail(h, FMX_E_HIP, "ensure_runs failed: %s", hipGetErrorString(e));
  }
  // greedy, in file order: a run ends in front of the first row that shares a feature with a row of the run (prev - 1 >= start), in front of
  // and behind a row that repeats an id, and at 4096 rows (one wavefront evaluates the run's bias recurrence)
  std::vector<uint32_t> starts; std::vector<uint8_t> single;
  uint32_t start = 0;
  for (uint32_t r = 0; r < n; r++) {
    const bool rep = (prev[r] & 0x80000000u) != 0;
    const uint32_t p = prev[r] & 0x7FFFFFFFu;                     // 1 + the latest earlier row sharing a feature, 0: none
    if (rep) {
      if (r > start) { starts.push_back(start); single.push_back(0); }
      starts.push_back(r); single.push_back(1);
      start = r + 1;
    } else if ((p > start && r > start) || r - start >= 4096u) {
      starts.push_back(start); single.push_back(0);
      start = r;
    }
  }
  if (start < n) { starts.push_back(start); single.push_back(0); }
  starts.push_back(n);
  s.run_start.swap(starts); s.run_single.swap(single);
  return FMX_OK;
}
// a run as ONE launch (k_run_fused): 1 = launched, 0 = not this run (rows too long for the registers, no instance, the device does not hold
// the run's workgroups at once), < 0 = error
static int launch_run_one(fmx_handle h, const Slot& s, const Hyper& hy, uint32_t row0, uint32_t nb, int zr, const double* bias_in, double* bias_out,
                          unsigned long long* slots, uint32_t tag) {
  hipStream_t st = h->stream;
  const size_t lds = (size_t)nb * 5 * sizeof(float);
  const dim3 grid((nb + 3u) / 4u);
  const RunSync rs{slots, tag, h->handoff_err, std::min<uint32_t>(h->pit_spins, 1u << 21)};   // (FMX_DEBUG_PIT_SPINS=0 at fmx_create: every poll gives up at once)
  int launched = 0;
#define FMX_RUN1(KPV, ZRV, TK) do { if (h->KP == KPV && zr == ZRV && hy.task == TK) {                                                    \
    auto kf = k_run_fused<KPV, ZRV, TK>;                                                                                                 \
    auto it = h->run_one_occ.find((const void*)kf);                                                                                      \
    if (it == h->run_one_occ.end()) {                                                                                                    \
      int per_cu = 0;                                                                                                                    \
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kf, 256, (size_t)RUN_ONE_MAX * 5 * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; } \
      it = h->run_one_occ.emplace((const void*)kf, per_cu * h->num_cu).first;                                                            \
    }                                                                                                                                    \
    if ((int)grid.x <= it->second) {                                                                                                     \
      hipLaunchKernelGGL(kf, grid, dim3(256), lds, st, s.ent, s.row_ptr, s.target, (uint64_t)row0, nb, h->tb, hy, bias_in, bias_out, rs, s.fixed_nnz); \
      launched = 1; } } } while (0)
  FMX_RUN1(8, 8, 0);    FMX_RUN1(16, 16, 0);  FMX_RUN1(32, 32, 0);  FMX_RUN1(8, 8, 1);    FMX_RUN1(16, 16, 1);  FMX_RUN1(32, 32, 1);
  FMX_RUN1(64, 16, 0);  FMX_RUN1(64, 40, 0);  FMX_RUN1(64, 64, 0);  FMX_RUN1(64, 16, 1);  FMX_RUN1(64, 40, 1);  FMX_RUN1(64, 64, 1);
  FMX_RUN1(128, 16, 0); FMX_RUN1(128, 40, 0); FMX_RUN1(128, 64, 0); FMX_RUN1(128, 16, 1); FMX_RUN1(128, 40, 1); FMX_RUN1(128, 64, 1);
#undef FMX_RUN1
  return launched;
}

// one epoch over the runs.  A run of up to RUN_ONE_MAX rows that fit the registers is ONE launch (k_run_fused: the rows stay in the wavefronts'
// registers across the run's bias recurrence); up to RUN_FUSED_MAX rows TWO: the sums, then the update whose every workgroup solves the
// recurrence for itself (k_run_apply); a longer one three (sums, k_scan_pit on one workgroup at micro-chunk 1, update).
// FMX_SEQ_RUNS_FUSED=0: always three, with the one-wavefront chain (what the first version did); FMX_SEQ_RUNS_ONE=0: never one (both read by fmx_create).
static int seq_runs_epoch(fmx_handle h, Slot& s, const Hyper& hy) {
  hipStream_t st = h->stream;
  const bool fused = h->seq_runs_fused, one_env = h->seq_runs_one;
  uint32_t longest = 1;
  for (size_t i = 0; i + 1 < s.run_start.size(); i++) longest = std::max(longest, s.run_start[i + 1] - s.run_start[i]);
  int rc = ensure_scratch(h, longest, 0);
  if (rc) return rc;
  if (!h->pit_tmp) HIPCHK(h, fmx_dev_alloc(&h->pit_tmp, 64 * sizeof(double)));
  double* bias[2] = {h->w0, h->pit_tmp + 48};                     // the fused forms read the bias in one slot and leave it in the other
  if (!h->run_slots) HIPCHK(h, fmx_dev_alloc(&h->run_slots, (size_t)RUN_ONE_MAX * sizeof(unsigned long long)));
  unsigned long long* slots = h->run_slots;                       // {tag, rest_e} of a one-launch run's examples
  int zr = 0;
  bool one = fused && one_env && h->run_one && (h->KP == 8 || h->KP == 16 || h->KP == 32 || h->KP == 64 || h->KP == 128) && s.max_row <= 64u;
  if (one && h->KP < 64) zr = h->KP;                              // (k <= 32: 64 / KP entries per row slot, KP slots hold any row of <= 64 entries)
  else if (one) {
    zr = (h->KP == 64) ? fused_zr_select<64>(s.max_row) : fused_zr_select<128>(s.max_row);
    if (s.max_row > (uint32_t)zr) one = false;                    // (rows beyond the register path)
    if (zr == 8) zr = 16;                                         // (three instances per row width: 16, 40, 64 row slots)
    if (zr == 32) zr = 40;
  }
  if (one) HIPCHK(h, hipMemsetAsync(slots, 0, (size_t)RUN_ONE_MAX * sizeof(unsigned long long), st));
  int cur = 0;
  for (size_t i = 0; i + 1 < s.run_start.size(); i++) {
    const uint32_t row0 = s.run_start[i], nb = s.run_start[i + 1] - row0;
    if (s.run_single[i]) {                                        // a row that repeats an id: entry by entry (fm_sgd.h:44-50)
      KP_SWITCH(h->KP, hipLaunchKernelGGL((k_sequential<KP>), dim3(1), dim3(64), 0, st, s.ent, s.row_ptr + row0, s.target + row0, nb, h->tb, hy, bias[cur]));
      h->run_status |= FMX_STAT_SEQ_ENTRIES;
      continue;
    }
    if (one && nb <= RUN_ONE_MAX) {
      rc = launch_run_one(h, s, hy, row0, nb, zr, bias[cur], bias[cur ^ 1], slots, (uint32_t)i + 1u);
      if (rc < 0) return rc;
      if (rc == 1) { h->run_one_used = true; h->run_status |= FMX_STAT_RUN_ONE; if (hy.k0) cur ^= 1; continue; }
    }
    float* S = h->partial;
    float* rest = S + (size_t)nb * h->KP;
    KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, true, true>), nb, st, s.ent, s.row_ptr, (uint64_t)row0, nb, RowsF32{h->tb}, h->cfg.k1, S, rest));
    if (fused && nb <= RUN_FUSED_MAX) {
      const dim3 grid((nb + 3u) / 4u);
      const size_t lds = (size_t)nb * 5 * sizeof(float);
      if (hy.task == 0) { KP_SWITCH(h->KP, hipLaunchKernelGGL((k_run_apply<KP, 0>), grid, dim3(256), lds, st, s.ent, s.row_ptr, (uint64_t)row0, nb, h->tb, hy, S, rest, s.target, bias[cur], bias[cur ^ 1])); }
      else              { KP_SWITCH(h->KP, hipLaunchKernelGGL((k_run_apply<KP, 1>), grid, dim3(256), lds, st, s.ent, s.row_ptr, (uint64_t)row0, nb, h->tb, hy, S, rest, s.target, bias[cur], bias[cur ^ 1])); }
      h->run_status |= FMX_STAT_RUN_TWO;
      if (hy.k0) cur ^= 1;
      continue;
    }
    h->run_status |= FMX_STAT_RUN_THREE;
    rc = launch_scan(h, rest, s.target + row0, nb, 1u, hy, h->mult, st, bias[cur], bias[cur], Handoff{nullptr, 0ull, nullptr}, fused);
    if (rc) return rc;
    KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_apply<KP, false>), nb, st, s.ent, s.row_ptr, (uint64_t)row0, nb, h->tb, hy, S, h->mult));
  }
  if (cur) HIPCHK(h, hipMemcpyAsync(h->w0, bias[1], sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// ---- fmx_sgd_epoch: one driver per mode (epoch_sequential, epoch_hogwild, epoch_split, sgd_epoch_fused), then epoch_close ----
static int epoch_sequential(fmx_handle h, Slot& s, const Hyper& hy, EpochCounts* n) {
  // rows of 64 / 128 lanes: a row at a time with the next example's rows in flight (fmx_seq_kernels.h: 20 k -> ~1 M examples/s on the
  // reference's own trajectory); FMX_SEQ_ROWS=0 and the other row widths: entry by entry
  const bool seq_rows = h->seq_rows, seq_wg = h->seq_wg;      // (FMX_SEQ_ROWS / FMX_SEQ_WG: read by fmx_create)
  // where consecutive rows rarely share a feature: the same trajectory as conflict-free runs at batch speed (fmx_seq_kernels.h); taken when
  // the slot's runs average >= 16 rows (FMX_SEQ_RUNS=0: never, =1: always)
  const char* sr = getenv("FMX_SEQ_RUNS");
  bool use_runs = !(sr && sr[0] == '0');
  int rc = FMX_OK;
  if (use_runs) {
    rc = ensure_runs(h, s); if (rc) return rc;
    const size_t n_runs = s.run_start.size() - 1;
    use_runs = !(s.run_single.size() == 1 && s.run_single[0] == 2) && ((sr && sr[0] == '1') || (uint64_t)s.n_rows >= 16ull * n_runs);
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));             // (the one-time cut is not the epoch's time)
  }
  if (use_runs) {
    rc = seq_runs_epoch(h, s, hy); if (rc) return rc;
    h->run_status |= FMX_STAT_SEQ_RUNS;
  } else if (seq_rows && seq_wg && h->KP <= 128) {
    // eight wavefronts on each example (fmx_seq_kernels.h k_sequential_wg); FMX_SEQ_WG=0: one wavefront, a row at a time.
    // Fewer than 33 factors run the 64-lane instance too: a row access masks the lanes beyond the row (tb.rs), whatever the lane mapping
    auto kf = h->KP <= 64 ? k_sequential_wg<64> : k_sequential_wg<128>;
    const size_t lds = h->KP <= 64 ? sizeof(SeqLds<64>) : sizeof(SeqLds<128>);
    FMX_RAISE_LDS(kf, lds);
    hipLaunchKernelGGL(kf, dim3(1), dim3(64 * SEQ_W), lds, h->stream, s.ent, s.row_ptr, s.target, s.n_rows, s.nnz, h->tb, hy, h->w0);
    h->run_status |= FMX_STAT_SEQ_WG;
  } else if (seq_rows && h->KP <= 128) {
    h->run_status |= FMX_STAT_SEQ_ROWS;
    const bool wide = s.max_row > 32u;
    auto kf = h->KP <= 64 ? (wide ? k_sequential_rows<64, 64> : k_sequential_rows<64, 32>) : (wide ? k_sequential_rows<128, 64> : k_sequential_rows<128, 32>);
    hipLaunchKernelGGL(kf, dim3(1), dim3(64), 0, h->stream, s.ent, s.row_ptr, s.target, s.n_rows, h->tb, hy, h->w0);
  } else {
    KP_SWITCH(h->KP, hipLaunchKernelGGL((k_sequential<KP>), dim3(1), dim3(64), 0, h->stream, s.ent, s.row_ptr,
                                          s.target, s.n_rows, h->tb, hy, h->w0));
    h->run_status |= FMX_STAT_SEQ_ENTRIES;
  }
  HIPCHK(h, hipGetLastError());
  n->batches = use_runs ? s.run_start.size() - 1 : s.n_rows;
  n->launches = 1;
  return FMX_OK;
}
static int epoch_hogwild(fmx_handle h, Slot& s, const fmx_sgd_opts* opts, const Hyper& hy, EpochCounts* n) {
  if (opts->apply == FMX_APPLY_SEGMENTED) return fail(h, FMX_E_ARG, "HOGWILD has no segmented apply");
  // rows per launch M: w0 is frozen inside a launch.  The bias recurrence of launch i (k_scan, one wavefront) runs
  // on a side stream WHILE launches i+1, i+2 stream; launch i reads the w0 produced by scan i-3 (a ring of 3
  // slots / rest buffers, so the result does not depend on timing and a slow scan has two launches of slack).
  const uint32_t M = opts->batch ? opts->batch : 262144u;
  const uint32_t chunk = opts->w0_chunk ? opts->w0_chunk : default_w0_chunk(h->cfg);
  const uint32_t cap = std::min<uint32_t>(M, s.n_rows);
  int rc = ensure_scratch(h, 0, (size_t)cap * 3); if (rc) return rc;
  if (!s.ids_asked) {
    rc = ensure_ids(h, s); if (rc) return rc;               // unit-valued fixed-length rows: k_fused streams the ids alone
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));           // (the one-time copy is not the epoch's time)
  }
  const uint64_t n_launch = ((uint64_t)s.n_rows + M - 1) / M;
  while (h->ev_sync.size() < 2 * n_launch) { hipEvent_t e; HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->ev_sync.push_back(e); }
  for (int r = 0; r < 3; r++) HIPCHK(h, hipMemcpyAsync(h->w0_pp + r, h->w0, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  for (uint64_t i = 0; i < n_launch; i++) {
    const uint64_t row0 = i * M;
    const uint32_t nb = (uint32_t)std::min<uint64_t>(M, s.n_rows - row0);
    float* rest = h->rest + (size_t)(i % 3) * cap;
    hipStream_t fs = h->stream;
    if (i >= 3) HIPCHK(h, hipStreamWaitEvent(fs, h->ev_sync[2 * (i - 3) + 1], 0));   // scan i-3 done
    // (no per-launch events here: a timing event between two launches costs ~13 % on this path; the epoch is
    //  bracketed by ev0/ev1 on the launch stream and the average launch time is epoch time / launches)
    n->launches++;
    const double* w0_in = h->w0_pp + ((i + 1) % 3);      // slot written by scan i-3 (initial value for i < 3)
    if (opts->apply == FMX_APPLY_ATOMIC) {
      KP_SWITCH(h->KP, { rc = launch_fused_zr<KP, FUSED_ATOMIC>(h, s, hy, row0, nb, fs, w0_in, rest); });
    } else {
      KP_SWITCH(h->KP, { rc = launch_fused_zr<KP, FUSED_STORE>(h, s, hy, row0, nb, fs, w0_in, rest); });
    }
    if (rc) return rc;
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev_sync[2 * i], fs));
    HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_sync[2 * i], 0));
    rc = launch_scan(h, rest, s.target + row0, nb, chunk, hy, nullptr, h->stream2, h->w0_pp + (i % 3), h->w0_pp + ((i + 1) % 3)); if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->ev_sync[2 * i + 1], h->stream2));
    n->batches++;
  }
  // stream2 is in order: its last event covers every scan, and scan i waited for launch i
  HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_sync[2 * (n_launch - 1) + 1], 0));
  if (hy.k0) HIPCHK(h, hipMemcpyAsync(h->w0, h->w0_pp + (n_launch % 3), sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  return FMX_OK;
}
// the two-pass forms of the MINIBATCH rule on one handle: per batch the sums (k_rowsums leaves rest[] too), then the split step.
// FMX_FLAG_TIME_MAIN_KERNEL: a pair of events from h->ev_pool around every batch's update (n->launches counts the pairs)
static int epoch_split(fmx_handle h, Slot& s, const fmx_sgd_opts* opts, EpochCounts* n) {
  const uint32_t B = opts->batch;
  const bool timed = (opts->flags & FMX_FLAG_TIME_MAIN_KERNEL) != 0;
  const bool segmented = (opts->apply == FMX_APPLY_DEFAULT || opts->apply == FMX_APPLY_SEGMENTED);
  const uint32_t lag_depth = opts->bias_lag ? opts->bias_lag : 1u;
  if (lag_depth > 4) return fail(h, FMX_E_ARG, "bias_lag %u: at most 4 batches", lag_depth);
  const uint32_t Bc = std::min<uint32_t>(B, s.n_rows);
  int rc = ensure_scratch(h, (size_t)Bc * ((opts->flags & FMX_FLAG_BIAS_LAG) ? lag_depth + 1 : 1), 0); if (rc) return rc;
  if (segmented) {
    rc = ensure_segments(h, s, B); if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));           // do not bill the one-time bucketing to the epoch
  }
  StepPlan plan = step_plan(h, s, opts, segmented ? 0 : -1, true);   // the same for every batch, its index aside
  while (timed && h->ev_pool.size() < 2 * (((size_t)s.n_rows + B - 1) / B)) { hipEvent_t e; HIPCHK(h, hipEventCreate(&e)); h->ev_pool.push_back(e); }
  for (uint64_t row0 = 0; row0 < s.n_rows; row0 += B) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>(B, s.n_rows - row0);
    int pslot = 0;
    if (plan.lag) { rc = lag_prepare(h, h->stream, plan, &pslot); if (rc) return rc; }
    float* S = h->partial + (size_t)pslot * Bc * (size_t)(h->KP + 1);
    float* rest = S + (size_t)nb * h->KP;
    KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, true, true>), nb, h->stream,
                                       s.ent, s.row_ptr, row0, nb, RowsF32{h->tb}, h->cfg.k1, S, rest));
    hipEvent_t ea = nullptr, eb = nullptr;
    if (timed) { ea = h->ev_pool[2 * n->launches]; eb = h->ev_pool[2 * n->launches + 1]; n->launches++; }
    if (segmented) plan.seg_batch = (int64_t)(row0 / B);
    rc = sgd_finish_impl(h, s, row0, nb, S, rest, nullptr, plan, h->stream, ea, eb); if (rc) return rc;
    n->batches++;
  }
  return FMX_OK;
}

// the end of every epoch: drain, the bias back in h->w0, what the device's error word says about the epoch, the stats
static int epoch_close(fmx_handle h, Slot& s, const fmx_sgd_opts* opts, const fmx_batch_info& bi, const EpochCounts& n, fmx_epoch_stats* stats) {
  if (h->lag.active)       // the last recurrence must finish inside the timed region; then w0 returns to h->w0
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->lag.ev_scan[(h->lag.step - 1) % LagState::RING], 0));
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipGetLastError());
  int rc = lag_flush(h); if (rc) return rc;
  rc = scan_error_check(h); if (rc) return rc;
  uint32_t bits = 0;
  // one launch per small batch / per conflict-free run of FMX_SGD_SEQUENTIAL: did every owner, the recurrence, every workgroup see its examples?
  const struct { bool* used; bool* enabled; const char* text; } one_launch[2] = {
    {&h->small_one_used, &h->small_one,
     "a one-launch batch never saw all of its examples (the device is shared or partitioned): the features concerned took no "
     "step (the parameters are valid numbers, the epoch is not the batch rule's) -- reload the parameters; the handle takes "
     "two launches per batch from now on"},
    {&h->run_one_used, &h->run_one,
     "a conflict-free run never saw all of its workgroups (the device is shared or partitioned): the rows concerned took no "
     "step (the parameters are valid numbers, the epoch is not the reference's) -- reload the parameters; the handle takes "
     "two launches per run from now on"}};
  for (const auto& o : one_launch) {
    if (!*o.used) continue;
    *o.used = false;
    rc = take_error_bits(h, RUN_ERR_EXCHANGE, &bits); if (rc) return rc;
    if (!bits) continue;
    *o.enabled = false;
    h->run_status |= FMX_STAT_HANDOFF_TIMEOUT;
    if (stats) stats->status = bi.status | h->run_status;
    return fail(h, FMX_E_HIP, "%s", o.text);
  }
  if (h->handoff_err_host & 3u) {
    // a hand-off wait ran into its bound (the probe said the streams run side by side, and then they did not: the device is shared with
    // work that starved one of them).  Nothing was computed from a bias that was not there: the examples concerned took no step, a
    // recurrence that never saw its batch handed the bias on unchanged (fmx_kernels.h) -- every parameter is a valid number, but the
    // epoch is not the rule's.  The handle orders its streams with events from now on.
    const uint32_t e = h->handoff_err_host;
    h->handoff_err_host = 0;
    (void)take_error_bits(h, 3u, &bits);                        // (only the hand-off's own bits: bit 4 belongs to scan_error_check)
    h->handoff = false;
    h->run_status |= FMX_STAT_HANDOFF_TIMEOUT;
    if (stats) stats->status = bi.status | h->run_status;
    return fail(h, FMX_E_HIP, "the bias hand-off between the launch stream and the recurrence timed out (flags %u): the examples concerned took no "
                              "step (the parameters are valid numbers, the epoch is not the batch rule's); the handle orders its streams with "
                              "events from now on", e);
  }
  if (n.kept_wside) s.wside_version = h->w_version;          // the epoch is complete: the stream holds this w
  if (n.kept_wtrain) s.wtrain_version = h->w_version;        // ... and so does the training-side one
  if (stats) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    stats->rows = s.n_rows; stats->batches = n.batches; stats->device_seconds = ms * 1e-3;
    if (opts->mode == FMX_SGD_MINIBATCH && s.seg_B) stats->max_feature_count = s.max_seg_count;
    stats->deferred_features = n.deferred;
    if (opts->mode == FMX_SGD_MINIBATCH || opts->mode == FMX_SGD_HOGWILD) {     // (HOGWILD: batch_used = the rows in flight)
      stats->batch_used = bi.batch; stats->collision_mass = bi.collision_mass; stats->batch_gain = bi.batch_gain; stats->status = bi.status;
    }
    stats->status |= h->run_status;
    stats->setup_seconds = h->setup_acc;
    if (opts->mode != FMX_SGD_SEQUENTIAL) stats->w0_chunk_used = opts->w0_chunk ? opts->w0_chunk : default_w0_chunk(h->cfg);
    stats->main_kernel_seconds = stats->device_seconds;
    stats->main_kernel_launches = n.launches;
    if (opts->mode == FMX_SGD_MINIBATCH && (opts->flags & FMX_FLAG_TIME_MAIN_KERNEL) && opts->apply != FMX_APPLY_FUSED) {
      double tot = 0;                                           // epoch_split's event pairs
      for (size_t i = 0; i < n.launches; i++) {
        float m2 = 0;
        HIPCHK(h, hipEventElapsedTime(&m2, h->ev_pool[2 * i], h->ev_pool[2 * i + 1]));
        tot += m2 * 1e-3;
      }
      stats->main_kernel_seconds = tot;
    }
  }
  return FMX_OK;
}

int fmx_sgd_epoch(fmx_handle h, int slot, const fmx_sgd_opts* opts, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_sgd_epoch"); if (_sr) return _sr; }
  int rc = check_slot(h, slot, true); if (rc) return rc;
  rc = refuse_weighted(h, slot, "fmx_sgd_epoch"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  if (!opts) return fail(h, FMX_E_ARG, "fmx_sgd_epoch: opts is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[slot];
  if (stats) memset(stats, 0, sizeof(*stats));
  if (s.n_rows == 0) return FMX_OK;
  if (!s.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "relations are not supported with SGD");   // fm_learn_sgd.h:61-63
  if (!(h->group && !h->owns_group)) { h->setup_acc = 0.0; h->run_status = 0; }   // (a group clears its members' before the epoch)
  if (h->cfg.shard_world > 1 && opts->mode != FMX_SGD_MINIBATCH)
    return fail(h, FMX_E_UNSUPPORTED, "feature shards train with FMX_SGD_MINIBATCH (the split step)");
  if (h->cfg.shard_world > 1 || h->comm) return comm_sgd_epoch(h, slot, opts, stats);   // (a communicator of one rank drives the same schedule)
  const Hyper hy = make_hyper(h->cfg);
  fmx_sgd_opts ropts = *opts;                               // MINIBATCH: `batch` resolved against the rows' collision mass
  fmx_batch_info bi; memset(&bi, 0, sizeof(bi));
  if (opts->mode == FMX_SGD_MINIBATCH) {
    rc = sgd_resolve_batch(h, s, opts, &bi); if (rc) return rc;
    if ((opts->flags & FMX_FLAG_REJECT_UNSTABLE) && (bi.status & FMX_STAT_UNSTABLE)) {
      if (opts->batch == 0)       // the library's own choice is at its floor and still unstable: say THAT, not "let the library choose"
        return fail(h, FMX_E_ARG, "these rows are too dense for the batch rule: at the smallest batch the library takes (%u rows) learn_rate * "
                                  "curvature * batch * collision mass = %.3g > 2 (collision mass %.4g) -- lower learn_rate or train with "
                                  "FMX_SGD_SEQUENTIAL", bi.batch, bi.batch_gain, bi.collision_mass);
      return fail(h, FMX_E_ARG, "batch %u on these rows: learn_rate * curvature * batch * collision mass = %.3g > 2 -- the batch rule "
                                "diverges (collision mass %.4g; batch 0 lets the library choose)", bi.batch, bi.batch_gain, bi.collision_mass);
    }
    ropts.batch = bi.batch;
    opts = &ropts;
  } else if (opts->mode == FMX_SGD_HOGWILD) {
    // the asynchronous step freezes nothing, but an update becomes visible only when its wavefront retires: the rows in flight
    // (5 wavefronts per SIMD x 4 SIMDs x CUs on this part, one example each) are the window the criterion of MINIBATCH applies to
    rc = ensure_coll_mass(h, s); if (rc) return rc;
    const uint32_t in_flight = (uint32_t)std::min<uint64_t>(s.n_rows, (uint64_t)20 * (uint64_t)h->num_cu);
    resolve_batch(h->cfg, s.coll_mass, in_flight, in_flight, 1.0, &bi);
    if ((opts->flags & FMX_FLAG_REJECT_UNSTABLE) && (bi.status & FMX_STAT_UNSTABLE))
      return fail(h, FMX_E_ARG, "HOGWILD on these rows: learn_rate * curvature * %u rows in flight * collision mass = %.3g > 2 -- the asynchronous "
                                "step diverges (collision mass %.4g; use FMX_SGD_MINIBATCH with batch 0)", in_flight, bi.batch_gain, bi.collision_mass);
  }
  EpochCounts n;
  n.wtrain_fresh = s.wtrain && s.wtrain_version == h->w_version;   // (decided on the w this epoch starts from)
  touch_w(h);                                                // (every side stream is stale from here on; this epoch may re-validate ITS slot's)
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  switch (opts->mode) {
    case FMX_SGD_SEQUENTIAL: rc = epoch_sequential(h, s, hy, &n); break;
    case FMX_SGD_HOGWILD:    rc = epoch_hogwild(h, s, opts, hy, &n); break;
    case FMX_SGD_MINIBATCH:  rc = opts->apply == FMX_APPLY_FUSED ? sgd_epoch_fused(h, s, opts, hy, &n) : epoch_split(h, s, opts, &n); break;
    default: return fail(h, FMX_E_ARG, "unknown SGD mode %d", opts->mode);
  }
  if (rc) return rc;
  return epoch_close(h, s, opts, bi, n, stats);
}

// ---------------------------------------------------------------------------------------------
// SGDA
// ---------------------------------------------------------------------------------------------
extern "C++" void sgda_free(fmx_handle h) {
  if (h->sgda.gw) fmx_dev_free(h->sgda.gw);
  if (h->sgda.gv) fmx_dev_free(h->sgda.gv);
  if (h->sgda.reg) fmx_dev_free(h->sgda.reg);
  if (h->sgda.dreg) fmx_dev_free(h->sgda.dreg);
  h->sgda = SgdaState();
}

int fmx_sgda_end(fmx_handle h) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_sgda_end"); if (_sr) return _sr; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  sgda_free(h);
  return FMX_OK;
}

int fmx_sgda_begin(fmx_handle h) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_sgda_begin"); if (_sr) return _sr; }
  touch_w(h);
  if (!h) return FMX_E_ARG;
  if (h->adapt.nv) return fail(h, FMX_E_STATE, "fmx_sgda_begin: an fmx_adapt session is open (call fmx_adapt_end first)");
  if (h->ftrl.nv) return fail(h, FMX_E_STATE, "fmx_sgda_begin: an fmx_ftrl session is open (call fmx_ftrl_end first)");
  if (h->cfg.shard_world > 1) return fail(h, FMX_E_UNSUPPORTED, "SGDA on a feature shard is not implemented");
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  sgda_free(h);
  const size_t nv = h->n_local * (size_t)h->tb.rs, nreg = (size_t)h->num_groups * (1 + (size_t)h->KP);   // [G][1 + KP]
  HIPCHK(h, fmx_dev_alloc(&h->sgda.gw, h->n_local * sizeof(float)));
  HIPCHK(h, fmx_dev_alloc(&h->sgda.gv, nv * sizeof(float)));
  HIPCHK(h, fmx_dev_alloc(&h->sgda.reg, nreg * sizeof(double)));
  HIPCHK(h, hipMemsetAsync(h->sgda.gw, 0, h->n_local * sizeof(float), h->stream));
  HIPCHK(h, hipMemsetAsync(h->sgda.gv, 0, nv * sizeof(float), h->stream));
  HIPCHK(h, hipMemsetAsync(h->sgda.reg, 0, nreg * sizeof(double), h->stream));
  // fm->w.init(0) (:256): the linear weights restart from zero
  if (h->tb.ws == 1) HIPCHK(h, hipMemsetAsync(h->tb.w, 0, h->n_local * sizeof(float), h->stream));
  else HIPCHK(h, hipMemset2DAsync(h->tb.w, (size_t)h->tb.ws * sizeof(float), 0, sizeof(float), h->n_local, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return FMX_OK;
}

int fmx_sgda_get_reg(fmx_handle h, double* reg) {
  if (!h || !reg) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_sgda_get_reg"); if (_sr) return _sr; }
  if (!h->sgda.reg) return fail(h, FMX_E_STATE, "fmx_sgda_get_reg before fmx_sgda_begin");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t G = h->num_groups, k = (size_t)h->cfg.num_factor, KP = (size_t)h->KP;
  std::vector<double> dev(G * (1 + KP));
  HIPCHK(h, hipMemcpyAsync(dev.data(), h->sgda.reg, dev.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t g = 0; g < G; g++) memcpy(reg + g * (1 + k), dev.data() + g * (1 + KP), (1 + k) * sizeof(double));
  return FMX_OK;
}

int fmx_sgda_epoch(fmx_handle h, int train_slot, int validation_slot, int do_lambda_steps, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_sgda_epoch"); if (_sr) return _sr; }
  touch_w(h);
  int rc = check_slot(h, train_slot, true);
  if (rc) return rc;
  rc = check_slot(h, validation_slot, true);
  if (rc) return rc;
  if (!h->sgda.reg) return fail(h, FMX_E_STATE, "fmx_sgda_epoch before fmx_sgda_begin");
  rc = refuse_weighted(h, train_slot, "fmx_sgda_epoch"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[train_slot];
  const Slot& v = h->slots[validation_slot];
  if (!s.blocks.empty() || !v.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "relations are not supported with SGD");   // fm_learn_sgd.h:61-63
  const Hyper hy = make_hyper(h->cfg);
  if (stats) memset(stats, 0, sizeof(*stats));
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  if (h->num_groups <= 1) {
    KP_SWITCH(h->KP, hipLaunchKernelGGL((k_sgda<KP, false>), dim3(1), dim3(64), 0, h->stream, s.ent, s.row_ptr, s.target, s.n_rows,
                                          v.ent, v.row_ptr, v.target, v.n_rows, h->tb, h->sgda.gw, h->sgda.gv, hy, h->w0,
                                          h->sgda.reg, do_lambda_steps, nullptr, 1u));
  } else {
    // LDS tables of k_sgda<KP, true>: regw[G] regv[G][KP] lwg[G] sfg[G][KP] sdfg[G][KP] (doubles) + stamp[G] (u32)
    const size_t G = h->num_groups, lds = (2 * G + 3 * G * (size_t)h->KP) * sizeof(double) + G * sizeof(uint32_t);
    const size_t lds_max = h->prop.sharedMemPerBlock ? h->prop.sharedMemPerBlock : 64 * 1024;
    if (lds > lds_max)
      return fail(h, FMX_E_UNSUPPORTED, "SGDA: %zu attribute groups x %d factors need %zu bytes of LDS (limit %zu)", G, h->KP, lds, lds_max);
    KP_SWITCH(h->KP, hipLaunchKernelGGL((k_sgda<KP, true>), dim3(1), dim3(64), lds, h->stream, s.ent, s.row_ptr, s.target, s.n_rows,
                                          v.ent, v.row_ptr, v.target, v.n_rows, h->tb, h->sgda.gw, h->sgda.gv, hy, h->w0,
                                          h->sgda.reg, do_lambda_steps, h->grp, (uint32_t)G));
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (stats) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    stats->rows = s.n_rows; stats->batches = s.n_rows; stats->device_seconds = ms * 1e-3;
    stats->main_kernel_seconds = stats->device_seconds; stats->main_kernel_launches = 1;
  }
  return FMX_OK;
}

// the batch form of the learner (oracle fmo_sgda_epoch_minibatch): per batch of `batch` train rows the theta step as a
// minibatch rule, then -- do_lambda_steps -- the lambda steps of the next `batch` validation rows, summed and applied once
int fmx_sgda_epoch_minibatch(fmx_handle h, int train_slot, int validation_slot, int do_lambda_steps, uint32_t batch,
                             uint32_t w0_chunk, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_sgda_epoch_minibatch"); if (_sr) return _sr; }
  touch_w(h);
  int rc = check_slot(h, train_slot, true);
  if (rc) return rc;
  rc = check_slot(h, validation_slot, true);
  if (rc) return rc;
  if (!h->sgda.reg) return fail(h, FMX_E_STATE, "fmx_sgda_epoch_minibatch before fmx_sgda_begin");
  rc = refuse_weighted(h, train_slot, "fmx_sgda_epoch_minibatch"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[train_slot];
  const Slot& v = h->slots[validation_slot];
  if (stats) memset(stats, 0, sizeof(*stats));
  if (s.n_rows == 0) return FMX_OK;
  if (!s.blocks.empty() || !v.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "relations are not supported with SGD");   // fm_learn_sgd.h:61-63
  Hyper hy = make_hyper(h->cfg);
  hy.sgda = 1; hy.reg0 = 0.f; hy.reg0_d = 0.0;                  // reg_0 = 0 (:100, :149)
  // batch 0: the default cut to the rows' stability bound; this learner's regression multiplier is 2 (p - y): twice the curvature
  fmx_batch_info bi;
  rc = ensure_coll_mass(h, s);
  if (rc) return rc;
  resolve_batch(h->cfg, s.coll_mass, batch, FMX_DEFAULT_BATCH, h->cfg.task == FMX_TASK_REGRESSION ? 2.0 : 1.0, &bi);
  const uint32_t B = bi.batch;
  // micro-chunk of the bias: this learner's regression multiplier is 2 (p - y), i.e. twice the curvature of plain SGD
  uint32_t chunk = w0_chunk ? w0_chunk : std::max<uint32_t>(1u, default_w0_chunk(h->cfg) / (h->cfg.task == FMX_TASK_REGRESSION ? 2u : 1u));
  rc = ensure_segments(h, s, B);
  if (rc) return rc;
  const uint32_t Bc = std::min<uint32_t>(B, s.n_rows);
  rc = ensure_scratch(h, Bc, 0);
  if (rc) return rc;
  const size_t G = h->num_groups, cells = G * (1 + (size_t)h->KP);
  const bool grouped = G > 1;                                    // one group: the row's tables and the workgroup's sums live in registers
  const size_t lds = grouped ? (G + 2 * G * (size_t)h->KP + cells) * sizeof(double) : 0;
  if (do_lambda_steps && lds > 64 * 1024)
    return fail(h, FMX_E_UNSUPPORTED, "SGDA batch form: %zu attribute groups x %d factors need %zu bytes of LDS per validation row (limit 65536)", G, h->KP, lds);
  // workgroups of the lambda step (one partial [G][1 + KP] each, summed in a fixed order by k_sgda_reg_update)
  const uint32_t n_wg = (uint32_t)std::max<size_t>(64, std::min<size_t>(4096, ((size_t)8 << 20) / cells));
  if (do_lambda_steps && h->sgda.dreg_cap < (size_t)n_wg * cells) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->sgda.dreg) { fmx_dev_free(h->sgda.dreg); h->sgda.dreg = nullptr; h->sgda.dreg_cap = 0; }
    HIPCHK(h, fmx_dev_alloc(&h->sgda.dreg, (size_t)n_wg * cells * sizeof(double)));
    h->sgda.dreg_cap = (size_t)n_wg * cells;
  }
  hipStream_t st = h->stream;
  HIPCHK(h, hipEventRecord(h->ev0, st));
  uint64_t vpos = 0, batches = 0;                                // validation->data->begin() at the start of the epoch (:266)
  for (uint64_t row0 = 0; row0 < s.n_rows; row0 += B) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>(B, s.n_rows - row0);
    float* S = h->partial;
    float* rest = S + (size_t)nb * h->KP;
    KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, true, true>), nb, st, s.ent, s.row_ptr, row0, nb, RowsF32{h->tb}, h->cfg.k1, S, rest));
    rc = launch_scan(h, rest, s.target + row0, nb, chunk, hy, h->mult, st);
    if (rc) return rc;
    const SegWork sw = seg_work_dense(h, s, (size_t)(row0 / B), S, h->mult);
    if (sw.nseg) {
      KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_sgda_apply_seg<KP, 8>), ((uint64_t)sw.nseg + 63) / 64, st, sw, h->tb, hy,
                                         (const double*)h->sgda.reg, (const uint32_t*)h->grp, h->sgda.gw, h->sgda.gv));
    }
    if (do_lambda_steps && v.n_rows) {
      const uint32_t wg = std::min<uint32_t>(nb, n_wg);
      if (grouped) { KP_SWITCH(h->KP, hipLaunchKernelGGL((k_sgda_lambda<KP, true>), dim3(wg), dim3(64), lds, st, v.ent, v.row_ptr, v.target,
                                            v.n_rows, (uint32_t)vpos, nb, h->tb, (const float*)h->sgda.gw, (const float*)h->sgda.gv, hy,
                                            (const double*)h->w0, (const double*)h->sgda.reg, h->sgda.dreg, (const uint32_t*)h->grp, (uint32_t)G)); }
      else         { KP_SWITCH(h->KP, hipLaunchKernelGGL((k_sgda_lambda<KP, false>), dim3(wg), dim3(64), 0, st, v.ent, v.row_ptr, v.target,
                                            v.n_rows, (uint32_t)vpos, nb, h->tb, (const float*)h->sgda.gw, (const float*)h->sgda.gv, hy,
                                            (const double*)h->w0, (const double*)h->sgda.reg, h->sgda.dreg, (const uint32_t*)h->grp, (uint32_t)G)); }
      hipLaunchKernelGGL(k_sgda_reg_update, dim3((unsigned)std::min<size_t>(cells, 1024)), dim3(256), 0, st, h->sgda.reg, (const double*)h->sgda.dreg,
                         wg, (uint32_t)cells, h->KP, h->cfg.k1);
      vpos = (vpos + nb) % v.n_rows;
    }
    HIPCHK(h, hipGetLastError());
    batches++;
  }
  HIPCHK(h, hipEventRecord(h->ev1, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (stats) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    stats->rows = s.n_rows; stats->batches = batches; stats->device_seconds = ms * 1e-3;
    stats->main_kernel_seconds = stats->device_seconds; stats->main_kernel_launches = batches;
    stats->max_feature_count = s.max_seg_count;
    stats->batch_used = bi.batch; stats->collision_mass = bi.collision_mass; stats->batch_gain = bi.batch_gain; stats->status = bi.status;
  }
  return FMX_OK;
}

// ---------------------------------------------------------------------------------------------
// AdaGrad on the minibatch rule (include/fmx.h "fmx_adapt_*"; the owner kernel is fmx_adapt_kernels.h)
// ---------------------------------------------------------------------------------------------
extern "C++" void adapt_free(fmx_handle h) {
  if (h->adapt.nw) fmx_dev_free(h->adapt.nw);
  if (h->adapt.nv) fmx_dev_free(h->adapt.nv);
  h->adapt = AdaptState();
}

// what every fmx_adapt_* entry point refuses whatever the session's state
static int adapt_check_handle(fmx_handle h, const char* what) {
  if (h->cfg.shard_world > 1 || h->comm || (h->group && !h->owns_group))
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", what);
  return FMX_OK;
}

extern "C++" int adapt_tables(fmx_handle h, const char* who) {
  if (h->adapt.nv) return FMX_OK;
  const size_t nv = h->n_local * (size_t)h->tb.rs;
  HIPCHK(h, fmx_dev_alloc(&h->adapt.nw, h->n_local * sizeof(float)));
  hipError_t e = fmx_dev_alloc(&h->adapt.nv, nv * sizeof(float));
  if (e != hipSuccess) { adapt_free(h); return fail(h, FMX_E_HIP, "%s: the accumulator table (%zu bytes): %s", who, nv * sizeof(float), hipGetErrorString(e)); }
  return FMX_OK;
}

extern "C++" int adapt_start_state(fmx_handle h) {
  const size_t nv = h->n_local * (size_t)h->tb.rs;
  hipLaunchKernelGGL(k_adapt_fill, dim3((unsigned)std::min<size_t>((h->n_local + 255) / 256, 2048)), dim3(256), 0, h->stream, h->adapt.nw, (uint64_t)h->n_local, h->adapt.init_acc);
  hipLaunchKernelGGL(k_adapt_fill, dim3((unsigned)std::min<size_t>((nv + 255) / 256, 2048)), dim3(256), 0, h->stream, h->adapt.nv, (uint64_t)nv, h->adapt.init_acc);
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// fmx_adapt_begin in two halves, so that fmx_group_adapt_begin (fmx_comm.hip) can refuse for every member before it opens a session on
// any: adapt_begin_check is every refusal (no device work; in_group: the handle is a member of the group that asks, so the handle-kind
// refusal is the group's business), adapt_begin_open the tables and the start state
extern "C++" int adapt_begin_check(fmx_handle h, const fmx_adapt_opts* opts, bool in_group, float* init_acc_out) {
  if (!h) return FMX_E_ARG;
  if (!opts) return fail(h, FMX_E_ARG, "fmx_adapt_begin: opts is NULL");
  if (opts->rule != FMX_ADAPT_ADAGRAD) return fail(h, FMX_E_ARG, "fmx_adapt_begin: unknown rule %u", opts->rule);
  if (opts->flags != 0) return fail(h, FMX_E_ARG, "fmx_adapt_begin: flags must be 0");
  if (!(opts->init_acc >= 0.0) || std::isinf(opts->init_acc)) return fail(h, FMX_E_ARG, "fmx_adapt_begin: init_acc must be finite and >= 0 (0 = 1.0)");
  if (!(opts->learn_rate >= 0.0)) return fail(h, FMX_E_ARG, "fmx_adapt_begin: learn_rate must be >= 0 (0 = fmx_config::learn_rate)");
  if (!in_group) { int rc = adapt_check_handle(h, "fmx_adapt_begin"); if (rc) return rc; }
  if (h->sgda.reg) return fail(h, FMX_E_STATE, "fmx_adapt_begin: an SGDA session is open (call fmx_sgda_end first)");
  if (h->ftrl.nv) return fail(h, FMX_E_STATE, "fmx_adapt_begin: an fmx_ftrl session is open (call fmx_ftrl_end first)");
  const float init_acc = opts->init_acc > 0.0 ? (float)opts->init_acc : 1.0f;
  if (!(init_acc > 0.f) || std::isinf(init_acc)) return fail(h, FMX_E_ARG, "fmx_adapt_begin: init_acc %g is not a positive fp32 number", opts->init_acc);
  *init_acc_out = init_acc;
  return FMX_OK;
}
extern "C++" int adapt_begin_open(fmx_handle h, const fmx_adapt_opts* opts, float init_acc) {
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int rc = adapt_tables(h, "fmx_adapt_begin"); if (rc) return rc;   // (again = reset: the tables are there)
  h->adapt.eta = (float)(opts->learn_rate > 0.0 ? opts->learn_rate : h->cfg.learn_rate);
  h->adapt.init_acc = init_acc;
  rc = adapt_start_state(h); if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return FMX_OK;
}

int fmx_adapt_begin(fmx_handle h, const fmx_adapt_opts* opts) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_adapt_begin"); if (_sr) return _sr; }
  float init_acc = 0.f;
  int rc = adapt_begin_check(h, opts, false, &init_acc); if (rc) return rc;
  return adapt_begin_open(h, opts, init_acc);
}

// (in_group, here and below: the call comes from the group the handle is a member of -- fmx_group_adapt_* / fmx_group_ftrl_*,
// fmx_comm.hip; a member's session belongs to its group, so the per-handle entry points keep refusing it)
extern "C++" int adapt_end_impl(fmx_handle h, bool in_group) {
  if (!h) return FMX_E_ARG;
  if (!h->adapt.nv) return fail(h, FMX_E_STATE, "fmx_adapt_end before fmx_adapt_begin");
  if (!in_group) { int rc = adapt_check_handle(h, "fmx_adapt_end"); if (rc) return rc; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  adapt_free(h);
  return FMX_OK;
}
int fmx_adapt_end(fmx_handle h) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_adapt_end"); if (_sr) return _sr; }
  return adapt_end_impl(h, false);
}

// the gather of fmx_get_param_rows over nt state tables, one after the other: outs[t] = {the linear weights' state, the factors' state}
static int state_rows(fmx_handle h, const char* what, const uint32_t* ids, uint32_t count, const Tab* tabs, double* const (*outs)[2], int nt) {
  const Shard sh = make_shard(h->cfg);
  for (uint32_t i = 0; i < count; i++) {
    if (ids[i] >= h->cfg.num_attribute) return fail(h, FMX_E_ARG, "feature id %u >= num_attribute", ids[i]);
    if (!sh.owns(ids[i])) return fail(h, FMX_E_ARG, "feature id %u is not on this shard", ids[i]);   // (the group routes every id to its owner)
  }
  if (count == 0) return FMX_OK;
  return gather_rows(h, what, ids, count, nt, outs, [&](int t, dim3 grid, const uint32_t* d_ids, double* d_w, double* d_v) {
    hipLaunchKernelGGL(k_fetch_rows<RowsF32>, grid, dim3(256), 0, h->stream, d_ids, count, h->cfg.num_factor, sh, RowsF32{tabs[t]}, d_w, d_v);
  });
}

extern "C++" int adapt_state_rows_impl(fmx_handle h, bool in_group, const uint32_t* ids, uint32_t count, double* nw_out, double* nv_out) {
  if (!h) return FMX_E_ARG;
  if (!ids || !nw_out || (h->cfg.num_factor > 0 && !nv_out)) return fail(h, FMX_E_ARG, "fmx_adapt_get_state_rows: ids / nw_out / nv_out is NULL");
  if (!h->adapt.nv) return fail(h, FMX_E_STATE, "fmx_adapt_get_state_rows before fmx_adapt_begin");
  if (!in_group) { int rc = adapt_check_handle(h, "fmx_adapt_get_state_rows"); if (rc) return rc; }
  const Tab tabs[1] = {Tab{h->adapt.nv, h->adapt.nw, h->tb.rs, 1u}};
  double* const outs[1][2] = {{nw_out, nv_out}};
  return state_rows(h, "fmx_adapt_get_state_rows", ids, count, tabs, outs, 1);
}
int fmx_adapt_get_state_rows(fmx_handle h, const uint32_t* ids, uint32_t count, double* nw_out, double* nv_out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_adapt_get_state_rows"); if (_sr) return _sr; }
  return adapt_state_rows_impl(h, false, ids, count, nw_out, nv_out);
}

// step 2 of a batch on a slot with weights (include/fmx.h "fmx_set_row_weights"): k_scan_weighted, the one-wavefront chain with
// mult_e = c_e * multiplier, on the caller's stream.  Never parallel in time, whatever the batch; without k0 the micro-chunk means
// nothing and the batch is one chunk.  Micro-chunks of 16 / 32 / 64 examples (the defaults) take the kernel's sub-piece form.
static int launch_scan_weighted(fmx_handle h, const float* rest, const float* target, const float* weight, uint32_t n_rows, uint32_t chunk,
                                const Hyper& hy, float* mult, hipStream_t st) {
  h->run_status |= FMX_STAT_WEIGHTED | FMX_STAT_SCAN_SERIAL;
  const uint32_t ch = hy.k0 ? chunk : n_rows;
  const uint32_t sub = (hy.k0 && (chunk == 16u || chunk == 32u || chunk == 64u)) ? chunk : 0u;   // the sub-piece form of the default micro-chunks
#define FMX_SCANW(TK, CH) hipLaunchKernelGGL((k_scan_weighted<TK, CH>), dim3(1), dim3(64), 0, st, rest, target, weight, n_rows, ch, hy, h->w0, mult)
#define FMX_SCANW_CH(TK) do { if (sub == 16u) FMX_SCANW(TK, 16); else if (sub == 32u) FMX_SCANW(TK, 32); \
                              else if (sub == 64u) FMX_SCANW(TK, 64); else FMX_SCANW(TK, 0); } while (0)
  if (hy.task == 0) FMX_SCANW_CH(0); else FMX_SCANW_CH(1);
#undef FMX_SCANW_CH
#undef FMX_SCANW
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// one epoch of an optimiser that keeps per-coordinate state (AdaGrad, FTRL), after its entry point's own session checks: per batch the
// batch rule's row sums and bias recurrence (fmx_sgda_epoch_minibatch's three launches), then launch_owner(sw, hy, st) starts the one
// kernel in which an owner per (batch, feature) segment takes the rule's step.  The bias stays plain SGD at fmx_config::learn_rate.
extern "C++" {
// the tail of one batch, shared by stateful_epoch and the group driver's shard step (stateful_shard_step): from the batch's factor sums S
// and rest[] -- the handle's own (k_rowsums) or derived from the exchanged sums of the shards -- the bias recurrence with the
// multipliers into h->mult, then the owner kernel over the (batch, feature) segments the handle holds of batch row0 / B
template <class Owner>
static int stateful_batch_tail(fmx_handle h, const Slot& s, uint64_t row0, uint32_t nb, uint32_t B, uint32_t chunk, const Hyper& hy,
                               const float* S, const float* rest, hipStream_t st, Owner launch_owner) {
  int rc = s.weighted ? launch_scan_weighted(h, rest, s.target + row0, s.weight + row0, nb, chunk, hy, h->mult, st)
                      : launch_scan(h, rest, s.target + row0, nb, chunk, hy, h->mult, st);
  if (rc) return rc;
  const SegWork sw = seg_work_dense(h, s, (size_t)(row0 / B), S, h->mult);
  if (sw.nseg) { rc = launch_owner(sw, hy, st); if (rc) return rc; }
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

template <class Owner>
static int stateful_epoch(fmx_handle h, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats, Owner launch_owner) {
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[slot];
  if (stats) memset(stats, 0, sizeof(*stats));
  if (s.n_rows == 0) return FMX_OK;
  if (!s.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "relations are not supported with SGD");   // fm_learn_sgd.h:61-63
  h->setup_acc = 0.0; h->run_status = 0;
  const Hyper hy = make_hyper(h->cfg);
  // batch 0: fmx_sgd_epoch's choice (the plain rule's stability cut, curvature factor 1): conservative on purpose -- the step is bounded
  // by eta whatever the batch, but whether a larger default pays is a measurement, not this function's decision
  fmx_batch_info bi;
  int rc = ensure_coll_mass(h, s); if (rc) return rc;
  resolve_batch(h->cfg, s.coll_mass, batch, FMX_DEFAULT_BATCH, 1.0, &bi);
  const uint32_t B = bi.batch;
  const uint32_t chunk = w0_chunk ? w0_chunk : default_w0_chunk(h->cfg);
  rc = ensure_segments(h, s, B); if (rc) return rc;
  const uint32_t Bc = std::min<uint32_t>(B, s.n_rows);
  rc = ensure_scratch(h, Bc, 0); if (rc) return rc;
  touch_w(h);                                                   // (a side stream kept by FMX_FLAG_KEEP_WSIDE is stale from here on)
  hipStream_t st = h->stream;
  HIPCHK(h, hipEventRecord(h->ev0, st));
  uint64_t batches = 0;
  for (uint64_t row0 = 0; row0 < s.n_rows; row0 += B) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>(B, s.n_rows - row0);
    float* S = h->partial;
    float* rest = S + (size_t)nb * h->KP;
    KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, true, true>), nb, st, s.ent, s.row_ptr, row0, nb, RowsF32{h->tb}, h->cfg.k1, S, rest));
    rc = stateful_batch_tail(h, s, row0, nb, B, chunk, hy, S, rest, st, launch_owner); if (rc) return rc;
    batches++;
  }
  HIPCHK(h, hipEventRecord(h->ev1, st));
  HIPCHK(h, hipStreamSynchronize(st));
  rc = scan_error_check(h); if (rc) return rc;
  if (stats) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    stats->rows = s.n_rows; stats->batches = batches; stats->device_seconds = ms * 1e-3;
    stats->main_kernel_seconds = stats->device_seconds; stats->main_kernel_launches = batches;
    stats->max_feature_count = s.max_seg_count;
    stats->batch_used = bi.batch; stats->collision_mass = bi.collision_mass; stats->batch_gain = bi.batch_gain;
    stats->status = bi.status | h->run_status;
    stats->w0_chunk_used = chunk;
    stats->setup_seconds = h->setup_acc;
  }
  return FMX_OK;
}
}  // extern "C++"

// the owner kernels of the two rules on the handle's own tables (a shard's: n_local rows, local feature ids)
static int launch_adapt_owner(fmx_handle h, const SegWork& sw, const Hyper& hy, hipStream_t st) {
  const AdagradRule rule{{Tab{h->adapt.nv, h->adapt.nw, h->tb.rs, 1u}}, h->adapt.eta};
  KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_adapt_apply_seg<KP, AdaptU<KP>::value>), ((uint64_t)sw.nseg + 63) / 64, st, sw, h->tb, rule, hy));
  return FMX_OK;
}
static int launch_ftrl_owner(fmx_handle h, const SegWork& sw, const Hyper& hy, hipStream_t st) {
  const FtrlState& fs = h->ftrl;
  const FtrlRule rule{{Tab{fs.zv, fs.zw, h->tb.rs, 1u}, Tab{fs.nv, fs.nw, h->tb.rs, 1u}}, FtrlHyper{fs.inv_alpha, fs.beta, fs.l1_w, fs.l1_v, fs.l2_w, fs.l2_v}};
  KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_ftrl_apply_seg<KP, FtrlU<KP>::value>), ((uint64_t)sw.nseg + 63) / 64, st, sw, h->tb, rule, hy));
  return FMX_OK;
}

extern "C++" int adapt_epoch_impl(fmx_handle h, bool in_group, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats) {
  int rc = check_slot(h, slot, true);
  if (rc) return rc;
  if (!h->adapt.nv) return fail(h, FMX_E_STATE, "fmx_adapt_epoch before fmx_adapt_begin");
  if (!in_group) { rc = adapt_check_handle(h, "fmx_adapt_epoch"); if (rc) return rc; }
  if (h->sgda.reg) return fail(h, FMX_E_STATE, "fmx_adapt_epoch: an SGDA session is open (call fmx_sgda_end first)");
  rc = slot_in_session(h, slot, "fmx_adapt_epoch"); if (rc) return rc;
  return stateful_epoch(h, slot, batch, w0_chunk, stats, [&](const SegWork& sw, const Hyper& hy, hipStream_t st) -> int {
    return launch_adapt_owner(h, sw, hy, st);
  });
}
int fmx_adapt_epoch(fmx_handle h, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_adapt_epoch"); if (_sr) return _sr; }
  return adapt_epoch_impl(h, false, slot, batch, w0_chunk, stats);
}

// ---- one shard's share of a stateful epoch over feature shards (fmx_group_adapt_epoch / fmx_group_ftrl_epoch, fmx_comm.hip) ----
// The driver has checked the group, the slot and the session on every member.  stateful_shard_prepare: what stateful_epoch does in
// front of its loop (the bias back in h->w0, the shard's segments for batch B, its scratch).  stateful_shard_step: steps 3 - 6 of a batch
// on the shard's own stream from the EXCHANGED sums d_sum ([nb][KP] factor sums, then [nb] scalars) -- rest_e, then the batch tail of
// stateful_epoch with the owner kernel of `rule` on the shard's tables.  Every shard runs the same recurrence from the same sums.
extern "C++" int stateful_shard_prepare(fmx_handle h, int slot, uint32_t B) {
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[slot];
  int rc = ensure_segments(h, s, B); if (rc) return rc;
  const uint32_t Bc = std::min<uint32_t>(B, std::max<uint32_t>(s.n_rows, 1u));
  rc = ensure_scratch(h, Bc, Bc); if (rc) return rc;
  touch_w(h);
  return FMX_OK;
}
extern "C++" int stateful_shard_step(fmx_handle h, int slot, StatefulRule rule, uint64_t row0, uint32_t nb, uint32_t B, uint32_t chunk, const float* d_sum) {
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  if (nb == 0 || row0 + nb > s.n_rows || nb > h->cap || nb > h->cap_rest) return fail(h, FMX_E_ARG, "stateful_shard_step: rows outside the slot or the scratch");
  const Hyper hy = make_hyper(h->cfg);
  hipStream_t st = h->stream;
  const float* S = d_sum;
  const float* c = d_sum + (size_t)nb * h->KP;
  KP_SWITCH(h->KP, hipLaunchKernelGGL((k_rest_from_partial<KP>), dim3(wave_grid((nb + Map<KP>::EPI - 1) / Map<KP>::EPI)), dim3(256), 0, st, S, c, nb, h->rest));
  HIPCHK(h, hipGetLastError());
  return stateful_batch_tail(h, s, row0, nb, B, chunk, hy, S, h->rest, st, [&](const SegWork& sw, const Hyper& hyp, hipStream_t stp) -> int {
    return rule == STATEFUL_FTRL ? launch_ftrl_owner(h, sw, hyp, stp) : launch_adapt_owner(h, sw, hyp, stp);
  });
}

// ---------------------------------------------------------------------------------------------
// FTRL-proximal with L1 on the minibatch rule (include/fmx.h "fmx_ftrl_*"; the kernels are fmx_ftrl_kernels.h)
// ---------------------------------------------------------------------------------------------
extern "C++" void ftrl_free(fmx_handle h) {
  if (h->ftrl.zw) fmx_dev_free(h->ftrl.zw);
  if (h->ftrl.zv) fmx_dev_free(h->ftrl.zv);
  if (h->ftrl.nw) fmx_dev_free(h->ftrl.nw);
  if (h->ftrl.nv) fmx_dev_free(h->ftrl.nv);
  h->ftrl = FtrlState();
}

static bool ftrl_value_ok(double x) { return x >= 0.0 && !std::isinf(x); }                  // (NaN fails the comparison)

extern "C++" int ftrl_tables(fmx_handle h, const char* who) {
  if (h->ftrl.nv) return FMX_OK;
  const size_t nv = h->n_local * (size_t)h->tb.rs, nw = h->n_local;
  hipError_t e = fmx_dev_alloc(&h->ftrl.zw, nw * sizeof(float));
  if (e == hipSuccess) e = fmx_dev_alloc(&h->ftrl.nw, nw * sizeof(float));
  if (e == hipSuccess) e = fmx_dev_alloc(&h->ftrl.zv, nv * sizeof(float));
  if (e == hipSuccess) e = fmx_dev_alloc(&h->ftrl.nv, nv * sizeof(float));
  if (e != hipSuccess) { ftrl_free(h); return fail(h, FMX_E_HIP, "%s: the z and n tables (%zu bytes): %s", who, 2 * (nv + nw) * sizeof(float), hipGetErrorString(e)); }
  return FMX_OK;
}

extern "C++" int ftrl_start_state(fmx_handle h) {
  const FtrlState& f = h->ftrl;
  const size_t nv = h->n_local * (size_t)h->tb.rs, nw = h->n_local;
  hipLaunchKernelGGL(k_ftrl_init, dim3((unsigned)std::min<size_t>((nw + 255) / 256, 2048)), dim3(256), 0, h->stream, (const float*)h->tb.w, (size_t)h->tb.ws,
                     f.zw, f.nw, (uint64_t)nw, f.start_D(f.l2_w), f.l1_w, f.init_acc);
  hipLaunchKernelGGL(k_ftrl_init, dim3((unsigned)std::min<size_t>((nv + 255) / 256, 2048)), dim3(256), 0, h->stream, (const float*)h->tb.V, (size_t)1,
                     f.zv, f.nv, (uint64_t)nv, f.start_D(f.l2_v), f.l1_v, f.init_acc);
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// fmx_ftrl_begin in two halves, as fmx_adapt_begin: ftrl_begin_check is every refusal and leaves the rule's constants in *out (its table
// pointers null), ftrl_begin_open the tables and the start state
extern "C++" int ftrl_begin_check(fmx_handle h, const fmx_ftrl_opts* opts, bool in_group, FtrlState* out) {
  if (!h) return FMX_E_ARG;
  if (!opts) return fail(h, FMX_E_ARG, "fmx_ftrl_begin: opts is NULL");
  if (opts->flags != 0) return fail(h, FMX_E_ARG, "fmx_ftrl_begin: flags must be 0");
  if (!ftrl_value_ok(opts->alpha) || !ftrl_value_ok(opts->beta) || !ftrl_value_ok(opts->l1_w) || !ftrl_value_ok(opts->l1_v) ||
      !ftrl_value_ok(opts->l2_w) || !ftrl_value_ok(opts->l2_v) || !ftrl_value_ok(opts->init_acc))
    return fail(h, FMX_E_ARG, "fmx_ftrl_begin: alpha, beta, l1, l2 and init_acc must be finite and >= 0");
  if (opts->beta == 0.0 && opts->init_acc == 0.0) return fail(h, FMX_E_ARG, "fmx_ftrl_begin: beta = 0 needs init_acc > 0 (D would start at 0)");
  const double alpha_d = opts->alpha > 0.0 ? opts->alpha : h->cfg.learn_rate;
  const float alpha = (float)alpha_d, inv_alpha = 1.0f / alpha;
  if (!(alpha > 0.f) || std::isinf(alpha) || std::isinf(inv_alpha))
    return fail(h, FMX_E_ARG, "fmx_ftrl_begin: alpha %g (and its reciprocal) must be a positive fp32 number", alpha_d);
  FtrlState f;
  f.inv_alpha = inv_alpha; f.beta = (float)opts->beta;
  f.l1_w = (float)opts->l1_w; f.l1_v = (float)opts->l1_v; f.l2_w = (float)opts->l2_w; f.l2_v = (float)opts->l2_v;
  const float init_acc = f.init_acc = (float)opts->init_acc;
  const float base = (f.beta + sqrtf(init_acc)) * inv_alpha;     // (FtrlState::start_D is this expression + l2)
  if (std::isinf(f.beta) || std::isinf(f.l1_w) || std::isinf(f.l1_v) || std::isinf(init_acc) || std::isinf(base + f.l2_w) || std::isinf(base + f.l2_v) ||
      !(base + f.l2_w > 0.f) || !(base + f.l2_v > 0.f))
    return fail(h, FMX_E_ARG, "fmx_ftrl_begin: the options leave the fp32 range ((beta + sqrt(init_acc)) / alpha + l2 = %g)", (double)(base + f.l2_v));
  if (!in_group) { int rc = adapt_check_handle(h, "fmx_ftrl_begin"); if (rc) return rc; }
  if (h->sgda.reg) return fail(h, FMX_E_STATE, "fmx_ftrl_begin: an SGDA session is open (call fmx_sgda_end first)");
  if (h->adapt.nv) return fail(h, FMX_E_STATE, "fmx_ftrl_begin: an fmx_adapt session is open (call fmx_adapt_end first)");
  *out = f;
  return FMX_OK;
}
extern "C++" int ftrl_begin_open(fmx_handle h, const FtrlState& constants) {
  FtrlState f = constants;
  { int _rc = lag_flush(h); if (_rc) return _rc; }              // (z is derived from the parameters: they have to be current)
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int rc = ftrl_tables(h, "fmx_ftrl_begin"); if (rc) return rc; // (again = reset: the tables are there)
  f.zw = h->ftrl.zw; f.zv = h->ftrl.zv; f.nw = h->ftrl.nw; f.nv = h->ftrl.nv;
  h->ftrl = f;
  rc = ftrl_start_state(h); if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return FMX_OK;
}

int fmx_ftrl_begin(fmx_handle h, const fmx_ftrl_opts* opts) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_ftrl_begin"); if (_sr) return _sr; }
  FtrlState f;
  int rc = ftrl_begin_check(h, opts, false, &f); if (rc) return rc;
  return ftrl_begin_open(h, f);
}

extern "C++" int ftrl_end_impl(fmx_handle h, bool in_group) {
  if (!h) return FMX_E_ARG;
  if (!h->ftrl.nv) return fail(h, FMX_E_STATE, "fmx_ftrl_end before fmx_ftrl_begin");
  if (!in_group) { int rc = adapt_check_handle(h, "fmx_ftrl_end"); if (rc) return rc; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ftrl_free(h);
  return FMX_OK;
}
int fmx_ftrl_end(fmx_handle h) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_ftrl_end"); if (_sr) return _sr; }
  return ftrl_end_impl(h, false);
}

extern "C++" int ftrl_state_rows_impl(fmx_handle h, bool in_group, const uint32_t* ids, uint32_t count, double* zw, double* zv, double* nw, double* nv) {
  if (!h) return FMX_E_ARG;
  if (!ids || !zw || !nw || (h->cfg.num_factor > 0 && (!zv || !nv))) return fail(h, FMX_E_ARG, "fmx_ftrl_get_state_rows: ids / zw / zv / nw / nv is NULL");
  if (!h->ftrl.nv) return fail(h, FMX_E_STATE, "fmx_ftrl_get_state_rows before fmx_ftrl_begin");
  if (!in_group) { int rc = adapt_check_handle(h, "fmx_ftrl_get_state_rows"); if (rc) return rc; }
  const Tab tabs[2] = {Tab{h->ftrl.zv, h->ftrl.zw, h->tb.rs, 1u}, Tab{h->ftrl.nv, h->ftrl.nw, h->tb.rs, 1u}};
  double* const outs[2][2] = {{zw, zv}, {nw, nv}};
  return state_rows(h, "fmx_ftrl_get_state_rows", ids, count, tabs, outs, 2);
}
int fmx_ftrl_get_state_rows(fmx_handle h, const uint32_t* ids, uint32_t count, double* zw, double* zv, double* nw, double* nv) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_ftrl_get_state_rows"); if (_sr) return _sr; }
  return ftrl_state_rows_impl(h, false, ids, count, zw, zv, nw, nv);
}

// one epoch: stateful_epoch with k_ftrl_apply_seg as the owner kernel.  regw / regv are not read (L2 lives in the proximal step).
extern "C++" int ftrl_epoch_impl(fmx_handle h, bool in_group, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats) {
  int rc = check_slot(h, slot, true);
  if (rc) return rc;
  if (!h->ftrl.nv) return fail(h, FMX_E_STATE, "fmx_ftrl_epoch before fmx_ftrl_begin");
  if (!in_group) { rc = adapt_check_handle(h, "fmx_ftrl_epoch"); if (rc) return rc; }
  if (h->sgda.reg || h->adapt.nv) return fail(h, FMX_E_STATE, "fmx_ftrl_epoch: an SGDA or fmx_adapt session is open");
  rc = slot_in_session(h, slot, "fmx_ftrl_epoch"); if (rc) return rc;
  return stateful_epoch(h, slot, batch, w0_chunk, stats, [&](const SegWork& sw, const Hyper& hy, hipStream_t st) -> int {
    return launch_ftrl_owner(h, sw, hy, st);
  });
}
int fmx_ftrl_epoch(fmx_handle h, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_ftrl_epoch"); if (_sr) return _sr; }
  return ftrl_epoch_impl(h, false, slot, batch, w0_chunk, stats);
}

// how many coordinates of the model are exactly zero (include/fmx.h "fmx_param_sparsity"): one pass of k_param_sparsity
// (in_group on a feature shard: the counts over the features the shard owns -- its table holds exactly those rows, rank r of W owning
// ceil((n - r) / W) of n; fmx_group_param_sparsity sums the shards' counts)
extern "C++" int param_sparsity_impl(fmx_handle h, bool in_group, fmx_sparsity* out) {
  if (!h) return FMX_E_ARG;
  if (!out) return fail(h, FMX_E_ARG, "fmx_param_sparsity: out is NULL");
  if (!in_group) { int rc = adapt_check_handle(h, "fmx_param_sparsity"); if (rc) return rc; }
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const uint64_t W = (uint64_t)std::max(h->cfg.shard_world, 1), R = (uint64_t)h->cfg.shard_rank;
  const uint64_t n = W > 1 ? (h->cfg.num_attribute > R ? (h->cfg.num_attribute - R + W - 1) / W : 0) : h->cfg.num_attribute;
  const int k = h->cfg.num_factor;
  unsigned long long host[4] = {0ull, 0ull, 0ull, 0ull};
  if (n) {
    unsigned long long* d = nullptr;
    HIPCHK(h, fmx_dev_alloc(&d, sizeof(host)));
    hipError_t er = hipMemsetAsync(d, 0, sizeof(host), h->stream);
    if (er == hipSuccess) {
      const uint32_t L = (uint32_t)std::min(h->KP, 64);          // lanes per feature: a power of two
      const uint64_t waves = (n + 64 / L - 1) / (64 / L);
      hipLaunchKernelGGL(k_param_sparsity, dim3((unsigned)std::min<uint64_t>((waves + 3) / 4, 8192)), dim3(256), 0, h->stream, h->tb, n, k, h->cfg.k1, L, d);
      er = hipGetLastError();
    }
    if (er == hipSuccess) er = hipMemcpyAsync(host, d, sizeof(host), hipMemcpyDeviceToHost, h->stream);
    if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
    fmx_dev_free(d);
    if (er != hipSuccess) return fail(h, FMX_E_HIP, "fmx_param_sparsity: %s", hipGetErrorString(er));
  }
  out->features = n; out->w_zero = host[0]; out->v_coords = n * (uint64_t)k; out->v_zero = host[1];
  out->v_zero_rows = host[2]; out->dead_features = host[3];
  return FMX_OK;
}
int fmx_param_sparsity(fmx_handle h, fmx_sparsity* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_param_sparsity"); if (_sr) return _sr; }
  return param_sparsity_impl(h, false, out);
}

}  // extern "C"
