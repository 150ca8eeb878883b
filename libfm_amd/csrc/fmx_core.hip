// fmx_core.hip -- C-ABI (include/fmx.h): lifetime, parameters, rows, predict / evaluate.
// The read side of every unit starts here: launch_rest, slot_scores, predict_out / evaluate_out (the model or the bf16 snapshot).
// Build: python -m libfm_amd.build   (hipcc --offload-arch=gfx950 -O3 -munsafe-fp-atomics -shared -fPIC)
//
// No CPU fallback lives in this library: every compute entry point needs a HIP device and fails with FMX_E_HIP
// otherwise.  Nothing here links or calls oracle/.
#include "fmx_internal.h"

static thread_local std::string g_create_error = "";

int fail(fmx_handle h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->err = buf; else g_create_error = buf;
  return code;
}

static int next_pow2(int k) { int p = 1; while (p < k) p <<= 1; return p; }

Hyper make_hyper(const fmx_config& c) {
  Hyper h;
  h.lr = (float)c.learn_rate; h.reg0 = (float)c.reg0; h.regw = (float)c.regw; h.regv = (float)c.regv;
  h.min_target = (float)c.min_target; h.max_target = (float)c.max_target;
  h.task = c.task; h.k0 = c.k0; h.k1 = c.k1;
  h.lr_d = c.learn_rate; h.reg0_d = c.reg0; h.regw_d = c.regw; h.regv_d = c.regv;
  h.min_d = c.min_target; h.max_d = c.max_target;
  h.sgda = 0;
  return h;
}

Shard make_shard(const fmx_config& c) {
  Shard sh;
  sh.n = c.num_attribute; sh.rank = (uint32_t)c.shard_rank; sh.world = (uint32_t)c.shard_world;
  sh.hashed = (c.shard_hash != 0 && c.shard_world > 1) ? 1u : 0u;
  uint32_t bits = 1; while (bits < 32 && (1ull << bits) < c.num_attribute) bits++;
  sh.half_bits = std::max<uint32_t>(1u, (bits + 1) / 2);         // 2 * half_bits >= bits: the Feistel domain covers [0, n)
  return sh;
}

// grid sizing: never more workgroups than the work needs, and at most `over` x what can be resident (the kernels stride
// over their work).  Which `over` is a measured per-family choice (scripts/gpu_ab_inprocess.py FMX_GRID_OVER a b <what>,
// alternating inside one process): the row-gather kernels of the SGD family want NO cap -- one workgroup per four examples and
// the dispatcher balancing them beats grid-stride workgroups (one-pass step: x1 -7 %, x2 0, x8 +1.7 %, uncapped +3.0 %; two-pass
// +5.9 %, hogwild +4.7 %, predict +3.2 %) -- while the column kernels of the ALS sweep lose 8 % uncapped and keep x2.
uint32_t resident_grid(fmx_handle h, const void* kernel, uint64_t n_waves_wanted, int over_default) {
  auto& cache = h->occ_cache;                 // per handle (= per device, one calling thread): no process-wide state
  auto it = cache.find(kernel);
  int occ;
  if (it == cache.end()) {
    occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, 256, 0) != hipSuccess || occ < 1) occ = 4;
    if (occ > 8) occ = 8;
    cache[kernel] = occ;
  } else {
    occ = it->second;
  }
  uint64_t blocks = (n_waves_wanted + 3) / 4;
  const int over = over_default;
  const uint64_t cap = (uint64_t)occ * (uint64_t)h->num_cu * (uint64_t)over;
  if (blocks < 1) blocks = 1;
  if (blocks > cap) blocks = cap;
  return (uint32_t)blocks;
}
int ensure_scratch(fmx_handle h, size_t batch_cap, size_t rest_cap) {
  if (batch_cap > h->cap) {
    if (h->partial) fmx_dev_free(h->partial);
    if (h->mult) fmx_dev_free(h->mult);
    h->partial = nullptr; h->mult = nullptr; h->cap = 0;
    HIPCHK(h, fmx_dev_alloc(&h->partial, batch_cap * (size_t)(h->KP + 1) * sizeof(float)));
    HIPCHK(h, fmx_dev_alloc(&h->mult, batch_cap * sizeof(float)));
    h->cap = batch_cap;
  }
  if (rest_cap > h->cap_rest) {
    if (h->rest) fmx_dev_free(h->rest);
    h->rest = nullptr; h->cap_rest = 0;
    HIPCHK(h, fmx_dev_alloc(&h->rest, rest_cap * sizeof(float)));
    h->cap_rest = rest_cap;
  }
  return FMX_OK;
}

int check_slot(fmx_handle h, int slot, bool need_target) {
  if (!h) return FMX_E_ARG;
  if (slot < 0 || slot >= FMX_MAX_SLOTS) return fail(h, FMX_E_ARG, "slot %d out of range", slot);
  if (!h->slots[slot].used) return fail(h, FMX_E_STATE, "slot %d holds no rows (call fmx_upload_rows first)", slot);
  if (need_target && !h->slots[slot].target) return fail(h, FMX_E_STATE, "slot %d was uploaded without targets", slot);
  return FMX_OK;
}

// an open ALS / MCMC session keeps device structures derived from its train slot (X^T segments, level lists, e/q of
// that size): the slot must not be replaced, freed or re-bucketed until fmx_als_end
int slot_in_session(fmx_handle h, int slot, const char* what) {
  if (h->als.slot >= 0 && h->als.slot == slot)
    return fail(h, FMX_E_STATE, "%s: slot %d is the train slot of an open ALS / MCMC session (call fmx_als_end first)", what, slot);
  return FMX_OK;
}

void free_segments(Slot& s) {
  if (s.t_ent) fmx_dev_free(s.t_ent);
  if (s.seg_feat) fmx_dev_free(s.seg_feat);
  if (s.seg_rel) fmx_dev_free(s.seg_rel);
  if (s.cmask) fmx_dev_free(s.cmask);
  if (s.cseg) fmx_dev_free(s.cseg);
  if (s.cdesc) fmx_dev_free(s.cdesc);
  if (s.d_batch_seg) fmx_dev_free(s.d_batch_seg);
  if (s.d_cbatch) fmx_dev_free(s.d_cbatch);
  if (s.d_batch_base) fmx_dev_free(s.d_batch_base);
  s.cdesc = nullptr; s.d_batch_seg = nullptr; s.d_cbatch = nullptr; s.d_batch_base = nullptr;
  s.t_ent = nullptr; s.seg_feat = nullptr; s.seg_rel = nullptr; s.seg_B = 0; s.nseg = 0;
  s.cmask = nullptr; s.cseg = nullptr; s.ncseg = 0; s.fused_cap = 0;
  s.batch_seg.clear(); s.batch_base.clear(); s.cbatch.clear();
}

void free_block(BlockRows* b) {
  if (!b) return;
  free_slot(b->rows);
  if (b->map) fmx_dev_free(b->map);
  if (b->brow_ptr) fmx_dev_free(b->brow_ptr);
  if (b->brow_list) fmx_dev_free(b->brow_list);
  if (b->pbuf) fmx_dev_free(b->pbuf);
  delete b;
}

void free_slot(Slot& s) {
  for (BlockRows* b : s.blocks) free_block(b);
  s.blocks.clear();
  free_segments(s);
  free_pairs(s);
  free_interactions(s);
  free_post(s);
  if (s.ent) fmx_dev_free(s.ent);
  if (s.row_ptr) fmx_dev_free(s.row_ptr);
  if (s.target) fmx_dev_free(s.target);
  if (s.wside) fmx_dev_free(s.wside);
  if (s.lmask) fmx_dev_free(s.lmask);
  if (s.ids) fmx_dev_free(s.ids);
  if (s.smask) fmx_dev_free(s.smask);
  if (s.soff) fmx_dev_free(s.soff);
  if (s.wtrain) fmx_dev_free(s.wtrain);
  if (s.qid) fmx_dev_free(s.qid);
  if (s.weight) fmx_dev_free(s.weight);
  s = Slot();
}

// the slot's weight side stream (row_sums, fmx_kernels.h): allocated and armed once -- every entry "gather", the flags of the entries
// that are the last occurrence of their feature in the slot -- and from then on kept current by the one-pass epochs run with
// FMX_FLAG_KEEP_WSIDE.  4 bytes per entry + 8 per row; temporary: 4 bytes per feature (at most 2^27 buckets).
int ensure_wside(fmx_handle h, Slot& s) {
  if (s.wside) return FMX_OK;
  if (s.nnz == 0 || s.nnz >= (1ull << 32) - 1) return FMX_OK;        // (entry indices + 1 live in 32 bits; such a slot simply keeps gathering)
  struct Acc { fmx_handle h; std::chrono::steady_clock::time_point t0;
               ~Acc() { h->setup_acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } } acc_{h, std::chrono::steady_clock::now()};
  const uint32_t M = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(h->n_local, 1), 1ull << 27);
  uint32_t* last = nullptr;
  hipError_t er = fmx_dev_alloc(&last, (size_t)M * 4);
  if (er == hipSuccess) er = fmx_dev_alloc(&s.wside, (size_t)s.nnz * 4);
  if (er == hipSuccess) er = fmx_dev_alloc(&s.lmask, (size_t)s.n_rows * 8);
  if (er == hipSuccess) er = hipMemsetAsync(last, 0, (size_t)M * 4, h->stream);
  if (er == hipSuccess) {
    hipLaunchKernelGGL(k_wside_last, dim3((unsigned)std::min<uint64_t>((s.nnz + 255) / 256, 8192)), dim3(256), 0, h->stream, s.ent, s.nnz, M, last);
    hipLaunchKernelGGL(k_wside_mask, dim3((unsigned)std::min<uint32_t>((s.n_rows + 3) / 4, 16384)), dim3(256), 0, h->stream, s.ent, s.row_ptr, s.n_rows, M,
                       (const uint32_t*)last, s.lmask, s.wside);
    er = hipGetLastError();
  }
  if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  if (last) fmx_dev_free(last);
  if (er != hipSuccess) {
    if (s.wside) fmx_dev_free(s.wside);
    if (s.lmask) fmx_dev_free(s.lmask);
    s.wside = nullptr; s.lmask = nullptr;
    return fail(h, FMX_E_HIP, "weight side stream of the slot: %s", hipGetErrorString(er));
  }
  s.wside_version = 0;
  if (getenv("FMX_TRACE_SETUP")) fprintf(stderr, "[fmx setup] weight side stream %8.3f ms\n", 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - acc_.t0).count());
  return FMX_OK;
}

// the slot's id-only stream (load_entry, fmx_kernels.h): where every row has the same length and every value is 1.0f -- one-hot field
// data, libFM's usual input -- the value half of the {id, value} entries carries nothing, and k_fused streams 4 bytes per entry instead of
// 8.  The rows of a slot never change between epochs (fm_learn_sgd_element.h:56), so it is built once, by the first one-pass epoch after an
// upload: one pass over the entries that copies the ids and looks at every value; one value that is not 1.0f and the stream is dropped.
// 4 bytes per entry stay resident until the slot is replaced or freed (free_slot).  Single handles only: a feature shard's rows vary.
int ensure_ids(fmx_handle h, Slot& s) {
  if (s.ids_asked) return FMX_OK;
  s.ids_asked = true;
  if (!h->ids || !s.fixed_nnz || s.nnz == 0 || h->cfg.shard_world != 1 || !s.blocks.empty()) return FMX_OK;
  if (s.nnz != (uint64_t)s.n_rows * s.fixed_nnz) return FMX_OK;
  struct Acc { fmx_handle h; std::chrono::steady_clock::time_point t0;
               ~Acc() { h->setup_acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } } acc_{h, std::chrono::steady_clock::now()};
  uint32_t* flag = nullptr;
  uint32_t not_one = 1u;
  hipError_t er = fmx_dev_alloc(&flag, 256);
  if (er == hipSuccess) er = fmx_dev_alloc(&s.ids, (size_t)s.nnz * 4);
  if (er == hipSuccess) er = hipMemsetAsync(flag, 0, 4, h->stream);
  if (er == hipSuccess) {
    hipLaunchKernelGGL(k_ids_build, dim3((unsigned)std::min<uint64_t>((s.nnz + 255) / 256, 8192)), dim3(256), 0, h->stream, s.ent, s.nnz, s.ids, flag);
    er = hipGetLastError();
  }
  if (er == hipSuccess) er = hipMemcpyAsync(&not_one, flag, 4, hipMemcpyDeviceToHost, h->stream);
  if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  if (flag) fmx_dev_free(flag);
  if (er != hipSuccess || not_one) {
    if (s.ids) fmx_dev_free(s.ids);
    s.ids = nullptr;
    if (er != hipSuccess) return fail(h, FMX_E_HIP, "id-only stream of the slot: %s", hipGetErrorString(er));
  }
  if (getenv("FMX_TRACE_SETUP")) fprintf(stderr, "[fmx setup] id-only stream %s %8.3f ms\n", s.ids ? "built" : "not unit-valued",
                                         1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - acc_.t0).count());
  return FMX_OK;
}

// the slot's training-side weight stream (WTrain, fmx_kernels.h): the entries whose feature occurs ONCE in the slot ("singles") get a packed
// copy of their linear weight that k_fused<FUSED_EXACT> reads instead of gathering w[j].  Built once, by the first one-pass epoch after an
// upload: one count per feature (at most 2^27 buckets, temporary), one mask per row, the exclusive sum of the rows' counts.  Kept only where
// the singles are at least 1/16 of the entries (field data with skewed ids has next to none: 12 bytes per row would buy nothing); resident
// then: 12 bytes per row + 4 per single.  Whatever goes wrong here -- an allocation above all -- leaves the slot gathering as before.
int ensure_wtrain(fmx_handle h, Slot& s, uint32_t row_cap) {
  if (s.wtrain_asked) return FMX_OK;
  s.wtrain_asked = true;
  if (!h->wtrain || s.nnz == 0 || s.nnz >= (1ull << 32) - 1 || s.n_rows >= 0x7FFFFFFEu) return FMX_OK;   // (soff counts in 32 bits)
  struct Acc { fmx_handle h; std::chrono::steady_clock::time_point t0;
               ~Acc() { h->setup_acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } } acc_{h, std::chrono::steady_clock::now()};
  const uint32_t M = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(h->n_local, 1), 1ull << 27);
  const size_t n1 = (size_t)s.n_rows + 1;
  uint32_t* cnt = nullptr; uint32_t* scount = nullptr; void* tmp = nullptr;
  size_t tmp_bytes = 0;
  uint32_t total = 0;
  hipError_t er = hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)n1, h->stream);
  if (er == hipSuccess) er = fmx_dev_alloc(&cnt, (size_t)M * 4);
  if (er == hipSuccess) er = fmx_dev_alloc(&scount, n1 * 4);
  if (er == hipSuccess) er = fmx_dev_alloc(&tmp, std::max<size_t>(tmp_bytes, 256));
  if (er == hipSuccess) er = fmx_dev_alloc(&s.smask, (size_t)s.n_rows * 8);
  if (er == hipSuccess) er = fmx_dev_alloc(&s.soff, n1 * 4);
  if (er == hipSuccess) er = hipMemsetAsync(cnt, 0, (size_t)M * 4, h->stream);
  if (er == hipSuccess) er = hipMemsetAsync(scount + s.n_rows, 0, 4, h->stream);
  if (er == hipSuccess) {
    hipLaunchKernelGGL(k_wtrain_count, dim3((unsigned)std::min<uint64_t>((s.nnz + 255) / 256, 8192)), dim3(256), 0, h->stream, s.ent, s.nnz, M, cnt);
    hipLaunchKernelGGL(k_wtrain_mask, dim3((unsigned)std::min<uint32_t>((s.n_rows + 3) / 4, 16384)), dim3(256), 0, h->stream, s.ent, s.row_ptr, s.n_rows, M,
                       (const uint32_t*)cnt, row_cap, s.smask, scount);
    er = hipGetLastError();
  }
  if (er == hipSuccess) er = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, scount, s.soff, (int)n1, h->stream);
  if (er == hipSuccess) er = hipMemcpyAsync(&total, s.soff + s.n_rows, 4, hipMemcpyDeviceToHost, h->stream);
  if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  if (cnt) fmx_dev_free(cnt);
  if (scount) fmx_dev_free(scount);
  if (tmp) fmx_dev_free(tmp);
  if (er == hipSuccess) s.wtrain_n = total;
  const bool keep = er == hipSuccess && total != 0 && (uint64_t)total * 16u >= s.nnz;
  if (keep) er = fmx_dev_alloc(&s.wtrain, (size_t)total * 4);
  if (!keep || er != hipSuccess) {
    if (er != hipSuccess) (void)hipGetLastError();               // (the stream is an extra: the epoch runs without it)
    if (s.smask) fmx_dev_free(s.smask);
    if (s.soff) fmx_dev_free(s.soff);
    s.smask = nullptr; s.soff = nullptr; s.wtrain = nullptr;
  }
  s.wtrain_version = 0;                                          // nothing is in the stream yet: the first epoch gathers and fills it
  if (getenv("FMX_TRACE_SETUP")) fprintf(stderr, "[fmx setup] training weight stream %s (%llu singles of %llu entries) %8.3f ms\n", s.wtrain ? "built" : "not kept",
                                         (unsigned long long)s.wtrain_n, (unsigned long long)s.nnz,
                                         1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - acc_.t0).count());
  return FMX_OK;
}

// rest[e] (= y-hat - w0) for rows [row0,row0+n) of a slot, single device
int launch_rest(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n, float* rest, hipStream_t st, const CompactState* snap) {
  if (!s.blocks.empty()) {                                     // (never with a snapshot: its entry points refuse such slots)
    // kept `-relation` blocks: the partial sums of the main rows, plus -- through the mappings -- those of the block rows
    // (every block row is evaluated once, however many main rows use it), then rest = c + 0.5 * sum_f S_f^2
    if (row0 != 0 || n != s.n_rows) return fail(h, FMX_E_ARG, "rows with kept blocks are predicted as a whole");
    int rc = ensure_scratch(h, n, 0);
    if (rc) return rc;
    float* S = h->partial;
    float* c = S + (size_t)n * h->KP;
    KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, true, false>), n, st, s.ent, s.row_ptr, (uint64_t)0, n, RowsF32{h->tb}, h->cfg.k1, S, c));
    for (BlockRows* br : s.blocks) {
      const uint32_t B = br->rows.n_rows;
      if (!B) continue;
      Tab tb = h->tb;                                        // the block's attribute 0 is global attribute attr_offset
      tb.V += (size_t)br->attr_offset * tb.rs; tb.w += (size_t)br->attr_offset * tb.ws;
      float* Sb = br->pbuf;
      KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, true, false>), B, st, br->rows.ent, br->rows.row_ptr, (uint64_t)0, B, RowsF32{tb}, h->cfg.k1,
                                         Sb, Sb + (size_t)B * h->KP));
      KP_SWITCH(h->KP, hipLaunchKernelGGL((k_rel_add_partial<KP>), dim3(std::min<uint32_t>((uint32_t)(((uint64_t)n * (h->KP + 1) + 255) / 256), 4096)),
                                            dim3(256), 0, st, br->map, (uint64_t)0, n, B, (const float*)Sb, S));
    }
    KP_SWITCH(h->KP, hipLaunchKernelGGL((k_rest_from_partial<KP>), dim3(wave_grid((n + Map<KP>::EPI - 1) / Map<KP>::EPI)), dim3(256), 0, st,
                                          (const float*)S, (const float*)c, n, rest));
    HIPCHK(h, hipGetLastError());
    return FMX_OK;
  }
  // the linear weights come out of the slot's side stream where it is current (it is after a one-pass epoch on THIS slot that kept it,
  // and until anything else touches w): 4 coalesced bytes per entry instead of a 64-byte fabric request
  const float* ws = (s.wside && s.wside_version == h->w_version && h->cfg.shard_world == 1) ? s.wside : nullptr;
  if (snap && snap->dir && snap->format == FMX_COMPACT_INT8) { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, false, true, RowsI8P>), n, st,
                                                 s.ent, s.row_ptr, row0, n, compact_rows8_p(*snap), h->cfg.k1, (float*)nullptr, rest)); }
  else if (snap && snap->dir) { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, false, true, RowsBf16P>), n, st,
                                                 s.ent, s.row_ptr, row0, n, compact_rows_p(h, *snap), h->cfg.k1, (float*)nullptr, rest)); }
  else if (snap && snap->format == FMX_COMPACT_INT8) { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, false, true, RowsI8>), n, st,
                                                 s.ent, s.row_ptr, row0, n, compact_rows8(*snap), h->cfg.k1, (float*)nullptr, rest)); }
  else if (snap) { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, false, true, RowsBf16>), n, st,
                                                 s.ent, s.row_ptr, row0, n, compact_rows(h, *snap), h->cfg.k1, (float*)nullptr, rest)); }
  else { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_rowsums<KP, false, true>), n, st,
                                            s.ent, s.row_ptr, row0, n, RowsF32{h->tb, ws}, h->cfg.k1, (float*)nullptr, rest)); }
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

int slot_scores(fmx_handle h, const Slot& s, const CompactState* snap, bool want_yhat, const float** score) {
  int rc = ensure_scratch(h, 0, (size_t)s.n_rows * 2); if (rc) return rc;
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  rc = launch_rest(h, s, 0, s.n_rows, h->rest, h->stream, snap); if (rc) return rc;
  *score = h->rest;
  if (!want_yhat) return FMX_OK;
  float* yhat = h->rest + s.n_rows;
  const int k0 = (h->cfg.shard_world > 1 && h->cfg.shard_rank != 0) ? 0 : h->cfg.k0;
  hipLaunchKernelGGL(k_yhat, dim3(std::min<uint32_t>((s.n_rows + 255) / 256, 2048)), dim3(256), 0, h->stream,
                     h->rest, s.n_rows, k0, snap ? snap->w0 : h->w0, yhat);
  HIPCHK(h, hipGetLastError());
  *score = yhat;
  return FMX_OK;
}

int predict_out(fmx_handle h, const Slot& s, const CompactState* snap, double* out) {
  if (s.n_rows == 0) return FMX_OK;
  const float* yhat;
  const int rc = slot_scores(h, s, snap, true, &yhat); if (rc) return rc;
  std::vector<float> tmp(s.n_rows);
  HIPCHK(h, hipMemcpyAsync(tmp.data(), yhat, (size_t)s.n_rows * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (uint32_t r = 0; r < s.n_rows; r++) out[r] = (double)tmp[r];
  return FMX_OK;
}

int evaluate_out(fmx_handle h, const Slot& s, const CompactState* snap, fmx_eval* out) {
  const float* rest;
  const int rc = slot_scores(h, s, snap, false, &rest); if (rc) return rc;
  HIPCHK(h, hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));
  hipLaunchKernelGGL(k_eval, dim3(std::min<uint32_t>((s.n_rows + 255) / 256, 2048)), dim3(256), 0, h->stream,
                     rest, s.target, s.n_rows, make_hyper(h->cfg), snap ? snap->w0 : h->w0, h->acc);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  double acc[4];
  HIPCHK(h, hipMemcpyAsync(acc, h->acc, sizeof(acc), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  out->device_seconds = ms * 1e-3;
  out->rmse = std::sqrt(acc[0] / s.n_rows);          // fm_learn.h:152
  out->mae = acc[1] / s.n_rows;                      // fm_learn.h:148
  out->accuracy = acc[2] / s.n_rows;                 // fm_learn.h:129
  return FMX_OK;
}

// collision mass of a slot's rows (cached in the slot): one histogram pass over the entries + one reduction.  On a feature
// shard this is the shard's share (its features only); the shares add up to the rows' C (fmx_comm.hip sums them).
int ensure_coll_mass(fmx_handle h, Slot& s) {
  if (s.coll_mass >= 0.0) return FMX_OK;
  if (s.nnz == 0 || s.n_rows == 0) { s.coll_mass = 0.0; return FMX_OK; }
  struct Acc { fmx_handle h; std::chrono::steady_clock::time_point t0;
               ~Acc() { h->setup_acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } } acc_{h, std::chrono::steady_clock::now()};
  HIPCHK(h, hipSetDevice(h->device));
  const uint32_t M = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(h->n_local, 1), 1ull << 27);
  double* hist = nullptr;
  HIPCHK(h, fmx_dev_alloc(&hist, (size_t)M * sizeof(double)));
  hipError_t er = hipMemsetAsync(hist, 0, (size_t)M * sizeof(double), h->stream);
  if (er == hipSuccess) er = hipMemsetAsync(h->acc, 0, 2 * sizeof(double), h->stream);
  if (er == hipSuccess) {
    hipLaunchKernelGGL(k_coll_hist, dim3((unsigned)std::min<uint64_t>((s.nnz + 255) / 256, 8192)), dim3(256), 0, h->stream, s.ent, s.nnz, M, hist, h->acc + 1);
    hipLaunchKernelGGL(k_coll_sumsq, dim3((unsigned)std::min<uint64_t>(((uint64_t)M + 255) / 256, 4096)), dim3(256), 0, h->stream,
                       (const double*)hist, M, h->acc);
    er = hipGetLastError();
  }
  double c[2] = {0.0, 0.0};
  if (er == hipSuccess) er = hipMemcpyAsync(c, h->acc, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  fmx_dev_free(hist);
  if (er != hipSuccess) return fail(h, FMX_E_HIP, "collision mass of the rows: %s", hipGetErrorString(er));
  // pairs of DIFFERENT rows: what a row shares with itself (sum of x^2 over its entries) is taken out.  On a feature shard this is
  // the shard's share of the numerator over the same N (N - 1): the shares add up.
  const double N = (double)s.n_rows;
  s.coll_mass = (s.n_rows > 1) ? std::max(0.0, c[0] - c[1]) / (N * (N - 1.0)) : 0.0;
  if (getenv("FMX_TRACE_SETUP")) fprintf(stderr, "[fmx setup] collision mass     %8.3f ms\n", 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - acc_.t0).count());
  return FMX_OK;
}

// the batch an epoch runs with (fmx_sgd_opts::batch): explicit, or the default cut to learn_rate * curvature * batch * C <= 1
void resolve_batch(const fmx_config& cfg, double coll_mass, uint32_t requested, uint32_t dflt, double curv_scale, fmx_batch_info* out) {
  const double curv = ((cfg.task == FMX_TASK_REGRESSION) ? 1.0 : 0.25) * curv_scale;
  const double per_row = cfg.learn_rate * curv * coll_mass;         // gain of one row of batch
  uint32_t B = requested ? requested : dflt;
  uint32_t status = 0;
  if (!requested && per_row > 0.0 && (double)B * per_row > 1.0) {
    uint32_t cut = 1;
    while ((double)(cut * 2) * per_row <= 1.0 && cut * 2 <= dflt) cut *= 2;
    B = std::max(cut, 32u);                                      // (rows that dense -- C in the hundreds -- are SEQUENTIAL's case: the gain says so)
    status |= FMX_STAT_BATCH_CUT;
  }
  out->collision_mass = coll_mass;
  out->batch = B;
  out->batch_gain = (double)B * per_row;
  if (out->batch_gain > 2.0) status |= FMX_STAT_UNSTABLE;
  out->status = status;
}

extern "C" {

int fmx_abi_version(void) { return FMX_ABI_VERSION; }

int fmx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* fmx_last_error(fmx_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int fmx_create(const fmx_config* cfg, fmx_handle* out) { return create_handle(cfg, out, false); }

}  // extern "C"

int create_handle(const fmx_config* cfg, fmx_handle* out, bool serve_only) {
  if (!cfg || !out) return fail(nullptr, FMX_E_ARG, "fmx_create: null argument");
  *out = nullptr;
  if (cfg->num_attribute == 0) return fail(nullptr, FMX_E_ARG, "num_attribute must be > 0");
  if (cfg->num_attribute > 0xFFFFFFFFull) return fail(nullptr, FMX_E_ARG, "num_attribute must fit uint32 (fm_model.h:51)");
  if (cfg->num_factor < 0) return fail(nullptr, FMX_E_ARG, "num_factor must be >= 0");
  if (cfg->num_factor > 1024) return fail(nullptr, FMX_E_UNSUPPORTED, "num_factor > 1024 is not supported");
  if (cfg->task != FMX_TASK_REGRESSION && cfg->task != FMX_TASK_CLASSIFICATION)
    return fail(nullptr, FMX_E_ARG, "unknown task");                       // fm_learn.h:81 "unknown task"
  if (cfg->shard_world < 1 || cfg->shard_rank < 0 || cfg->shard_rank >= cfg->shard_world)
    return fail(nullptr, FMX_E_ARG, "bad shard_rank/shard_world");
  if (cfg->shard_hash != 0 && cfg->shard_hash != 1) return fail(nullptr, FMX_E_ARG, "shard_hash must be 0 or 1");
  if (cfg->place_candidates < 0 || cfg->place_candidates > 6) return fail(nullptr, FMX_E_ARG, "place_candidates must be 0 (default) .. 6");
  if (cfg->exchange_algo != FMX_EXCHANGE_ALLREDUCE && cfg->exchange_algo != FMX_EXCHANGE_RS_AG)
    return fail(nullptr, FMX_E_ARG, "exchange_algo %u: FMX_EXCHANGE_ALLREDUCE (0) or FMX_EXCHANGE_RS_AG (1)", cfg->exchange_algo);
  if ((uint64_t)cfg->shard_world > cfg->num_attribute) return fail(nullptr, FMX_E_ARG, "more feature shards than features");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(nullptr, FMX_E_HIP, "no HIP device available (%s); libfmx has no CPU fallback",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  int dev = cfg->device;
  if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
  if (dev >= ndev) return fail(nullptr, FMX_E_ARG, "device %d out of range (%d devices)", dev, ndev);

  fmx_handle h = new fmx_context_s();
  h->cfg = *cfg;
  h->device = dev;
  h->KP = next_pow2(std::max(cfg->num_factor, 1));
  const uint64_t n = cfg->num_attribute, W = (uint64_t)cfg->shard_world, R = (uint64_t)cfg->shard_rank;
  h->n_local = (n > R) ? (n - R + W - 1) / W : 0;
  if (h->n_local == 0) h->n_local = 1;
#define CREATE_CHK(expr)                                                                     \
  do { hipError_t _e = (expr); if (_e != hipSuccess) {                                       \
      fail(nullptr, FMX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));               \
      fmx_destroy(h); return FMX_E_HIP; } } while (0)
  CREATE_CHK(hipSetDevice(dev));
  mark_device_used(dev);
  CREATE_CHK(hipGetDeviceProperties(&h->prop, dev));
  CREATE_CHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  CREATE_CHK(hipEventCreate(&h->ev0));
  CREATE_CHK(hipEventCreate(&h->ev1));
  {
    // row layout: V rows of KP floats, the linear weights in an array of their own (co-locating w_j behind its row was measured
    // in rounds 1 and 2: HBM fetches 64-byte sectors, a 4-byte w costs one wherever it lives, and unaligned rows cost more)
    // ... rows of num_factor floats rounded up to 16 (one 64-byte sector), not to the power of two KP of the lane mapping: k = 100 keeps rows of
    // 112 floats (448 B) where the padded 128 moved 512 (round-5 verdict item 9; fmx_kernels.h row_ld).  FMX_ROW_STRIDE_KP=1: the padded rows.
    h->tb.rs = (uint32_t)h->KP;
    { const char* rk = getenv("FMX_ROW_STRIDE_KP");
      if (h->KP >= 32 && !(rk && rk[0] == '1')) h->tb.rs = std::min<uint32_t>((uint32_t)h->KP, ((uint32_t)cfg->num_factor + 15u) / 16u * 16u); }
    // a serve-only handle (fmx_serve_open) gets everything below but no parameter tables: tb.V, tb.w and w_sep stay null
    h->serve_only = serve_only;
    if (!serve_only && place_tables(h) != FMX_OK) { fmx_destroy(h); return FMX_E_HIP; }      // fmx_mem.hip: the arena, or the best of place_candidates allocations
    h->tb.w = h->w_sep; h->tb.ws = 1;
  }
  CREATE_CHK(fmx_dev_alloc(&h->w0, sizeof(double)));
  CREATE_CHK(fmx_dev_alloc(&h->w0_pp, 8 * sizeof(double)));
  {  // device-side hand-off of the bias (fmx_sgd.hip: sgd_epoch_fused): a counter + an error word, both start at 0
    CREATE_CHK(fmx_dev_alloc(&h->handoff_ctr, 2 * sizeof(unsigned long long)));
    h->handoff_err = reinterpret_cast<uint32_t*>(h->handoff_ctr + 1);
    CREATE_CHK(hipMemsetAsync(h->handoff_ctr, 0, 2 * sizeof(unsigned long long), h->stream));
    const char* e = getenv("FMX_HANDOFF");
    h->handoff = !(e && e[0] == '0');
    CREATE_CHK(fmx_dev_alloc(&h->pit_ctr, (PIT_MAX_IT + 1) * sizeof(unsigned long long)));
    CREATE_CHK(fmx_dev_alloc(&h->pit_slots, (size_t)2 * PIT_MAX_WG * 4 * sizeof(double)));
    CREATE_CHK(hipMemsetAsync(h->pit_slots, 0, (size_t)2 * PIT_MAX_WG * 4 * sizeof(double), h->stream));
    const char* sc = getenv("FMX_SCAN");
    h->scan_pit = !(sc && strcmp(sc, "serial") == 0);
    const char* so = getenv("FMX_SMALL_ONE");
    h->small_one = !(so && so[0] == '0');                       // small batches as one launch per batch (fmx_small_kernels.h); FMX_SMALL_ONE=0: two
    const char* si = getenv("FMX_IDS");
    h->ids = !(si && si[0] == '0');                             // id-only entry stream of unit-valued fixed-length slots (ensure_ids); FMX_IDS=0: entries
    const char* sw = getenv("FMX_WTRAIN");
    h->wtrain = !(sw && sw[0] == '0');                          // packed stream of the singles' linear weights (ensure_wtrain); FMX_WTRAIN=0: every w_j is gathered
    auto env_on = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };
    h->seq_rows = env_on("FMX_SEQ_ROWS");                       // FMX_SGD_SEQUENTIAL (fmx_sgd.hip fmx_sgd_epoch, seq_runs_epoch): =0 turns a form off
    h->seq_wg = env_on("FMX_SEQ_WG");
    h->seq_runs_fused = env_on("FMX_SEQ_RUNS_FUSED");
    h->seq_runs_one = env_on("FMX_SEQ_RUNS_ONE");
    const char* ts = getenv("FMX_TOPK_SPLITS");                 // fmx_topk (fmx_topk.hip): force the candidate splits, 1 .. 1024
    if (ts) h->topk_splits = (uint32_t)std::min<unsigned long>(strtoul(ts, nullptr, 10), 1024ul);
    const char* sp = getenv("FMX_DEBUG_PIT_SPINS");
    h->pit_spins = sp ? (uint32_t)strtoul(sp, nullptr, 10) : HANDOFF_SPINS;
  }
  {  // the side stream runs the one-workgroup bias recurrence next to chip-filling gathers: give it priority so
     // that its workgroup is placed as soon as any CU has room
    int lo = 0, hi = 0;
    CREATE_CHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    CREATE_CHK(hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, hi));
  }
  h->num_cu = h->prop.multiProcessorCount > 0 ? h->prop.multiProcessorCount : 256;
  CREATE_CHK(fmx_dev_alloc(&h->acc, 4 * sizeof(double)));
  CREATE_CHK(hipMemsetAsync(h->w0, 0, sizeof(double), h->stream));
  CREATE_CHK(hipStreamSynchronize(h->stream));
#undef CREATE_CHK
  *out = h;
  return FMX_OK;
}

extern "C" {

int fmx_batch_rule(int32_t task, double learn_rate, double collision_mass, uint32_t requested, fmx_batch_info* out) {
  if (!out || (task != FMX_TASK_REGRESSION && task != FMX_TASK_CLASSIFICATION) || !(learn_rate >= 0.0) || !(collision_mass >= 0.0)) return FMX_E_ARG;
  fmx_config c = {};
  c.task = task; c.learn_rate = learn_rate;
  resolve_batch(c, collision_mass, requested, FMX_DEFAULT_BATCH, 1.0, out);
  return FMX_OK;
}

int fmx_destroy(fmx_handle h) {
  if (!h) return FMX_OK;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  comm_free(h);
  als_free(h);
  sgda_free(h);
  adapt_free(h);
  ftrl_free(h);
  compact_free(h);
  for (auto& s : h->slots) free_slot(s);
  if (h->grp) fmx_dev_free(h->grp);
  free_tables(h);
  if (h->w0) fmx_dev_free(h->w0);
  if (h->w0_pp) fmx_dev_free(h->w0_pp);
  if (h->handoff_ctr) fmx_dev_free(h->handoff_ctr);
  if (h->pit_ctr) fmx_dev_free(h->pit_ctr);
  if (h->probe_flags) fmx_dev_free(h->probe_flags);
  if (h->pit_tmp) fmx_dev_free(h->pit_tmp);
  if (h->run_slots) fmx_dev_free(h->run_slots);
  if (h->small_slots) fmx_dev_free(h->small_slots);
  if (h->pit_slots) fmx_dev_free(h->pit_slots);
  if (h->w0_slots) fmx_dev_free(h->w0_slots);
  if (h->stream2) hipStreamDestroy(h->stream2);
  if (h->acc) fmx_dev_free(h->acc);
  if (h->partial) fmx_dev_free(h->partial);
  if (h->mult) fmx_dev_free(h->mult);
  if (h->rest) fmx_dev_free(h->rest);
  for (auto ev : h->ev_pool) hipEventDestroy(ev);
  for (auto ev : h->ev_sync) hipEventDestroy(ev);
  if (h->lag.ev_rest) hipEventDestroy(h->lag.ev_rest);
  for (auto e : h->lag.ev_scan) if (e) hipEventDestroy(e);
  if (h->ev0) hipEventDestroy(h->ev0);
  if (h->ev1) hipEventDestroy(h->ev1);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return FMX_OK;
}

int fmx_get_info(fmx_handle h, fmx_info* out) {
  if (!h || !out) return FMX_E_ARG;
  memset(out, 0, sizeof(*out));
  out->n_local = h->n_local;
  out->k_padded = h->KP;
  out->device = h->device;
  out->bytes_params = h->serve_only ? 0 : h->n_local * (size_t)(h->tb.rs + (h->w_sep ? 1 : 0)) * sizeof(float);
  snprintf(out->device_name, sizeof(out->device_name), "%s", h->prop.name);
  snprintf(out->arch, sizeof(out->arch), "%s", h->prop.gcnArchName);
  return FMX_OK;
}

int fmx_synchronize(fmx_handle h) {
  if (!h) return FMX_E_ARG;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return scan_error_check(h);
}

// ---------------------------------------------------------------------------------------------
// parameters
// ---------------------------------------------------------------------------------------------
static int stage_params(fmx_handle h, bool to_device, double* w0, double* w, double* v) {
  if (to_device) touch_w(h);
  HIPCHK(h, hipSetDevice(h->device));
  const uint64_t n = h->cfg.num_attribute;
  const int k = h->cfg.num_factor, KP = h->KP;
  const int W = h->cfg.shard_world;
  const Shard sh = make_shard(h->cfg);
  if (to_device) {
    HIPCHK(h, hipMemcpyAsync(h->w0, w0, sizeof(double), hipMemcpyHostToDevice, h->stream));
  } else {
    HIPCHK(h, hipMemcpyAsync(w0, h->w0, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  const uint32_t chunk = (uint32_t)std::min<uint64_t>(n, 1u << 18);
  double* stage = nullptr;
  HIPCHK(h, fmx_dev_alloc(&stage, (size_t)chunk * (size_t)std::max(k, 1) * sizeof(double)));
  int rc = FMX_OK;
#define STAGE_CHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
    rc = fail(h, FMX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); goto done; } } while (0)
  for (uint64_t j0 = 0; j0 < n; j0 += chunk) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(chunk, n - j0);
    if (w) {
      if (to_device) {
        STAGE_CHK(hipMemcpyAsync(stage, w + j0, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_w_in, dim3((cnt + 255) / 256), dim3(256), 0, h->stream, stage, j0, cnt, sh, h->tb);
      } else {
        if (W > 1) STAGE_CHK(hipMemcpyAsync(stage, w + j0, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_w_out, dim3((cnt + 255) / 256), dim3(256), 0, h->stream, stage, j0, cnt, sh, h->tb);
        STAGE_CHK(hipMemcpyAsync(w + j0, stage, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      }
      STAGE_CHK(hipStreamSynchronize(h->stream));
    }
    if (v && k > 0) {
      if (to_device) {
        for (int f = 0; f < k; f++)
          STAGE_CHK(hipMemcpyAsync(stage + (size_t)f * cnt, v + (size_t)f * n + j0, cnt * sizeof(double),
                                   hipMemcpyHostToDevice, h->stream));
        const uint64_t total = (uint64_t)cnt * KP;
        hipLaunchKernelGGL(k_stage_in, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, h->stream,
                           stage, j0, cnt, k, KP, sh, h->tb);
      } else {
        if (W > 1)
          for (int f = 0; f < k; f++)
            STAGE_CHK(hipMemcpyAsync(stage + (size_t)f * cnt, v + (size_t)f * n + j0, cnt * sizeof(double),
                                     hipMemcpyHostToDevice, h->stream));
        const uint64_t total = (uint64_t)cnt * k;
        hipLaunchKernelGGL(k_stage_out, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, h->stream,
                           stage, j0, cnt, k, KP, sh, h->tb);
        for (int f = 0; f < k; f++)
          STAGE_CHK(hipMemcpyAsync(v + (size_t)f * n + j0, stage + (size_t)f * cnt, cnt * sizeof(double),
                                   hipMemcpyDeviceToHost, h->stream));
      }
      STAGE_CHK(hipStreamSynchronize(h->stream));
    }
  }
  STAGE_CHK(hipGetLastError());
  STAGE_CHK(hipStreamSynchronize(h->stream));
done:
#undef STAGE_CHK
  fmx_dev_free(stage);
  return rc;
}

int fmx_set_params(fmx_handle h, double w0, const double* w, const double* v) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_set_params"); if (_sr) return _sr; }
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  if (h->cfg.num_factor > 0 && !v) return fail(h, FMX_E_ARG, "fmx_set_params: v is NULL but num_factor > 0");
  double w0c = w0;
  return stage_params(h, true, &w0c, const_cast<double*>(w), const_cast<double*>(v));
}

int fmx_get_params(fmx_handle h, double* w0, double* w, double* v) {
  if (!h || !w0) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_get_params"); if (_sr) return _sr; }
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  return stage_params(h, false, w0, w, v);
}

int fmx_get_param_rows(fmx_handle h, const uint32_t* ids, uint32_t count, double* w_out, double* v_out) {
  if (!h || !ids || !w_out) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_get_param_rows"); if (_sr) return _sr; }
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  const int k = h->cfg.num_factor;
  const Shard sh = make_shard(h->cfg);
  if (k > 0 && !v_out) return fail(h, FMX_E_ARG, "fmx_get_param_rows: v_out is NULL");
  if (count == 0) return FMX_OK;
  for (uint32_t i = 0; i < count; i++) {
    if (ids[i] >= h->cfg.num_attribute) return fail(h, FMX_E_ARG, "feature id %u >= num_attribute", ids[i]);
    if (!sh.owns(ids[i])) return fail(h, FMX_E_ARG, "feature id %u is not on this shard", ids[i]);
  }
  double* const outs[1][2] = {{w_out, v_out}};
  return gather_rows(h, "fmx_get_param_rows", ids, count, 1, outs, [&](int, dim3 grid, const uint32_t* d_ids, double* d_w, double* d_v) {
    hipLaunchKernelGGL(k_fetch_rows<RowsF32>, grid, dim3(256), 0, h->stream, d_ids, count, k, sh, RowsF32{h->tb}, d_w, d_v);
  });
}

// ---- fm_model::saveModel / loadModel (fm_model.h:132-190) straight from / into the device table ----------------------
// The device keeps the factors FEATURE-major, which is the order of the file's "#pairwise interactions Vj,f" section (one
// line per feature, its k factors in order): the table is streamed in chunks of rows, never converted to the reference's
// fp64 factor-major block (51 GB at the north-star size).  Numbers are written as the reference's ostream writes doubles
// (6 significant digits, printf "%g").
int fmx_save_model(fmx_handle h, const char* path) {
  if (!h || !path) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_save_model"); if (_sr) return _sr; }
  if (h->cfg.shard_world > 1) return fail(h, FMX_E_UNSUPPORTED, "fmx_save_model on a feature shard: collect the parameters with fmx_get_params");
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  FILE* f = fopen(path, "w");
  if (!f) return fail(h, FMX_E_ARG, "fmx_save_model: cannot open %s", path);
  const uint64_t n = h->cfg.num_attribute;
  const int k = h->cfg.num_factor;
  const size_t chunk = 1u << 16;
  std::vector<float> buf(chunk * (size_t)std::max<uint32_t>(h->tb.rs, 1));
  int rc = FMX_OK;
  if (h->cfg.k0) {
    double w0 = 0;
    if (hipMemcpy(&w0, h->w0, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = FMX_E_HIP;
    fprintf(f, "#global bias W0\n%g\n", w0);
  }
  if (rc == FMX_OK && h->cfg.k1) {
    fprintf(f, "#unary interactions Wj\n");
    for (uint64_t j0 = 0; j0 < n && rc == FMX_OK; j0 += chunk) {
      const size_t cnt = (size_t)std::min<uint64_t>(chunk, n - j0);
      if (h->tb.ws == 1) { if (hipMemcpy(buf.data(), h->tb.w + j0, cnt * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = FMX_E_HIP; }
      else if (hipMemcpy2D(buf.data(), sizeof(float), h->tb.w + j0 * h->tb.ws, (size_t)h->tb.ws * sizeof(float), sizeof(float), cnt, hipMemcpyDeviceToHost) != hipSuccess) rc = FMX_E_HIP;
      for (size_t i = 0; i < cnt && rc == FMX_OK; i++) fprintf(f, "%g\n", (double)buf[i]);
    }
  }
  if (rc == FMX_OK) {
    fprintf(f, "#pairwise interactions Vj,f\n");
    for (uint64_t j0 = 0; j0 < n && rc == FMX_OK; j0 += chunk) {
      const size_t cnt = (size_t)std::min<uint64_t>(chunk, n - j0);
      if (k > 0 && hipMemcpy(buf.data(), h->tb.V + j0 * h->tb.rs, cnt * (size_t)h->tb.rs * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = FMX_E_HIP;
      for (size_t i = 0; i < cnt && rc == FMX_OK; i++) {
        const float* row = buf.data() + i * h->tb.rs;
        for (int ff = 0; ff < k; ff++) { fprintf(f, "%g", (double)row[ff]); if (ff != k - 1) fputc(' ', f); }
        fputc('\n', f);
      }
    }
  }
  const bool werr = ferror(f) != 0;
  if (fclose(f) != 0 || werr) return fail(h, FMX_E_ARG, "fmx_save_model: write error on %s", path);
  if (rc != FMX_OK) return fail(h, rc, "fmx_save_model: device copy failed");
  return FMX_OK;
}

// returns FMX_E_ARG ("malformed model file") where fm_model::loadModel returns 0 (libfm.cpp:264-267).  Every shard of a
// sharded model may load the same file: it keeps its own features.
int fmx_load_model(fmx_handle h, const char* path) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_load_model"); if (_sr) return _sr; }
  touch_w(h);
  if (!h || !path) return FMX_E_ARG;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  FILE* f = fopen(path, "r");
  if (!f) return fail(h, FMX_E_ARG, "malformed model file (cannot open %s)", path);
  const uint64_t n = h->cfg.num_attribute;
  const int k = h->cfg.num_factor;
  const Shard sh = make_shard(h->cfg);
  char* line = nullptr; size_t cap = 0;
  auto next = [&]() -> bool { return getline(&line, &cap, f) >= 0; };
  int rc = FMX_OK;
  const char* what = "";
  std::vector<float> stage;
  std::vector<uint32_t> rows;
  auto flush_w = [&]() {                                    // scatter the staged linear weights to their local rows
    for (size_t i = 0; i < rows.size() && rc == FMX_OK; i++)
      if (hipMemcpyAsync(h->tb.w + (size_t)rows[i] * h->tb.ws, &stage[i], sizeof(float), hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = FMX_E_HIP;
    if (hipStreamSynchronize(h->stream) != hipSuccess) rc = FMX_E_HIP;
    rows.clear(); stage.clear();
  };
  if (h->cfg.k0) {
    double w0 = 0;
    if (!next() || !next()) { rc = FMX_E_ARG; what = "bias section"; }
    else { w0 = atof(line); if (hipMemcpy(h->w0, &w0, sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = FMX_E_HIP; }
  }
  if (rc == FMX_OK && h->cfg.k1) {
    if (!next()) { rc = FMX_E_ARG; what = "linear section"; }
    const size_t chunk = 1u << 16;
    std::vector<float> wbuf;
    uint64_t j0 = 0;
    for (uint64_t j = 0; j < n && rc == FMX_OK; j++) {
      if (!next()) { rc = FMX_E_ARG; what = "linear weights"; break; }
      const float val = (float)atof(line);
      if (sh.world == 1) {
        wbuf.push_back(val);
        if (wbuf.size() == chunk || j + 1 == n) {
          if (h->tb.ws == 1) { if (hipMemcpy(h->tb.w + j0, wbuf.data(), wbuf.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = FMX_E_HIP; }
          else if (hipMemcpy2D(h->tb.w + j0 * h->tb.ws, (size_t)h->tb.ws * sizeof(float), wbuf.data(), sizeof(float), sizeof(float), wbuf.size(), hipMemcpyHostToDevice) != hipSuccess) rc = FMX_E_HIP;
          j0 = j + 1; wbuf.clear();
        }
      } else {
        uint32_t jl;
        if (sh.place((uint32_t)j, &jl)) { rows.push_back(jl); stage.push_back(val); if (rows.size() == chunk) flush_w(); }
      }
    }
    if (rc == FMX_OK && !rows.empty()) flush_w();
  }
  if (rc == FMX_OK && !next()) { rc = FMX_E_ARG; what = "factor section"; }
  if (rc == FMX_OK) {
    const size_t chunk = 1u << 14;
    std::vector<float> vbuf(chunk * (size_t)h->tb.rs, 0.f);
    size_t filled = 0; uint64_t j0 = 0;
    for (uint64_t j = 0; j < n && rc == FMX_OK; j++) {
      if (!next()) { rc = FMX_E_ARG; what = "factor rows"; break; }
      uint32_t jl = (uint32_t)j;
      const bool mine = sh.place((uint32_t)j, &jl);
      float* row = vbuf.data() + filled * h->tb.rs;
      // the reference splits at single blanks and wants exactly num_factor tokens (fm_model.h:176-179)
      int cnt = 0;
      char* p = line;
      size_t len = strlen(p);
      while (len && (p[len - 1] == '\n' || p[len - 1] == '\r')) p[--len] = 0;
      if (k > 0) {
        for (char* tok = p;; ) {
          char* sp = strchr(tok, ' ');
          if (sp) *sp = 0;
          if (cnt < k) row[cnt] = (float)atof(tok);
          cnt++;
          if (!sp) break;
          tok = sp + 1;
        }
        if (cnt != k) { rc = FMX_E_ARG; what = "factor count of a row"; break; }
      }
      if (sh.world == 1) {
        filled++;
        if (filled == chunk || j + 1 == n) {
          if (k > 0 && hipMemcpy(h->tb.V + j0 * h->tb.rs, vbuf.data(), filled * (size_t)h->tb.rs * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = FMX_E_HIP;
          j0 = j + 1; filled = 0;
        }
      } else if (mine && k > 0) {
        if (hipMemcpy(h->tb.V + (size_t)jl * h->tb.rs, row, (size_t)k * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = FMX_E_HIP;
      }
    }
  }
  free(line);
  fclose(f);
  if (rc == FMX_E_ARG) return fail(h, FMX_E_ARG, "malformed model file (%s)", what);
  if (rc != FMX_OK) return fail(h, rc, "fmx_load_model: device copy failed");
  return FMX_OK;
}

int fmx_get_w0(fmx_handle h, double* w0) {
  if (!h || !w0) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_get_w0"); if (_sr) return _sr; }
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(w0, h->w0, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return FMX_OK;
}

int fmx_set_groups(fmx_handle h, const uint32_t* group_of_feature, uint32_t num_groups) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_set_groups"); if (_sr) return _sr; }
  if (h->als.slot >= 0 || h->sgda.reg) return fail(h, FMX_E_STATE, "fmx_set_groups while an ALS / SGDA session is open");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->grp) { fmx_dev_free(h->grp); h->grp = nullptr; }
  h->num_groups = 1;
  if (!group_of_feature || num_groups <= 1) return FMX_OK;
  // the array is indexed by GLOBAL feature id ([num_attribute]); a shard keeps the entries of its own features
  const Shard sh = make_shard(h->cfg);
  std::vector<uint32_t> local(h->n_local);
  for (uint64_t jl = 0; jl < h->n_local; jl++) {
    const uint32_t j = sh.global(jl);
    local[jl] = ((uint64_t)j < h->cfg.num_attribute) ? group_of_feature[j] : 0u;
    if (local[jl] >= num_groups)
      return fail(h, FMX_E_ARG, "fmx_set_groups: feature %u has group %u >= num_groups %u", j, local[jl], num_groups);
  }
  HIPCHK(h, fmx_dev_alloc(&h->grp, h->n_local * sizeof(uint32_t)));
  HIPCHK(h, hipMemcpy(h->grp, local.data(), h->n_local * sizeof(uint32_t), hipMemcpyHostToDevice));
  h->num_groups = num_groups;
  return FMX_OK;
}

int fmx_init_params(fmx_handle h, double init_mean, double init_stdev, uint64_t seed) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_init_params"); if (_sr) return _sr; }
  touch_w(h);
  if (!h) return FMX_E_ARG;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(k_init_params, dim3(256 * 8), dim3(256), 0, h->stream, h->tb, h->n_local,
                     h->cfg.num_factor, h->KP, make_shard(h->cfg), (float)init_mean, init_stdev, seed);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemsetAsync(h->w0, 0, sizeof(double), h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return FMX_OK;
}

// ---------------------------------------------------------------------------------------------
// rows
// ---------------------------------------------------------------------------------------------
int fmx_free_rows(fmx_handle h, int slot) {
  if (!h || slot < 0 || slot >= FMX_MAX_SLOTS) return FMX_E_ARG;
  { int _rc = slot_in_session(h, slot, "fmx_free_rows"); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_interactions(h, slot);
  free_slot(h->slots[slot]);
  return FMX_OK;
}

int fmx_upload_rows(fmx_handle h, int slot, const void* entries, const uint64_t* row_ptr, const float* target,
                    uint32_t n_rows, uint64_t nnz) {
  if (!h) return FMX_E_ARG;
  if (slot < 0 || slot >= FMX_MAX_SLOTS) return fail(h, FMX_E_ARG, "slot %d out of range", slot);
  { int _rc = slot_in_session(h, slot, "fmx_upload_rows"); if (_rc) return _rc; }
  if (!row_ptr || (nnz > 0 && !entries)) return fail(h, FMX_E_ARG, "fmx_upload_rows: null entries/row_ptr");
  if (row_ptr[0] != 0 || row_ptr[n_rows] != nnz) return fail(h, FMX_E_ARG, "row_ptr[0] must be 0 and row_ptr[n_rows] == nnz");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_interactions(h, slot);
  free_slot(h->slots[slot]);
  const Entry* src = static_cast<const Entry*>(entries);
  const uint64_t n = h->cfg.num_attribute;
  const uint32_t W = (uint32_t)h->cfg.shard_world;
  const Shard sh = make_shard(h->cfg);
  std::vector<Entry> local_ent;
  std::vector<uint64_t> local_ptr;
  const Entry* up_ent = src;
  const uint64_t* up_ptr = row_ptr;
  uint64_t up_nnz = nnz;
  uint32_t max_row = 0;
  // unsharded: the entries go to the device as they are -- start the transfer now (DMA at PCIe speed when the buffer is
  // page-locked, e.g. from fmx_read_binary) and check the ids on the host while it runs
  Slot s;
  if (W == 1) {
    HIPCHK(h, fmx_dev_alloc(&s.ent, std::max<uint64_t>(nnz, 1) * sizeof(Entry)));
    if (nnz && hipMemcpyAsync(s.ent, src, nnz * sizeof(Entry), hipMemcpyHostToDevice, h->stream) != hipSuccess) {
      fmx_dev_free(s.ent); return fail(h, FMX_E_HIP, "fmx_upload_rows: copy of the entries failed");
    }
  }
  // bound check: the reference asserts id < num_attribute (fm_model.h:112)
  for (uint64_t i = 0; i < nnz; i++)
    if (src[i].id >= n) {
      if (s.ent) { hipStreamSynchronize(h->stream); fmx_dev_free(s.ent); }
      return fail(h, FMX_E_ARG, "feature id %u >= num_attribute %llu (row entry %llu)", src[i].id,
                  (unsigned long long)n, (unsigned long long)i);
    }
  if (W > 1) {   // keep this shard's features, ids become local rows (Shard::place)
    local_ptr.resize((size_t)n_rows + 1);
    local_ent.reserve((size_t)(nnz / W + n_rows));
    for (uint32_t r = 0; r < n_rows; r++) {
      local_ptr[r] = local_ent.size();
      for (uint64_t i = row_ptr[r]; i < row_ptr[r + 1]; i++)
        { Entry e; if (sh.place(src[i].id, &e.id)) { e.value = src[i].value; local_ent.push_back(e); } }
    }
    local_ptr[n_rows] = local_ent.size();
    up_ent = local_ent.data(); up_ptr = local_ptr.data(); up_nnz = local_ent.size();
  }
  uint32_t min_row = n_rows ? 0xFFFFFFFFu : 0u;
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint32_t sz = (uint32_t)(up_ptr[r + 1] - up_ptr[r]);
    max_row = std::max(max_row, sz); min_row = std::min(min_row, sz);
  }
  hipError_t er = hipSuccess;
  if (!s.ent) {
    er = fmx_dev_alloc(&s.ent, std::max<uint64_t>(up_nnz, 1) * sizeof(Entry));
    if (er == hipSuccess && up_nnz) er = hipMemcpyAsync(s.ent, up_ent, up_nnz * sizeof(Entry), hipMemcpyHostToDevice, h->stream);
  }
  if (er == hipSuccess) er = fmx_dev_alloc(&s.row_ptr, ((size_t)n_rows + 1) * sizeof(uint64_t));
  if (er == hipSuccess) er = hipMemcpyAsync(s.row_ptr, up_ptr, ((size_t)n_rows + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream);
  if (er == hipSuccess && target) {
    er = fmx_dev_alloc(&s.target, std::max<uint32_t>(n_rows, 1) * sizeof(float));
    if (er == hipSuccess && n_rows) er = hipMemcpyAsync(s.target, target, (size_t)n_rows * sizeof(float), hipMemcpyHostToDevice, h->stream);
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess && er == hipSuccess) er = hipGetLastError();   // the host buffers may go away after return
  if (er != hipSuccess) { free_slot(s); return fail(h, FMX_E_HIP, "fmx_upload_rows: %s", hipGetErrorString(er)); }
  s.n_rows = n_rows; s.nnz = up_nnz; s.max_row = max_row; s.used = true;
  s.fixed_nnz = (n_rows && min_row == max_row && max_row > 0) ? max_row : 0u;
  h->slots[slot] = s;
  return FMX_OK;
}

// The kept blocks of a slot whose main rows are in place (FMX_BLOCKS_KEEP): every block's own rows, the mapping and its inverse.
// A feature shard keeps the block attributes it owns -- owner = the shard rule on the global id attr_offset + j -- and their ids
// become its local table rows (the block's attr_offset is 0 there, so the kernels read w, V and the groups at the local row);
// the mapping and its inverse depend on the rows alone and are the same on every shard, a block none of whose attributes the
// shard owns included.
extern "C++" int attach_kept_blocks(fmx_handle h, int slot, uint32_t n_rows, const fmx_relation* relations, uint32_t n_relations) {
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[slot];
  const bool sharded = h->cfg.shard_world > 1;
  const Shard sh = make_shard(h->cfg);
  for (uint32_t r = 0; r < n_relations; r++) {
    const fmx_relation& q = relations[r];
    BlockRows* b = new BlockRows();
    s.blocks.push_back(b);
    const Entry* qe = static_cast<const Entry*>(q.entries);
    const uint64_t* qp = q.row_ptr;
    uint64_t qnnz = q.nnz;
    std::vector<Entry> le;
    std::vector<uint64_t> lp;
    if (sharded) {
      lp.resize((size_t)q.n_rows + 1);
      le.reserve((size_t)(q.nnz / h->cfg.shard_world + 1));
      for (uint32_t i = 0; i < q.n_rows; i++) {
        lp[i] = le.size();
        for (uint64_t t = q.row_ptr[i]; t < q.row_ptr[i + 1]; t++) {
          Entry e;
          if (sh.place((uint32_t)(qe[t].id + q.attr_offset), &e.id)) { e.value = qe[t].value; le.push_back(e); }
        }
      }
      lp[q.n_rows] = le.size();
      qe = le.data(); qp = lp.data(); qnnz = le.size();
    }
    b->attr_offset = sharded ? 0u : (uint32_t)q.attr_offset;
    std::vector<uint32_t> cnt((size_t)q.n_rows + 1, 0), list(std::max<uint32_t>(n_rows, 1));
    for (uint32_t c = 0; c < n_rows; c++) cnt[q.data_row_to_relation_row[c] + 1]++;
    for (uint32_t i = 0; i < q.n_rows; i++) cnt[i + 1] += cnt[i];
    { std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
      for (uint32_t c = 0; c < n_rows; c++) list[fill[q.data_row_to_relation_row[c]]++] = c; }   // ascending main row inside a block row
    uint32_t max_row = 0;
    for (uint32_t i = 0; i < q.n_rows; i++) max_row = std::max<uint32_t>(max_row, (uint32_t)(qp[i + 1] - qp[i]));
    hipError_t er = fmx_dev_alloc(&b->rows.ent, std::max<uint64_t>(qnnz, 1) * sizeof(Entry));
    if (er == hipSuccess && qnnz) er = hipMemcpy(b->rows.ent, qe, qnnz * sizeof(Entry), hipMemcpyHostToDevice);
    if (er == hipSuccess) er = fmx_dev_alloc(&b->rows.row_ptr, ((size_t)q.n_rows + 1) * sizeof(uint64_t));
    if (er == hipSuccess) er = hipMemcpy(b->rows.row_ptr, qp, ((size_t)q.n_rows + 1) * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (er == hipSuccess) er = fmx_dev_alloc(&b->map, std::max<uint32_t>(n_rows, 1) * sizeof(uint32_t));
    if (er == hipSuccess && n_rows) er = hipMemcpy(b->map, q.data_row_to_relation_row, (size_t)n_rows * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (er == hipSuccess) er = fmx_dev_alloc(&b->brow_ptr, cnt.size() * sizeof(uint32_t));
    if (er == hipSuccess) er = hipMemcpy(b->brow_ptr, cnt.data(), cnt.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (er == hipSuccess) er = fmx_dev_alloc(&b->brow_list, list.size() * sizeof(uint32_t));
    if (er == hipSuccess) er = hipMemcpy(b->brow_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (er == hipSuccess) er = fmx_dev_alloc(&b->pbuf, std::max<size_t>((size_t)q.n_rows, 1) * (size_t)(h->KP + 1) * sizeof(float));
    if (er != hipSuccess) { free_slot(s); return fail(h, FMX_E_HIP, "fmx_upload_block_rows_ex: %s", hipGetErrorString(er)); }
    b->rows.n_rows = q.n_rows; b->rows.nnz = qnnz; b->rows.max_row = max_row; b->rows.used = true;
  }
  return FMX_OK;
}

// FMX_BLOCKS_KEEP: the main rows and every block stay apart on the device -- nothing of the size of the joined table is
// built.  fm_model::predict and the ALS / MCMC sweeps then work block-wise (fmx_als.hip, k_rel_*).
static int upload_blocks_kept(fmx_handle h, int slot, const void* entries, const uint64_t* row_ptr, const float* target,
                              uint32_t n_rows, uint64_t nnz, const fmx_relation* relations, uint32_t n_relations) {
  int rc = fmx_upload_rows(h, slot, entries, row_ptr, target, n_rows, nnz);          // the main rows as any other data set
  if (rc) return rc;
  return attach_kept_blocks(h, slot, n_rows, relations, n_relations);
}

// what fmx_upload_block_rows_ex checks before anything reaches the device (fmx_group_upload_block_rows_ex checks the same)
extern "C++" int check_block_rows(fmx_handle h, const void* entries, const uint64_t* row_ptr, uint32_t n_rows, uint64_t nnz,
                     const fmx_relation* relations, uint32_t n_relations) {
  if (!relations || n_relations > FMX_MAX_RELATIONS) return fail(h, FMX_E_ARG, "fmx_upload_block_rows: 1..%d relations", FMX_MAX_RELATIONS);
  if (!row_ptr || (nnz > 0 && !entries)) return fail(h, FMX_E_ARG, "fmx_upload_block_rows: null entries/row_ptr");
  if (row_ptr[0] != 0 || row_ptr[n_rows] != nnz) return fail(h, FMX_E_ARG, "row_ptr[0] must be 0 and row_ptr[n_rows] == nnz");
  const uint64_t n = h->cfg.num_attribute;
  const Entry* src = static_cast<const Entry*>(entries);
  for (uint64_t i = 0; i < nnz; i++)
    if (src[i].id >= n) return fail(h, FMX_E_ARG, "feature id %u >= num_attribute %llu", src[i].id, (unsigned long long)n);
  for (uint32_t r = 0; r < n_relations; r++) {
    const fmx_relation& q = relations[r];
    if (!q.row_ptr || !q.data_row_to_relation_row || (q.nnz && !q.entries) || q.row_ptr[0] != 0 || q.row_ptr[q.n_rows] != q.nnz)
      return fail(h, FMX_E_ARG, "relation %u: malformed rows", r);
    const Entry* qe = static_cast<const Entry*>(q.entries);
    for (uint64_t i = 0; i < q.nnz; i++)
      if ((uint64_t)qe[i].id + q.attr_offset >= n)
        return fail(h, FMX_E_ARG, "relation %u: attribute %u + offset %llu >= num_attribute %llu", r, qe[i].id,
                    (unsigned long long)q.attr_offset, (unsigned long long)n);
    for (uint32_t c = 0; c < n_rows; c++)
      if (q.data_row_to_relation_row[c] >= q.n_rows)
        return fail(h, FMX_E_ARG, "relation %u: main row %u maps to block row %u >= %u", r, c, q.data_row_to_relation_row[c], q.n_rows);
  }
  return FMX_OK;
}

int fmx_upload_block_rows(fmx_handle h, int slot, const void* entries, const uint64_t* row_ptr, const float* target,
                          uint32_t n_rows, uint64_t nnz, const fmx_relation* relations, uint32_t n_relations) {
  return fmx_upload_block_rows_ex(h, slot, entries, row_ptr, target, n_rows, nnz, relations, n_relations, FMX_BLOCKS_EXPAND);
}

int fmx_upload_block_rows_ex(fmx_handle h, int slot, const void* entries, const uint64_t* row_ptr, const float* target,
                             uint32_t n_rows, uint64_t nnz, const fmx_relation* relations, uint32_t n_relations, uint32_t flags) {
  if (!h) return FMX_E_ARG;
  if (n_relations == 0) return fmx_upload_rows(h, slot, entries, row_ptr, target, n_rows, nnz);
  if (slot < 0 || slot >= FMX_MAX_SLOTS) return fail(h, FMX_E_ARG, "slot %d out of range", slot);
  { int _rc = slot_in_session(h, slot, "fmx_upload_block_rows"); if (_rc) return _rc; }
  if (!relations || n_relations > FMX_MAX_RELATIONS) return fail(h, FMX_E_ARG, "fmx_upload_block_rows: 1..%d relations", FMX_MAX_RELATIONS);
  if (h->cfg.shard_world > 1 && (flags & FMX_BLOCKS_KEEP))          // (kept blocks need the group's global view)
    return fail(h, FMX_E_UNSUPPORTED, "kept relation blocks on a feature shard go through fmx_group_upload_block_rows_ex (or upload them with FMX_BLOCKS_EXPAND)");
  { int _rc = check_block_rows(h, entries, row_ptr, n_rows, nnz, relations, n_relations); if (_rc) return _rc; }
  const Entry* src = static_cast<const Entry*>(entries);
  if (flags & FMX_BLOCKS_KEEP) return upload_blocks_kept(h, slot, entries, row_ptr, target, n_rows, nnz, relations, n_relations);
  if (h->cfg.shard_world > 1) {
    // a feature shard: the joined rows (main entries, then every block's mapped row with its ids shifted, libfm.cpp:213-216) are
    // built on the host and go through fmx_upload_rows, which keeps the shard's own features like for any rows
    std::vector<uint64_t> jp((size_t)n_rows + 1, 0);
    for (uint32_t c = 0; c < n_rows; c++) {
      uint64_t sz = row_ptr[c + 1] - row_ptr[c];
      for (uint32_t r = 0; r < n_relations; r++) { const uint32_t b = relations[r].data_row_to_relation_row[c]; sz += relations[r].row_ptr[b + 1] - relations[r].row_ptr[b]; }
      jp[c + 1] = jp[c] + sz;
    }
    std::vector<Entry> je((size_t)jp[n_rows]);
    for (uint32_t c = 0; c < n_rows; c++) {
      uint64_t o = jp[c];
      for (uint64_t i = row_ptr[c]; i < row_ptr[c + 1]; i++) je[o++] = src[i];
      for (uint32_t r = 0; r < n_relations; r++) {
        const fmx_relation& q = relations[r];
        const Entry* qe = static_cast<const Entry*>(q.entries);
        const uint32_t b = q.data_row_to_relation_row[c];
        for (uint64_t i = q.row_ptr[b]; i < q.row_ptr[b + 1]; i++) { Entry e = qe[i]; e.id += (uint32_t)q.attr_offset; je[o++] = e; }
      }
    }
    return fmx_upload_rows(h, slot, je.data(), jp.data(), target, n_rows, jp[n_rows]);
  }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_interactions(h, slot);
  free_slot(h->slots[slot]);
  std::vector<void*> tmp;                                     // staging buffers, freed on every exit path
  auto up = [&](const void* p, size_t bytes) -> void* {
    void* d = nullptr;
    if (fmx_dev_alloc(&d, std::max<size_t>(bytes, 8)) != hipSuccess) return nullptr;
    tmp.push_back(d);
    if (bytes && hipMemcpy(d, p, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
  };
  Slot s;
  bool committed = false;
  auto cleanup = [&]() { for (void* d : tmp) fmx_dev_free(d); if (!committed) free_slot(s); };
#define BLK_CHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { cleanup(); return fail(h, FMX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); } } while (0)
#define BLK_UP(dst, type, p, bytes) do { dst = (type)up((p), (bytes)); if (!dst) { cleanup(); return fail(h, FMX_E_HIP, "fmx_upload_block_rows: staging %s failed", #p); } } while (0)
  const Entry* d_ent; const uint64_t* d_ptr;
  BLK_UP(d_ent, const Entry*, entries, nnz * sizeof(Entry));
  BLK_UP(d_ptr, const uint64_t*, row_ptr, ((size_t)n_rows + 1) * sizeof(uint64_t));
  BlockRels rels;
  memset(&rels, 0, sizeof(rels));
  rels.n = n_relations;
  for (uint32_t r = 0; r < n_relations; r++) {
    const fmx_relation& q = relations[r];
    BLK_UP(rels.r[r].ent, const Entry*, q.entries, q.nnz * sizeof(Entry));
    BLK_UP(rels.r[r].row_ptr, const uint64_t*, q.row_ptr, ((size_t)q.n_rows + 1) * sizeof(uint64_t));
    BLK_UP(rels.r[r].map, const uint32_t*, q.data_row_to_relation_row, (size_t)n_rows * sizeof(uint32_t));
    rels.r[r].attr_offset = (uint32_t)q.attr_offset;
  }
  uint64_t* sizes = nullptr;
  BLK_CHK(fmx_dev_alloc(&sizes, ((size_t)n_rows + 1) * sizeof(uint64_t)));
  tmp.push_back(sizes);
  BLK_CHK(fmx_dev_alloc(&s.row_ptr, ((size_t)n_rows + 1) * sizeof(uint64_t)));
  const dim3 g1(std::min<uint32_t>((n_rows + 256) / 256, 2048)), b1(256);
  hipLaunchKernelGGL(k_block_sizes, g1, b1, 0, h->stream, d_ptr, n_rows, rels, sizes);
  size_t scan_bytes = 0;
  BLK_CHK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, sizes, s.row_ptr, (int)(n_rows + 1), h->stream));
  void* scan_tmp = nullptr;
  BLK_CHK(fmx_dev_alloc(&scan_tmp, std::max<size_t>(scan_bytes, 8)));
  tmp.push_back(scan_tmp);
  BLK_CHK(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, sizes, s.row_ptr, (int)(n_rows + 1), h->stream));
  std::vector<uint64_t> hs((size_t)n_rows + 1);
  uint64_t total = 0;
  BLK_CHK(hipMemcpyAsync(hs.data(), sizes, hs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  BLK_CHK(hipMemcpyAsync(&total, s.row_ptr + n_rows, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  BLK_CHK(hipStreamSynchronize(h->stream));
  uint32_t max_row = 0;
  for (uint32_t c = 0; c < n_rows; c++) max_row = std::max<uint32_t>(max_row, (uint32_t)hs[c]);
  BLK_CHK(fmx_dev_alloc(&s.ent, std::max<uint64_t>(total, 1) * sizeof(Entry)));
  hipLaunchKernelGGL(k_block_fill, g1, b1, 0, h->stream, d_ent, d_ptr, n_rows, rels, s.row_ptr, s.ent);
  BLK_CHK(hipGetLastError());
  if (target) {
    BLK_CHK(fmx_dev_alloc(&s.target, std::max<uint32_t>(n_rows, 1) * sizeof(float)));
    if (n_rows) BLK_CHK(hipMemcpy(s.target, target, (size_t)n_rows * sizeof(float), hipMemcpyHostToDevice));
  }
  BLK_CHK(hipStreamSynchronize(h->stream));
#undef BLK_CHK
#undef BLK_UP
  committed = true;
  cleanup();
  s.n_rows = n_rows; s.nnz = total; s.max_row = max_row; s.used = true;
  h->slots[slot] = s;
  return FMX_OK;
}

int fmx_rows_info(fmx_handle h, int slot, uint32_t* n_rows, uint64_t* nnz) {
  int rc = check_slot(h, slot, false);
  if (rc) return rc;
  if (n_rows) *n_rows = h->slots[slot].n_rows;
  if (nnz) *nnz = h->slots[slot].nnz;
  return FMX_OK;
}

int fmx_wtrain_info(fmx_handle h, int slot, uint64_t* singles, int* kept) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_wtrain_info"); if (_sr) return _sr; }
  int rc = check_slot(h, slot, false);
  if (rc) return rc;
  if (singles) *singles = h->slots[slot].wtrain_n;
  if (kept) *kept = h->slots[slot].wtrain != nullptr;
  return FMX_OK;
}

int fmx_download_rows(fmx_handle h, int slot, void* entries, uint64_t* row_ptr, float* target) {
  int rc = check_slot(h, slot, false);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const Slot& s = h->slots[slot];
  if (entries && s.nnz) HIPCHK(h, hipMemcpy(entries, s.ent, s.nnz * sizeof(Entry), hipMemcpyDeviceToHost));
  if (row_ptr) HIPCHK(h, hipMemcpy(row_ptr, s.row_ptr, ((size_t)s.n_rows + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (target && s.target && s.n_rows) HIPCHK(h, hipMemcpy(target, s.target, (size_t)s.n_rows * sizeof(float), hipMemcpyDeviceToHost));
  return FMX_OK;
}

int fmx_synth_rows(fmx_handle h, int slot, uint64_t seed, uint64_t row0, uint32_t n_rows, uint32_t nnz) {
  return fmx_synth_rows_ex(h, slot, seed, row0, n_rows, nnz, FMX_SYNTH_UNIFORM);
}

int fmx_synth_rows_ex(fmx_handle h, int slot, uint64_t seed, uint64_t row0, uint32_t n_rows, uint32_t nnz, uint32_t shape) {
  if (!h) return FMX_E_ARG;
  if (slot < 0 || slot >= FMX_MAX_SLOTS) return fail(h, FMX_E_ARG, "slot %d out of range", slot);
  { int _rc = slot_in_session(h, slot, "fmx_synth_rows"); if (_rc) return _rc; }
  if (nnz == 0 || n_rows == 0) return fail(h, FMX_E_ARG, "fmx_synth_rows: empty workload");
  if (shape != FMX_SYNTH_UNIFORM && shape != FMX_SYNTH_CRITEO) return fail(h, FMX_E_ARG, "fmx_synth_rows_ex: unknown shape %u", shape);
  const uint64_t n = h->cfg.num_attribute;
  uint32_t fs = (uint32_t)(n / nnz);
  if (shape == FMX_SYNTH_CRITEO) {
    const uint64_t dense = (uint64_t)SYNTH_DENSE_FIELDS * SYNTH_DENSE_IDS;
    if (nnz <= SYNTH_DENSE_FIELDS || n < dense + (nnz - SYNTH_DENSE_FIELDS))
      return fail(h, FMX_E_ARG, "fmx_synth_rows_ex: the Criteo shape needs nnz > 13 and num_attribute >= 1300 + (nnz - 13)");
    fs = (uint32_t)((n - dense) / (nnz - SYNTH_DENSE_FIELDS));
  }
  if (fs == 0) return fail(h, FMX_E_ARG, "fmx_synth_rows: num_attribute < nnz");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_interactions(h, slot);
  free_slot(h->slots[slot]);
  const Shard sh = make_shard(h->cfg);
  Slot s;
  uint32_t* cnt = nullptr;
  void* tmp = nullptr;
  uint64_t total = 0;
  // every error path releases what was allocated so far
#define SYN_CHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { if (cnt) fmx_dev_free(cnt); if (tmp) fmx_dev_free(tmp); free_slot(s); \
    return fail(h, FMX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); } } while (0)
  SYN_CHK(fmx_dev_alloc(&cnt, ((size_t)n_rows + 1) * sizeof(uint32_t)));
  SYN_CHK(hipMemsetAsync(cnt, 0, ((size_t)n_rows + 1) * sizeof(uint32_t), h->stream));
  SYN_CHK(fmx_dev_alloc(&s.row_ptr, ((size_t)n_rows + 1) * sizeof(uint64_t)));
  SYN_CHK(fmx_dev_alloc(&s.target, (size_t)n_rows * sizeof(float)));
  const dim3 grid((n_rows + 255) / 256), block(256);
  hipLaunchKernelGGL(k_synth, grid, block, 0, h->stream, seed, row0, n_rows, nnz, fs, shape, sh, cnt,
                     (const uint64_t*)nullptr, (Entry*)nullptr, s.target);
  SYN_CHK(hipGetLastError());
  {  // exclusive prefix sum u32 -> u64 over n_rows+1 items (last = total)
    size_t tmp_bytes = 0;
    auto conv = hipcub::TransformInputIterator<uint64_t, hipcub::CastOp<uint64_t>, uint32_t*>(cnt, hipcub::CastOp<uint64_t>());
    SYN_CHK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, conv, s.row_ptr, (int)(n_rows + 1), h->stream));
    SYN_CHK(fmx_dev_alloc(&tmp, tmp_bytes));
    SYN_CHK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, conv, s.row_ptr, (int)(n_rows + 1), h->stream));
    SYN_CHK(hipStreamSynchronize(h->stream));
    fmx_dev_free(tmp); tmp = nullptr;
  }
  SYN_CHK(hipMemcpy(&total, s.row_ptr + n_rows, sizeof(uint64_t), hipMemcpyDeviceToHost));
  SYN_CHK(fmx_dev_alloc(&s.ent, std::max<uint64_t>(total, 1) * sizeof(Entry)));
  hipLaunchKernelGGL(k_synth, grid, block, 0, h->stream, seed, row0, n_rows, nnz, fs, shape, sh, (uint32_t*)nullptr,
                     (const uint64_t*)s.row_ptr, s.ent, (float*)nullptr);
  SYN_CHK(hipGetLastError());
  SYN_CHK(hipStreamSynchronize(h->stream));
#undef SYN_CHK
  fmx_dev_free(cnt);
  s.n_rows = n_rows; s.nnz = total; s.max_row = nnz; s.used = true;
  s.fixed_nnz = (h->cfg.shard_world == 1) ? nnz : 0u;        // (a shard keeps a varying part of every row)
  h->slots[slot] = s;
  return FMX_OK;
}

// ---------------------------------------------------------------------------------------------
// predict / evaluate
// ---------------------------------------------------------------------------------------------
int fmx_predict(fmx_handle h, int slot, double* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_predict"); if (_sr) return _sr; }
  int rc = check_slot(h, slot, false); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_predict: out is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  return predict_out(h, h->slots[slot], nullptr, out);
}

int fmx_evaluate(fmx_handle h, int slot, fmx_eval* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_evaluate"); if (_sr) return _sr; }
  int rc = check_slot(h, slot, true); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_evaluate: out is NULL");
  if (h->cfg.shard_world > 1) return fail(h, FMX_E_UNSUPPORTED, "fmx_evaluate on a feature shard: use fmx_sgd_partial + all-reduce + fmx_predict_finish");
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  memset(out, 0, sizeof(*out));
  out->rows = s.n_rows;
  if (s.n_rows == 0) return FMX_OK;
  if (s.wside && s.wside_version == h->w_version && s.blocks.empty()) out->flags |= FMX_EVAL_WSIDE;
  return evaluate_out(h, s, nullptr, out);
}

}  // extern "C"
