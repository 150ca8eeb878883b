// fmx_compact.hip -- C-ABI (include/fmx.h "fmx_compact_*"): a frozen bf16 or int8 copy of the model to score from (DESIGN.md sections
// 19, 21).  fmx_compact_begin quantises V in one pass (k_compact_quant, and copies w; or k_compact_quant8, which puts w in the row) and
// copies w0; predict / evaluate / evaluate_ex / topk / get_rows are their own checks and then the fp32 entry points' code with the
// snapshot named as the rows' source (slot_scores, predict_out, evaluate_out, eval_ex_scores, topk_impl, gather_rows: k_rowsums and
// k_fetch_rows over RowsBf16 / RowsI8).  fmx_compact_begin_pruned keeps only the rows that can score: a rank
// directory first (prune_directory), then the same quantisers with a destination map; the scoring calls read through RowsBf16P / RowsI8P.
// Kernels: fmx_compact_kernels.h.
#include "fmx_internal.h"

namespace {

// what every entry point checks first: an unsharded handle, and (all but _begin) a snapshot
int compact_check(fmx_handle h, const char* who, bool need_snapshot) {
  if (h->cfg.shard_world > 1 || h->comm)
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", who);
  if (need_snapshot && !h->compact.w0) return fail(h, FMX_E_STATE, "%s before fmx_compact_begin", who);
  return FMX_OK;
}

// a slot the snapshot can score: uploaded, with targets where they are needed, without kept blocks
int compact_check_slot(fmx_handle h, const char* who, int slot, bool need_target) {
  if (slot < 0 || slot >= FMX_MAX_SLOTS) return fail(h, FMX_E_ARG, "%s: slot %d out of range", who, slot);
  const Slot& s = h->slots[slot];
  if (!s.used) return fail(h, FMX_E_STATE, "%s: slot %d holds no rows (call fmx_upload_rows first)", who, slot);
  if (need_target && !s.target) return fail(h, FMX_E_STATE, "%s: slot %d was uploaded without targets", who, slot);
  if (!s.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "%s: slots with kept `-relation` blocks are not supported", who);
  return FMX_OK;
}

// The rank directory of a pruned snapshot: which features keep a row (not dead; with `keep`, also met in that slot's entries) and where.
// Device memory beside the directory itself: two bit arrays and the popcounts of its size class and hipcub's scan scratch, all freed
// before the rows are allocated.  *dir_out is a plain allocation the caller owns; *kept the rows to allocate.
hipError_t prune_directory(fmx_handle h, const Slot* keep, uint2** dir_out, uint64_t* kept, fmx_compact_prune_info* pi) {
  const uint64_t n = h->n_local, nwords = (n + 31) / 32;
  uint32_t *live = nullptr, *seen = nullptr, *cnt = nullptr;
  unsigned long long* ctr = nullptr;                             // {dead, unseen}
  void* tmp = nullptr;
  uint2* dir = nullptr;
  size_t tmp_bytes = 0;
  const unsigned gw = (unsigned)std::min<uint64_t>((nwords + 255) / 256, COMPACT_BLOCKS);
  hipError_t er = fmx_dev_alloc_plain(&dir, (size_t)nwords * sizeof(uint2));
  if (er == hipSuccess) er = fmx_dev_alloc(&live, (size_t)nwords * 4);
  if (er == hipSuccess) er = fmx_dev_alloc(&cnt, (size_t)nwords * 4);
  if (er == hipSuccess) er = fmx_dev_alloc(&ctr, 16);
  if (er == hipSuccess) er = hipMemsetAsync(ctr, 0, 16, h->stream);
  if (er == hipSuccess && keep) {
    er = fmx_dev_alloc(&seen, (size_t)nwords * 4);
    if (er == hipSuccess) er = hipMemsetAsync(seen, 0, (size_t)nwords * 4, h->stream);
  }
  if (er == hipSuccess) er = hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt, cnt, (int)nwords, h->stream);
  if (er == hipSuccess) er = fmx_dev_alloc_bytes(&tmp, std::max<size_t>(tmp_bytes, 8));
  unsigned long long host_ctr[2] = {0ull, 0ull};
  uint32_t last[2] = {0u, 0u};
  if (er == hipSuccess) {
    hipLaunchKernelGGL(k_prune_live, dim3((unsigned)std::min<uint64_t>((nwords + 3) / 4, COMPACT_BLOCKS)), dim3(256), 0, h->stream,
                       (const float*)h->tb.V, (const float*)h->tb.w, h->tb.rs, n, h->cfg.num_factor, h->cfg.k1, live, ctr);
    if (keep && keep->nnz > 0)
      hipLaunchKernelGGL(k_prune_mark, dim3((unsigned)std::min<uint64_t>((keep->nnz + 255) / 256, COMPACT_BLOCKS)), dim3(256), 0, h->stream,
                         (const Entry*)keep->ent, keep->nnz, n, seen);
    hipLaunchKernelGGL(k_prune_keep, dim3(gw), dim3(256), 0, h->stream, live, (const uint32_t*)seen, nwords, cnt, ctr + 1);
    er = hipGetLastError();
    // (the last word's popcount is taken before the scan overwrites it in place)
    if (er == hipSuccess) er = hipMemcpyAsync(&last[1], cnt + (nwords - 1), 4, hipMemcpyDeviceToHost, h->stream);
    if (er == hipSuccess) er = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, cnt, (int)nwords, h->stream);
    if (er == hipSuccess) {
      hipLaunchKernelGGL(k_prune_dir, dim3(gw), dim3(256), 0, h->stream, (const uint32_t*)live, (const uint32_t*)cnt, nwords, dir);
      er = hipGetLastError();
    }
    if (er == hipSuccess) er = hipMemcpyAsync(&last[0], cnt + (nwords - 1), 4, hipMemcpyDeviceToHost, h->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(host_ctr, ctr, 16, hipMemcpyDeviceToHost, h->stream);
  }
  { const hipError_t es = hipStreamSynchronize(h->stream);       // (also on an error: a queued kernel may still write the temporaries)
    if (er == hipSuccess) er = es; }
  fmx_dev_free(live); fmx_dev_free(seen); fmx_dev_free(cnt); fmx_dev_free(ctr); fmx_dev_free(tmp);
  if (er != hipSuccess) { fmx_dev_free(dir); return er; }
  *dir_out = dir;
  *kept = (uint64_t)last[0] + last[1];
  memset(pi, 0, sizeof(*pi));
  pi->features = n;
  pi->kept = *kept;
  pi->dropped_dead = host_ctr[0];
  pi->dropped_unseen = host_ctr[1];
  pi->bytes_directory = nwords * sizeof(uint2);
  return hipSuccess;
}

// fmx_compact_begin and fmx_compact_begin_pruned behind their own checks.  pinfo != nullptr: a pruned snapshot (keep: the slot whose
// entries say which features were seen, or nullptr) -- the directory first, then the quantisers write row id to its slot.
int compact_build(fmx_handle h, const char* who, uint32_t format, const Slot* keep, fmx_compact_info* info, fmx_compact_prune_info* pinfo) {
  if (h->tb.ws != 1) return fail(h, FMX_E_UNSUPPORTED, "%s: the linear weights are not an array of their own", who);
  { int _rc = lag_flush(h); if (_rc) return _rc; }              // (the copy is of the parameters as they stand: they have to be current)
  HIPCHK(h, hipSetDevice(h->device));
  const uint64_t n = h->n_local;
  const uint32_t rs = h->tb.rs;
  const int k = h->cfg.num_factor;
  const bool i8 = format == FMX_COMPACT_INT8;
  const uint32_t P = compact8_row_bytes((uint32_t)k);           // int8: bytes of a feature's block
  uint32_t L = (uint32_t)std::min(h->KP, 64);                   // lanes per feature: a power of two
  if (i8) { L = 2; while (L < 64 && L < P / 4) L <<= 1; }       // (int8: one lane per dword of the block, QUANT8_T dwords at most)
  // the new snapshot is built beside the old one, which is replaced only when everything has succeeded
  CompactState c;
  c.format = format;
  uint64_t rows = n;                                            // rows the tables hold
  if (pinfo) {
    if ((n + 31) / 32 > 0x7FFFFFFFull) return fail(h, FMX_E_UNSUPPORTED, "%s: more than 2^36 features", who);
    const hipError_t e = prune_directory(h, keep, &c.dir, &rows, pinfo);
    if (e != hipSuccess) return fail(h, FMX_E_HIP, "%s: the directory: %s", who, hipGetErrorString(e));
    c.kept = rows;
  }
  const uint64_t bytes_rows = i8 ? rows * (uint64_t)P : rows * (2 * (uint64_t)rs + 4);
  const uint64_t bytes = bytes_rows + (pinfo ? pinfo->bytes_directory : 0);
  const uint64_t waves = (n + 64 / L - 1) / (64 / L);
  const uint32_t nblk = (uint32_t)std::min<uint64_t>((waves + 3) / 4, COMPACT_BLOCKS);
  void* part = nullptr;                                         // [nblk][2] doubles, [nblk] counts, then 2 doubles and 1 count
  // Plain allocations, not the chunked ranges fmx_dev_alloc builds from 768 MiB on.  A snapshot that replaces another takes its memory
  // milliseconds after a range of the same size went back, and physical chunks handed out again that soon have been seen to lose what
  // was just written to them (a 4 GB int8 snapshot taken in turns with a bf16 one read back as zeros).
  // (a pruned snapshot that keeps nothing still gets tables of one row, which no lookup reaches)
  const size_t arows = (size_t)std::max<uint64_t>(rows, 1);
  hipError_t er = hipSuccess;
  if (i8) { c.P = P; er = fmx_dev_alloc_plain(&c.B, arows * P); }
  else {
    er = fmx_dev_alloc_plain(&c.V, arows * rs * sizeof(uint16_t));
    if (er == hipSuccess) er = fmx_dev_alloc_plain(&c.w, arows * sizeof(float));
  }
  if (er == hipSuccess) er = fmx_dev_alloc(&c.w0, sizeof(double));
  if (er == hipSuccess) er = fmx_dev_alloc(&part, ((size_t)nblk * 3 + 3) * 8);
  struct { double d[2]; unsigned long long c; } res = {{0.0, 0.0}, 0ull};
  if (er == hipSuccess) {
    double* dpart = (double*)part;
    unsigned long long* cpart = (unsigned long long*)part + (size_t)nblk * 2;
    double* dres = (double*)part + (size_t)nblk * 3;
    const float* V = (const float*)h->tb.V; const float* w = (const float*)h->tb.w;
    const uint2* dir = c.dir;
    if (i8 && dir) hipLaunchKernelGGL(k_compact_quant8<true>, dim3(nblk), dim3(256), 0, h->stream, V, w, rs, n, k, L, P, c.B, dpart, cpart, dir);
    else if (i8) hipLaunchKernelGGL(k_compact_quant8<false>, dim3(nblk), dim3(256), 0, h->stream, V, w, rs, n, k, L, P, c.B, dpart, cpart, dir);
    else if (dir) hipLaunchKernelGGL(k_compact_quant<true>, dim3(nblk), dim3(256), 0, h->stream, V, rs, n, k, L, c.V, dpart, cpart, dir, w, c.w);
    else hipLaunchKernelGGL(k_compact_quant<false>, dim3(nblk), dim3(256), 0, h->stream, V, rs, n, k, L, c.V, dpart, cpart, dir, w, c.w);
    hipLaunchKernelGGL(k_compact_final, dim3(1), dim3(64), 0, h->stream, (const double*)dpart, (const unsigned long long*)cpart, nblk,
                       dres, (unsigned long long*)(dres + 2));
    er = hipGetLastError();
    if (er == hipSuccess && !i8 && !dir) er = hipMemcpyAsync(c.w, h->tb.w, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(c.w0, h->w0, sizeof(double), hipMemcpyDeviceToDevice, h->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(&res, dres, sizeof(res), hipMemcpyDeviceToHost, h->stream);
  }
  if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  fmx_dev_free(part);
  if (er != hipSuccess) {
    compact_release(c);
    return fail(h, FMX_E_HIP, "%s: the snapshot (%zu bytes): %s", who, (size_t)bytes, hipGetErrorString(er));
  }
  c.nonfinite = res.c; c.max_abs_err = res.d[0]; c.sum_sq_err = res.d[1];       // (kept for fmx_compact_save's header)
  if (pinfo) { c.dropped_dead = pinfo->dropped_dead; c.dropped_unseen = pinfo->dropped_unseen; }
  compact_release(h->compact);
  h->compact = c;
  if (pinfo) pinfo->bytes_rows = bytes_rows;
  if (info) {
    memset(info, 0, sizeof(*info));
    info->features = n;
    info->bytes_compact = bytes;
    info->bytes_params = h->n_local * (size_t)(h->tb.rs + (h->w_sep ? 1 : 0)) * sizeof(float);   // fmx_get_info
    info->nonfinite = res.c;
    info->max_abs_err = res.d[0];
    info->sum_sq_err = res.d[1];
  }
  return FMX_OK;
}

}  // namespace

void compact_release(CompactState& c) {
  fmx_dev_free(c.V); fmx_dev_free(c.w); fmx_dev_free(c.w0); fmx_dev_free(c.B); fmx_dev_free(c.dir);
  c = CompactState();
}

void compact_free(fmx_handle h) { compact_release(h->compact); }

extern "C" {

uint32_t fmx_compact_row_bytes(uint32_t format, int num_factor) {
  if (num_factor < 0) return 0;
  if (format == FMX_COMPACT_BF16) {                              // the rs of fmx_create (fmx_core.hip), 2 bytes an element, and w
    const uint32_t KP = (uint32_t)pow2_ge(std::max(num_factor, 1));
    const uint32_t rs = KP >= 32 ? std::min(KP, ((uint32_t)num_factor + 15u) / 16u * 16u) : KP;
    return 2 * rs + 4;
  }
  if (format == FMX_COMPACT_INT8) return compact8_row_bytes((uint32_t)num_factor);
  return 0;
}

int fmx_compact_begin(fmx_handle h, const fmx_compact_opts* opts, fmx_compact_info* info) {
  static const char who[] = "fmx_compact_begin";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_compact_begin"); if (_sr) return _sr; }
  if (!opts) return fail(h, FMX_E_ARG, "%s: opts is NULL", who);
  if (opts->format != FMX_COMPACT_BF16 && opts->format != FMX_COMPACT_INT8)
    return fail(h, FMX_E_ARG, "%s: unknown format %u (FMX_COMPACT_BF16, FMX_COMPACT_INT8)", who, opts->format);
  if (opts->flags != 0) return fail(h, FMX_E_ARG, "%s: flags must be 0 (got %u)", who, opts->flags);
  int rc = compact_check(h, who, false); if (rc) return rc;
  return compact_build(h, who, opts->format, nullptr, info, nullptr);
}

int fmx_compact_begin_pruned(fmx_handle h, const fmx_compact_prune_opts* o, fmx_compact_info* info, fmx_compact_prune_info* pinfo) {
  static const char who[] = "fmx_compact_begin_pruned";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_compact_begin_pruned"); if (_sr) return _sr; }
  if (!o) return fail(h, FMX_E_ARG, "%s: opts is NULL", who);
  if (o->format != FMX_COMPACT_BF16 && o->format != FMX_COMPACT_INT8)
    return fail(h, FMX_E_ARG, "%s: unknown format %u (FMX_COMPACT_BF16, FMX_COMPACT_INT8)", who, o->format);
  if (!(o->flags & FMX_PRUNE_DEAD) || (o->flags & ~(FMX_PRUNE_DEAD | FMX_PRUNE_SEEN)))
    return fail(h, FMX_E_ARG, "%s: flags 0x%x (FMX_PRUNE_DEAD, or FMX_PRUNE_DEAD | FMX_PRUNE_SEEN)", who, o->flags);
  if (o->reserved != 0) return fail(h, FMX_E_ARG, "%s: reserved must be 0 (got %u)", who, o->reserved);
  const bool seen = (o->flags & FMX_PRUNE_SEEN) != 0;
  if (!seen && o->keep_slot != -1) return fail(h, FMX_E_ARG, "%s: keep_slot = %d without FMX_PRUNE_SEEN (pass -1)", who, o->keep_slot);
  int rc = compact_check(h, who, false); if (rc) return rc;
  if (seen) {
    rc = compact_check_slot(h, who, o->keep_slot, false); if (rc) return rc;
    if (h->slots[o->keep_slot].nnz > 0 && !h->slots[o->keep_slot].ent)
      return fail(h, FMX_E_UNSUPPORTED, "%s: keep_slot %d has no entry stream on the device", who, o->keep_slot);
  }
  fmx_compact_prune_info pi;
  rc = compact_build(h, who, o->format, seen ? &h->slots[o->keep_slot] : (const Slot*)nullptr, info, &pi);
  if (rc == FMX_OK && pinfo) *pinfo = pi;
  return rc;
}

int fmx_compact_slot_of(fmx_handle h, const uint32_t* ids, uint32_t count, uint32_t* slot_out) {
  static const char who[] = "fmx_compact_slot_of";
  if (!h) return FMX_E_ARG;
  if (count > 0 && (!ids || !slot_out)) return fail(h, FMX_E_ARG, "%s: ids / slot_out is NULL", who);
  int rc = compact_check(h, who, true); if (rc) return rc;
  if (!h->compact.dir) return fail(h, FMX_E_STATE, "%s: the snapshot is not a pruned one (fmx_compact_begin_pruned)", who);
  for (uint32_t i = 0; i < count; i++)
    if (ids[i] >= h->cfg.num_attribute) return fail(h, FMX_E_ARG, "%s: feature id %u >= num_attribute", who, ids[i]);
  if (count == 0) return FMX_OK;
  HIPCHK(h, hipSetDevice(h->device));
  uint32_t* d = nullptr;                                         // ids, then slots
  hipError_t er = fmx_dev_alloc(&d, (size_t)count * 8);
  if (er == hipSuccess) er = hipMemcpyAsync(d, ids, (size_t)count * 4, hipMemcpyHostToDevice, h->stream);
  if (er == hipSuccess) {
    hipLaunchKernelGGL(k_prune_slot_of, dim3((count + 255u) / 256u), dim3(256), 0, h->stream, (const uint2*)h->compact.dir, (const uint32_t*)d,
                       count, d + count);
    er = hipGetLastError();
  }
  if (er == hipSuccess) er = hipMemcpyAsync(slot_out, d + count, (size_t)count * 4, hipMemcpyDeviceToHost, h->stream);
  if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  fmx_dev_free(d);
  if (er != hipSuccess) return fail(h, FMX_E_HIP, "%s: %s", who, hipGetErrorString(er));
  return FMX_OK;
}

int fmx_compact_end(fmx_handle h) {
  static const char who[] = "fmx_compact_end";
  if (!h) return FMX_E_ARG;
  int rc = compact_check(h, who, true); if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  compact_free(h);
  return FMX_OK;
}

int fmx_compact_predict(fmx_handle h, int slot, double* out) {
  static const char who[] = "fmx_compact_predict";
  if (!h) return FMX_E_ARG;
  if (!out) return fail(h, FMX_E_ARG, "%s: out is NULL", who);
  int rc = compact_check(h, who, true); if (rc) return rc;
  rc = compact_check_slot(h, who, slot, false); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }              // (the scratch below is shared with a bias-lag epoch still in flight)
  HIPCHK(h, hipSetDevice(h->device));
  return predict_out(h, h->slots[slot], &h->compact, out);
}

int fmx_compact_evaluate(fmx_handle h, int slot, fmx_eval* out) {
  static const char who[] = "fmx_compact_evaluate";
  if (!h) return FMX_E_ARG;
  if (!out) return fail(h, FMX_E_ARG, "%s: out is NULL", who);
  int rc = compact_check(h, who, true); if (rc) return rc;
  rc = compact_check_slot(h, who, slot, true); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }              // (the scratch below is shared with a bias-lag epoch still in flight)
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  memset(out, 0, sizeof(*out));
  out->rows = s.n_rows;
  if (s.n_rows == 0) return FMX_OK;
  return evaluate_out(h, s, &h->compact, out);
}

int fmx_compact_evaluate_ex(fmx_handle h, int slot, const fmx_eval_opts* opts, fmx_eval_ex* out) {
  static const char who[] = "fmx_compact_evaluate_ex";
  if (!h) return FMX_E_ARG;
  if (!out) return fail(h, FMX_E_ARG, "%s: out is NULL", who);
  uint32_t link;
  int rc = eval_ex_check_opts(h, who, opts, &link); if (rc) return rc;
  rc = compact_check(h, who, true); if (rc) return rc;
  rc = eval_ex_check_slot(h, who, slot); if (rc) return rc;
  rc = compact_check_slot(h, who, slot, true); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }              // (the scratch below is shared with a bias-lag epoch still in flight)
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  eval_ex_empty(out);
  if (s.n_rows == 0) return FMX_OK;
  // the finished y-hat with the SNAPSHOT's bias (eval_ex_scores would add the model's): exactly what fmx_compact_predict returns
  const float* yhat;
  rc = slot_scores(h, s, &h->compact, true, &yhat);
  if (rc) return rc;
  return eval_ex_scores(h, s, yhat, 0, link, out);
}

int fmx_compact_topk(fmx_handle h, int query_slot, int cand_slot, const fmx_topk_opts* opts, uint32_t* idx_out, double* score_out,
                     fmx_topk_stats* stats) {
  static const char who[] = "fmx_compact_topk";
  if (!h) return FMX_E_ARG;
  if (stats) memset(stats, 0, sizeof(*stats));
  int rc = compact_check(h, who, true); if (rc) return rc;
  return topk_impl(h, who, query_slot, cand_slot, opts, idx_out, score_out, stats, &h->compact);
}

int fmx_compact_get_rows(fmx_handle h, const uint32_t* ids, uint32_t count, double* w_out, double* v_out) {
  static const char who[] = "fmx_compact_get_rows";
  if (!h) return FMX_E_ARG;
  const int k = h->cfg.num_factor;
  if (!ids || !w_out || (k > 0 && !v_out)) return fail(h, FMX_E_ARG, "%s: ids / w_out / v_out is NULL", who);
  int rc = compact_check(h, who, true); if (rc) return rc;
  for (uint32_t i = 0; i < count; i++)
    if (ids[i] >= h->cfg.num_attribute) return fail(h, FMX_E_ARG, "%s: feature id %u >= num_attribute", who, ids[i]);
  if (count == 0) return FMX_OK;
  double* const outs[1][2] = {{w_out, v_out}};
  return gather_rows(h, who, ids, count, 1, outs, [&](int, dim3 grid, const uint32_t* d_ids, double* d_w, double* d_v) {
    if (h->compact.dir && h->compact.format == FMX_COMPACT_INT8)
      hipLaunchKernelGGL(k_fetch_rows<RowsI8P>, grid, dim3(256), 0, h->stream, d_ids, count, k, make_shard(h->cfg), compact_rows8_p(h->compact), d_w, d_v);
    else if (h->compact.dir)
      hipLaunchKernelGGL(k_fetch_rows<RowsBf16P>, grid, dim3(256), 0, h->stream, d_ids, count, k, make_shard(h->cfg), compact_rows_p(h, h->compact), d_w, d_v);
    else if (h->compact.format == FMX_COMPACT_INT8)
      hipLaunchKernelGGL(k_fetch_rows<RowsI8>, grid, dim3(256), 0, h->stream, d_ids, count, k, make_shard(h->cfg), compact_rows8(h->compact), d_w, d_v);
    else
      hipLaunchKernelGGL(k_fetch_rows<RowsBf16>, grid, dim3(256), 0, h->stream, d_ids, count, k, make_shard(h->cfg), compact_rows(h, h->compact), d_w, d_v);
  });
}

}  // extern "C"
