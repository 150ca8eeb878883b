// fmx_compact.hip -- C-ABI (include/fmx.h "fmx_compact_*"): a frozen bf16 or int8 copy of the model to score from (DESIGN.md sections
// 19, 21).  fmx_compact_begin quantises V in one pass (k_compact_quant, and copies w; or k_compact_quant8, which puts w in the row) and
// copies w0; predict / evaluate / evaluate_ex / topk / get_rows are their own checks and then the fp32 entry points' code with the
// snapshot named as the rows' source (slot_scores, predict_out, evaluate_out, eval_ex_scores, topk_impl, gather_rows: k_rowsums and
// k_fetch_rows over RowsBf16 / RowsI8).  Kernels: fmx_compact_kernels.h.
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

void compact_release(CompactState& c) {
  fmx_dev_free(c.V); fmx_dev_free(c.w); fmx_dev_free(c.w0); fmx_dev_free(c.B);
  c = CompactState();
}

}  // namespace

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
  if (!opts) return fail(h, FMX_E_ARG, "%s: opts is NULL", who);
  if (opts->format != FMX_COMPACT_BF16 && opts->format != FMX_COMPACT_INT8)
    return fail(h, FMX_E_ARG, "%s: unknown format %u (FMX_COMPACT_BF16, FMX_COMPACT_INT8)", who, opts->format);
  if (opts->flags != 0) return fail(h, FMX_E_ARG, "%s: flags must be 0 (got %u)", who, opts->flags);
  int rc = compact_check(h, who, false); if (rc) return rc;
  if (h->tb.ws != 1) return fail(h, FMX_E_UNSUPPORTED, "%s: the linear weights are not an array of their own", who);
  { int _rc = lag_flush(h); if (_rc) return _rc; }              // (the copy is of the parameters as they stand: they have to be current)
  HIPCHK(h, hipSetDevice(h->device));
  const uint64_t n = h->n_local;
  const uint32_t rs = h->tb.rs;
  const int k = h->cfg.num_factor;
  const bool i8 = opts->format == FMX_COMPACT_INT8;
  const uint32_t P = compact8_row_bytes((uint32_t)k);           // int8: bytes of a feature's block
  uint32_t L = (uint32_t)std::min(h->KP, 64);                   // lanes per feature: a power of two
  if (i8) { L = 2; while (L < 64 && L < P / 4) L <<= 1; }       // (int8: one lane per dword of the block, QUANT8_T dwords at most)
  const uint64_t bytes = i8 ? n * (uint64_t)P : n * (2 * (uint64_t)rs + 4);
  const uint64_t waves = (n + 64 / L - 1) / (64 / L);
  const uint32_t nblk = (uint32_t)std::min<uint64_t>((waves + 3) / 4, COMPACT_BLOCKS);
  // the new snapshot is built beside the old one, which is replaced only when everything has succeeded
  CompactState c;
  c.format = opts->format;
  void* part = nullptr;                                         // [nblk][2] doubles, [nblk] counts, then 2 doubles and 1 count
  // Plain allocations, not the chunked ranges fmx_dev_alloc builds from 768 MiB on.  A snapshot that replaces another takes its memory
  // milliseconds after a range of the same size went back, and physical chunks handed out again that soon have been seen to lose what
  // was just written to them (a 4 GB int8 snapshot taken in turns with a bf16 one read back as zeros).
  hipError_t er = hipSuccess;
  if (i8) { c.P = P; er = fmx_dev_alloc_plain(&c.B, (size_t)n * P); }
  else {
    er = fmx_dev_alloc_plain(&c.V, (size_t)n * rs * sizeof(uint16_t));
    if (er == hipSuccess) er = fmx_dev_alloc_plain(&c.w, (size_t)n * sizeof(float));
  }
  if (er == hipSuccess) er = fmx_dev_alloc(&c.w0, sizeof(double));
  if (er == hipSuccess) er = fmx_dev_alloc(&part, ((size_t)nblk * 3 + 3) * 8);
  struct { double d[2]; unsigned long long c; } res = {{0.0, 0.0}, 0ull};
  if (er == hipSuccess) {
    double* dpart = (double*)part;
    unsigned long long* cpart = (unsigned long long*)part + (size_t)nblk * 2;
    double* dres = (double*)part + (size_t)nblk * 3;
    if (i8) hipLaunchKernelGGL(k_compact_quant8, dim3(nblk), dim3(256), 0, h->stream, (const float*)h->tb.V, (const float*)h->tb.w, rs, n, k, L, P,
                               c.B, dpart, cpart);
    else hipLaunchKernelGGL(k_compact_quant, dim3(nblk), dim3(256), 0, h->stream, (const float*)h->tb.V, rs, n, k, L, c.V, dpart, cpart);
    hipLaunchKernelGGL(k_compact_final, dim3(1), dim3(64), 0, h->stream, (const double*)dpart, (const unsigned long long*)cpart, nblk,
                       dres, (unsigned long long*)(dres + 2));
    er = hipGetLastError();
    if (er == hipSuccess && !i8) er = hipMemcpyAsync(c.w, h->tb.w, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(c.w0, h->w0, sizeof(double), hipMemcpyDeviceToDevice, h->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(&res, dres, sizeof(res), hipMemcpyDeviceToHost, h->stream);
  }
  if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  fmx_dev_free(part);
  if (er != hipSuccess) {
    compact_release(c);
    return fail(h, FMX_E_HIP, "%s: the snapshot (%zu bytes): %s", who, (size_t)bytes, hipGetErrorString(er));
  }
  compact_release(h->compact);
  h->compact = c;
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
    if (h->compact.format == FMX_COMPACT_INT8)
      hipLaunchKernelGGL(k_fetch_rows<RowsI8>, grid, dim3(256), 0, h->stream, d_ids, count, k, make_shard(h->cfg), compact_rows8(h->compact), d_w, d_v);
    else
      hipLaunchKernelGGL(k_fetch_rows<RowsBf16>, grid, dim3(256), 0, h->stream, d_ids, count, k, make_shard(h->cfg), compact_rows(h, h->compact), d_w, d_v);
  });
}

}  // extern "C"
