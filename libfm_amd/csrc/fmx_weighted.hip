// fmx_weighted.hip -- per-row weights of a slot (include/fmx.h "fmx_set_row_weights"): fmx_set_row_weights /
// fmx_get_row_weights, the refusal every trainer without a weighted form gives a weighted slot, and fmx_evaluate_weighted: one scoring
// pass like fmx_evaluate_ex's (slot_scores, its option and slot checks), then the weighted sums as block partials summed in a fixed
// order (fmx_evalw_kernels.h).  The weighted epochs themselves are stateful_epoch's (fmx_sgd.hip, k_scan_weighted).
#include "fmx_internal.h"
#include "fmx_evalw_kernels.h"

#include <cmath>
#include <limits>

int refuse_weighted(fmx_handle h, int slot, const char* who) {
  if (!h || slot < 0 || slot >= FMX_MAX_SLOTS || !h->slots[slot].weighted) return FMX_OK;
  return fail(h, FMX_E_UNSUPPORTED, "%s: slot %d has row weights (fmx_set_row_weights) and this trainer has no weighted form: "
              "train it with fmx_adapt_epoch / fmx_ftrl_epoch, or drop the weights with fmx_set_row_weights(h, slot, NULL)", who, slot);
}

static void evalw_empty(fmx_eval_weighted* out) {
  memset(out, 0, sizeof(*out));
  out->logloss = out->rmse = out->mae = out->accuracy = std::numeric_limits<double>::quiet_NaN();
}

extern "C" {

int fmx_set_row_weights(fmx_handle h, int slot, const float* weight) {
  static const char who[] = "fmx_set_row_weights";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_set_row_weights"); if (_sr) return _sr; }
  if (slot < 0 || slot >= FMX_MAX_SLOTS) return fail(h, FMX_E_ARG, "%s: slot %d out of range", who, slot);
  if (h->cfg.shard_world > 1 || h->comm || (h->group && !h->owns_group))
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", who);
  Slot& s = h->slots[slot];
  if (!s.used) return fail(h, FMX_E_STATE, "%s: slot %d holds no rows (call fmx_upload_rows first)", who, slot);
  HIPCHK(h, hipSetDevice(h->device));
  if (!weight) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    fmx_dev_free(s.weight);
    s.weight = nullptr; s.weighted = false;
    return FMX_OK;
  }
  for (uint32_t r = 0; r < s.n_rows; r++)
    if (!(weight[r] >= 0.f) || std::isinf(weight[r]))                 // (NaN fails the comparison)
      return fail(h, FMX_E_ARG, "%s: row %u has weight %g: every weight must be finite and >= 0", who, r, (double)weight[r]);
  float* d = nullptr;
  if (s.n_rows) {
    HIPCHK(h, fmx_dev_alloc(&d, (size_t)s.n_rows * 4));
    const hipError_t er = hipMemcpy(d, weight, (size_t)s.n_rows * 4, hipMemcpyHostToDevice);
    if (er != hipSuccess) { fmx_dev_free(d); return fail(h, FMX_E_HIP, "%s: %s", who, hipGetErrorString(er)); }
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  fmx_dev_free(s.weight);
  s.weight = d; s.weighted = true;
  return FMX_OK;
}

int fmx_get_row_weights(fmx_handle h, int slot, float* out) {
  static const char who[] = "fmx_get_row_weights";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_get_row_weights"); if (_sr) return _sr; }
  if (slot < 0 || slot >= FMX_MAX_SLOTS) return fail(h, FMX_E_ARG, "%s: slot %d out of range", who, slot);
  const Slot& s = h->slots[slot];
  if (!s.used) return fail(h, FMX_E_STATE, "%s: slot %d holds no rows (call fmx_upload_rows first)", who, slot);
  if (!s.weighted) return fail(h, FMX_E_STATE, "%s: slot %d has no row weights (call fmx_set_row_weights first)", who, slot);
  if (s.n_rows == 0) return FMX_OK;
  if (!out) return fail(h, FMX_E_ARG, "%s: out is NULL", who);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(out, s.weight, (size_t)s.n_rows * 4, hipMemcpyDeviceToHost));
  return FMX_OK;
}

int fmx_evaluate_weighted(fmx_handle h, int slot, const fmx_eval_opts* opts, fmx_eval_weighted* out) {
  static const char who[] = "fmx_evaluate_weighted";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_evaluate_weighted"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "%s: out is NULL", who);
  uint32_t link;
  int rc = eval_ex_check_opts(h, who, opts, &link);
  if (rc) return rc;
  rc = eval_ex_check_slot(h, who, slot);
  if (rc) return rc;
  if (h->cfg.shard_world > 1) return fail(h, FMX_E_UNSUPPORTED, "%s on a feature shard: weights live on unsharded handles only", who);
  const Slot& s = h->slots[slot];
  if (!s.weighted) return fail(h, FMX_E_STATE, "%s: slot %d has no row weights (call fmx_set_row_weights first)", who, slot);
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  evalw_empty(out);
  if (s.n_rows == 0) return FMX_OK;
  const float* rest;
  rc = slot_scores(h, s, nullptr, false, &rest);
  if (rc) return rc;
  const uint32_t n = s.n_rows;
  const bool cls = (h->cfg.task == FMX_TASK_CLASSIFICATION);
  const uint32_t nblk = evalx_grid(n);
  EvalScratch sc;
  // [nblk][EVALW_SUMS] doubles, [nblk] counts, then EVALW_SUMS doubles and 1 count
  HIPCHK(h, fmx_dev_alloc(&sc.part, ((size_t)nblk * (EVALW_SUMS + 1) + EVALW_SUMS + 1) * 8));
  double* dpart = (double*)sc.part;
  unsigned long long* cpart = (unsigned long long*)sc.part + (size_t)nblk * EVALW_SUMS;
  double* dres = (double*)sc.part + (size_t)nblk * (EVALW_SUMS + 1);
  unsigned long long* cres = (unsigned long long*)(dres + EVALW_SUMS);
  hipLaunchKernelGGL(k_evalw_score, dim3(nblk), dim3(256), 0, h->stream, rest, (const float*)s.target, (const float*)s.weight, n,
                     make_hyper(h->cfg), (const double*)h->w0, link, dpart, cpart);
  hipLaunchKernelGGL(k_evalw_final, dim3(1), dim3(64), 0, h->stream, (const double*)dpart, (const unsigned long long*)cpart, nblk, dres, cres);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  struct { double d[EVALW_SUMS]; unsigned long long c; } res;
  HIPCHK(h, hipMemcpyAsync(&res, dres, sizeof(res), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  out->rows = n; out->nan_rows = res.c;
  out->weight_sum = res.d[0]; out->pos_weight = res.d[1]; out->neg_weight = res.d[2]; out->correct_weight = res.d[3];
  out->loss_sum = res.d[4]; out->sq_sum = res.d[5]; out->abs_sum = res.d[6];
  out->device_seconds = ms * 1e-3;
  if (out->weight_sum > 0.0 && out->nan_rows == 0) {
    if (cls) {
      out->logloss = out->loss_sum / out->weight_sum;
      out->accuracy = out->correct_weight / out->weight_sum;
    } else {
      out->rmse = std::sqrt(out->sq_sum / out->weight_sum);          // fm_learn.h:152 with the weights
      out->mae = out->abs_sum / out->weight_sum;                      // fm_learn.h:148
    }
  }
  return FMX_OK;
}

}  // extern "C"
