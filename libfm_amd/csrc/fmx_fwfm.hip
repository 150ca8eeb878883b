// fmx_fwfm.hip -- the field-weighted FM's session, scoring and AdaGrad epoch (include/fmx.h "fmx_fwfm_*").
// The kernels and their arithmetic are fmx_fwfm_kernels.h; the batch flow is stateful_epoch's (fmx_sgd.hip) with k_fwfm_rows in place of
// k_rowsums, k_fwfm_apply_seg as the owner and the two r kernels behind it.
#include "fmx_internal.h"
#include "fmx_fwfm_kernels.h"

void fwfm_free(fmx_handle h) {
  FwfmState& fw = h->fwfm;
  fmx_dev_free(fw.r); fmx_dev_free(fw.nr); fmx_dev_free(fw.R32); fmx_dev_free(fw.scratch);
  fw = FwfmState();
}

// what every fmx_fwfm_* entry point refuses whatever the session's state
static int fwfm_check_handle(fmx_handle h, const char* who) {
  if (h->cfg.shard_world > 1 || h->comm || (h->group && !h->owns_group))
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", who);
  if (h->num_groups > FMX_FWFM_MAX_FIELDS)
    return fail(h, FMX_E_UNSUPPORTED, "%s: %u fields, at most %d are supported", who, h->num_groups, FMX_FWFM_MAX_FIELDS);
  if (h->cfg.num_factor < 1 || h->cfg.num_factor > FMX_FWFM_MAX_FACTORS)
    return fail(h, FMX_E_UNSUPPORTED, "%s: num_factor %d, 1 .. %d are supported", who, h->cfg.num_factor, FMX_FWFM_MAX_FACTORS);
  if (h->sgda.reg) return fail(h, FMX_E_STATE, "%s: an SGDA session is open (call fmx_sgda_end first)", who);
  if (h->als.slot >= 0) return fail(h, FMX_E_STATE, "%s: an ALS / MCMC session is open (call fmx_als_end first)", who);
  return FMX_OK;
}
// ... and every one but _begin: the session, and the field count it was opened with
static int fwfm_check_session(fmx_handle h, const char* who) {
  int rc = fwfm_check_handle(h, who); if (rc) return rc;
  if (!h->fwfm.open) return fail(h, FMX_E_STATE, "%s before fmx_fwfm_begin", who);
  if (h->num_groups != h->fwfm.F)
    return fail(h, FMX_E_STATE, "%s: the session was opened with %u fields and the handle now has %u (fmx_set_groups): call fmx_fwfm_begin again",
                who, h->fwfm.F, h->num_groups);
  return FMX_OK;
}
static int fwfm_check_rows(fmx_handle h, int slot, const char* who) {
  const Slot& s = h->slots[slot];
  if (!s.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "%s: relations are not supported with the field-weighted FM", who);
  if (s.weighted) return fail(h, FMX_E_UNSUPPORTED, "%s: slot %d has row weights (fmx_set_row_weights), which the field-weighted FM does not take", who, slot);
  return FMX_OK;
}

// one-wavefront workgroups: as many as the device holds at once (the r fragments are loaded once per wavefront), never more than the work
static uint32_t fwfm_grid(fmx_handle h, const void* kernel, uint64_t want) {
  auto it = h->occ_cache.find(kernel);
  int occ = 0;
  if (it == h->occ_cache.end()) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, 64, 0) != hipSuccess || occ < 1) occ = 4;
    if (occ > 16) occ = 16;
    h->occ_cache[kernel] = occ;
  } else {
    occ = it->second;
  }
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)occ * (uint64_t)h->num_cu));
}

#define FWFM_FT_SWITCH(FTV, ...)                                       \
  switch (FTV) {                                                       \
    case 1: { constexpr int FT = 1; __VA_ARGS__; } break;              \
    case 2: { constexpr int FT = 2; __VA_ARGS__; } break;              \
    case 3: { constexpr int FT = 3; __VA_ARGS__; } break;              \
    default: { constexpr int FT = 4; __VA_ARGS__; } break;             \
  }
#define FWFM_KP_SWITCH(KPV, ...)                                       \
  switch (KPV) {                                                       \
    case 1:   { constexpr int KP = 1;   __VA_ARGS__; } break;          \
    case 2:   { constexpr int KP = 2;   __VA_ARGS__; } break;          \
    case 4:   { constexpr int KP = 4;   __VA_ARGS__; } break;          \
    case 8:   { constexpr int KP = 8;   __VA_ARGS__; } break;          \
    case 16:  { constexpr int KP = 16;  __VA_ARGS__; } break;          \
    case 32:  { constexpr int KP = 32;  __VA_ARGS__; } break;          \
    case 64:  { constexpr int KP = 64;  __VA_ARGS__; } break;          \
    default:  { constexpr int KP = 128; __VA_ARGS__; } break;          \
  }
#define FWFM_LAUNCH_1W(kfn, want, st, ...)                                                          \
  do { auto _k = kfn; hipLaunchKernelGGL(_k, dim3(fwfm_grid(h, (const void*)_k, (want))), dim3(64), 0, st, __VA_ARGS__); } while (0)

// the pointers of a batch's scratch: T and S [nb][FP][KP], D [nb][FP], the r partials P [chunks][FP][FP] and PD [chunks][FP]
struct FwfmScratch { float* T; float* S; float* D; float* P; float* PD; };
static size_t fwfm_scratch_floats(const fmx_handle h, size_t nb) {
  const size_t FP = h->fwfm.FP, nch = (nb + FWFM_RCHUNK - 1) / FWFM_RCHUNK;
  return nb * FP * (2 * (size_t)h->KP + 1) + nch * FP * (FP + 1);
}
static FwfmScratch fwfm_scratch(const fmx_handle h, size_t nb) {
  const size_t FP = h->fwfm.FP, nch = (nb + FWFM_RCHUNK - 1) / FWFM_RCHUNK, tile = nb * FP * (size_t)h->KP;
  float* p = h->fwfm.scratch;
  return FwfmScratch{p, p + tile, p + 2 * tile, p + 2 * tile + nb * FP, p + 2 * tile + nb * FP + nch * FP * FP};
}

// rest[] of rows [row0, row0 + n) under the session's r
static int fwfm_launch_rows(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n, float* rest, hipStream_t st, const FwfmScratch* train) {
  const FwfmState& fw = h->fwfm;
  const uint32_t* grp = h->grp;
  if (train) {
    FWFM_KP_SWITCH(h->KP, FWFM_FT_SWITCH(fw.FP / 16, FWFM_LAUNCH_1W((k_fwfm_rows<KP, FT, true>), n, st, s.ent, s.row_ptr, row0, n, h->tb, grp,
                                                                     (const float*)fw.R32, h->cfg.k1, rest, train->T, train->S, train->D)));
  } else {
    FWFM_KP_SWITCH(h->KP, FWFM_FT_SWITCH(fw.FP / 16, FWFM_LAUNCH_1W((k_fwfm_rows<KP, FT, false>), n, st, s.ent, s.row_ptr, row0, n, h->tb, grp,
                                                                     (const float*)fw.R32, h->cfg.k1, rest, (float*)nullptr, (float*)nullptr, (float*)nullptr)));
  }
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// the whole slot's rest pass for predict_out / evaluate_out (RestFn)
static int fwfm_rest_pass(fmx_handle h, const Slot& s, float* rest, hipStream_t st) { return fwfm_launch_rows(h, s, 0, s.n_rows, rest, st, nullptr); }

// One epoch's state and its three steps per batch (StatefulSteps, called in this order on one stream).  sc is the CURRENT batch's view of
// the session's scratch: rows sets it, owner and after read it.  The buffer is sized for the largest batch seen (the first of an epoch)
// and the views are laid out from the batch's own nb, so the short last batch's P / PD sit at other offsets than the others' -- inside
// the same buffer, and nothing is carried from one batch to the next in it.  FP and KP cannot change under a session: F is checked by
// every entry point (fwfm_check_session) and KP is the handle's.
struct FwfmEpoch { fmx_handle h; FwfmScratch sc; double eta_r; };
static int fwfm_step_rows(void* ctx, const Slot& s, uint64_t row0, uint32_t nb, float* rest, hipStream_t st) {
  FwfmEpoch& ep = *static_cast<FwfmEpoch*>(ctx);
  fmx_handle h = ep.h;
  FwfmState& fw = h->fwfm;
  if (nb > fw.scratch_rows) {
    HIPCHK(h, hipStreamSynchronize(st));
    fmx_dev_free(fw.scratch); fw.scratch = nullptr; fw.scratch_rows = 0;
    const size_t bytes = fwfm_scratch_floats(h, nb) * sizeof(float);
    const hipError_t e = fmx_dev_alloc(&fw.scratch, bytes);
    if (e != hipSuccess) return fail(h, FMX_E_HIP, "fmx_fwfm_epoch: %zu bytes of scratch for a batch of %u rows: %s", bytes, nb, hipGetErrorString(e));
    fw.scratch_rows = nb;
  }
  ep.sc = fwfm_scratch(h, nb);
  return fwfm_launch_rows(h, s, row0, nb, rest, st, &ep.sc);
}
static int fwfm_step_owner(void* ctx, const SegWork& sw, const Hyper& hy, hipStream_t st) {
  const FwfmEpoch& ep = *static_cast<FwfmEpoch*>(ctx);
  fmx_handle h = ep.h;
  const AdagradRule rule{{Tab{h->adapt.nv, h->adapt.nw, h->tb.rs, 1u}}, h->adapt.eta};
  const FwfmSums sum{ep.sc.T, h->grp, h->fwfm.R32, h->fwfm.FP, h->fwfm.FP * (uint32_t)h->KP};
  FWFM_KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_fwfm_apply_seg<KP, AdaptU<KP>::value>), ((uint64_t)sw.nseg + 63) / 64, st, sw, h->tb, rule, hy, sum));
  return FMX_OK;
}
static int fwfm_step_after(void* ctx, uint32_t nb, hipStream_t st) {
  const FwfmEpoch& ep = *static_cast<FwfmEpoch*>(ctx);
  fmx_handle h = ep.h;
  FwfmState& fw = h->fwfm;
  const FwfmScratch& sc = ep.sc;
  const uint32_t nch = (nb + FWFM_RCHUNK - 1) / FWFM_RCHUNK;
  FWFM_KP_SWITCH(h->KP, FWFM_FT_SWITCH(fw.FP / 16, FWFM_LAUNCH_1W((k_fwfm_rgrad<KP, FT>), nch, st, (const float*)sc.S, (const float*)sc.D,
                                                                   (const float*)h->mult, nb, sc.P, sc.PD)));
  hipLaunchKernelGGL(k_fwfm_rstep, dim3((fw.FP * fw.FP + 255) / 256), dim3(256), 0, st, (const float*)sc.P, (const float*)sc.PD, nch, fw.F, fw.FP,
                     fw.r, fw.nr, fw.R32, ep.eta_r, fw.reg_r);
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// r (host, [F][F]) into the session: the fp64 matrix and its padded fp32 copy
static int fwfm_put_r(fmx_handle h, const double* r) {
  FwfmState& fw = h->fwfm;
  HIPCHK(h, hipMemcpyAsync(fw.r, r, (size_t)fw.F * fw.F * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_fwfm_pad_r, dim3((fw.FP * fw.FP + 255) / 256), dim3(256), 0, h->stream, (const double*)fw.r, fw.F, fw.FP, fw.R32);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return FMX_OK;
}

extern "C" {

int fmx_fwfm_begin(fmx_handle h, const fmx_fwfm_opts* opts) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fwfm_begin"); if (_sr) return _sr; }
  if (!opts) return fail(h, FMX_E_ARG, "fmx_fwfm_begin: opts is NULL");
  if (opts->flags != 0) return fail(h, FMX_E_ARG, "fmx_fwfm_begin: flags must be 0");
  if (!(opts->learn_rate_r >= 0.0) || std::isinf(opts->learn_rate_r)) return fail(h, FMX_E_ARG, "fmx_fwfm_begin: learn_rate_r must be finite and >= 0 (0 = the AdaGrad session's eta)");
  if (!(opts->init_acc_r >= 0.0) || std::isinf(opts->init_acc_r)) return fail(h, FMX_E_ARG, "fmx_fwfm_begin: init_acc_r must be finite and >= 0 (0 = 1.0)");
  if (!(opts->reg_r >= 0.0) || std::isinf(opts->reg_r)) return fail(h, FMX_E_ARG, "fmx_fwfm_begin: reg_r must be finite and >= 0");
  int rc = fwfm_check_handle(h, "fmx_fwfm_begin"); if (rc) return rc;
  if (h->ffm.open) return fail(h, FMX_E_STATE, "fmx_fwfm_begin: a field-aware FM session is open (call fmx_ffm_end first)");
  if (h->fmfm.open) return fail(h, FMX_E_STATE, "fmx_fwfm_begin: a field-matrixed FM session is open (call fmx_fmfm_end first)");
  if (h->hofm.open) return fail(h, FMX_E_STATE, "fmx_fwfm_begin: a third-order FM session is open (call fmx_hofm_end first)");
  if (h->dfm.open) return fail(h, FMX_E_STATE, "fmx_fwfm_begin: a DeepFM session is open (call fmx_dfm_end first)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  fwfm_free(h);
  FwfmState& fw = h->fwfm;
  fw.F = h->num_groups; fw.FP = (fw.F + 15u) / 16u * 16u;
  fw.eta_r = opts->learn_rate_r; fw.reg_r = opts->reg_r;
  fw.init_acc = opts->init_acc_r > 0.0 ? opts->init_acc_r : 1.0;
  const size_t ff = (size_t)fw.F * fw.F;
  hipError_t e = fmx_dev_alloc(&fw.r, ff * sizeof(double));
  if (e == hipSuccess) e = fmx_dev_alloc(&fw.nr, ff * sizeof(double));
  if (e == hipSuccess) e = fmx_dev_alloc(&fw.R32, (size_t)fw.FP * fw.FP * sizeof(float));
  const std::vector<double> ones(ff, 1.0), acc(ff, fw.init_acc);
  if (e == hipSuccess) e = hipMemcpy(fw.nr, acc.data(), ff * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) { fwfm_free(h); return fail(h, FMX_E_HIP, "fmx_fwfm_begin: the field matrix: %s", hipGetErrorString(e)); }
  rc = fwfm_put_r(h, ones.data());
  if (rc) { fwfm_free(h); return rc; }
  fw.open = true;
  return FMX_OK;
}

int fmx_fwfm_set_r(fmx_handle h, const double* r) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fwfm_set_r"); if (_sr) return _sr; }
  if (!r) return fail(h, FMX_E_ARG, "fmx_fwfm_set_r: r is NULL");
  int rc = fwfm_check_session(h, "fmx_fwfm_set_r"); if (rc) return rc;
  const uint32_t F = h->fwfm.F;
  for (uint32_t g = 0; g < F; g++)
    for (uint32_t q = 0; q < F; q++) {
      if (!std::isfinite(r[(size_t)g * F + q])) return fail(h, FMX_E_ARG, "fmx_fwfm_set_r: r[%u][%u] is not finite", g, q);
      if (r[(size_t)g * F + q] != r[(size_t)q * F + g]) return fail(h, FMX_E_ARG, "fmx_fwfm_set_r: r[%u][%u] != r[%u][%u]: the matrix must be symmetric", g, q, q, g);
    }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return fwfm_put_r(h, r);
}

int fmx_fwfm_get_r(fmx_handle h, double* r, double* n_r) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fwfm_get_r"); if (_sr) return _sr; }
  if (!r) return fail(h, FMX_E_ARG, "fmx_fwfm_get_r: r is NULL");
  int rc = fwfm_check_session(h, "fmx_fwfm_get_r"); if (rc) return rc;
  const size_t bytes = (size_t)h->fwfm.F * h->fwfm.F * sizeof(double);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(r, h->fwfm.r, bytes, hipMemcpyDeviceToHost));
  if (n_r) HIPCHK(h, hipMemcpy(n_r, h->fwfm.nr, bytes, hipMemcpyDeviceToHost));
  return FMX_OK;
}

int fmx_fwfm_predict(fmx_handle h, int slot, double* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fwfm_predict"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_fwfm_predict: out is NULL");
  int rc = fwfm_check_session(h, "fmx_fwfm_predict"); if (rc) return rc;
  rc = check_slot(h, slot, false); if (rc) return rc;
  rc = fwfm_check_rows(h, slot, "fmx_fwfm_predict"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  return predict_out(h, h->slots[slot], nullptr, out, fwfm_rest_pass);
}

int fmx_fwfm_evaluate(fmx_handle h, int slot, fmx_eval* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fwfm_evaluate"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_fwfm_evaluate: out is NULL");
  int rc = fwfm_check_session(h, "fmx_fwfm_evaluate"); if (rc) return rc;
  rc = check_slot(h, slot, true); if (rc) return rc;
  rc = fwfm_check_rows(h, slot, "fmx_fwfm_evaluate"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  memset(out, 0, sizeof(*out));
  out->rows = s.n_rows;
  if (s.n_rows == 0) return FMX_OK;
  return evaluate_out(h, s, nullptr, out, fwfm_rest_pass);
}

int fmx_fwfm_epoch(fmx_handle h, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fwfm_epoch"); if (_sr) return _sr; }
  int rc = fwfm_check_session(h, "fmx_fwfm_epoch"); if (rc) return rc;
  if (!h->adapt.nv) return fail(h, FMX_E_STATE, "fmx_fwfm_epoch needs an open AdaGrad session (fmx_adapt_begin)");
  rc = check_slot(h, slot, true); if (rc) return rc;
  rc = fwfm_check_rows(h, slot, "fmx_fwfm_epoch"); if (rc) return rc;
  FwfmEpoch ep{h, FwfmScratch{}, h->fwfm.eta_r > 0.0 ? h->fwfm.eta_r : (double)h->adapt.eta};
  return stateful_epoch_steps(h, slot, batch, w0_chunk, stats, StatefulSteps{&ep, fwfm_step_rows, fwfm_step_owner, fwfm_step_after});
}

int fmx_fwfm_end(fmx_handle h) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fwfm_end"); if (_sr) return _sr; }
  if (!h->fwfm.open) return fail(h, FMX_E_STATE, "fmx_fwfm_end before fmx_fwfm_begin");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  fwfm_free(h);
  return FMX_OK;
}

}  // extern "C"
