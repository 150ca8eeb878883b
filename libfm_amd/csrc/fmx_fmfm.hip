// fmx_fmfm.hip -- the field-matrixed FM's session, scoring and AdaGrad epoch (include/fmx.h "fmx_fmfm_*").
// The kernels and their arithmetic are fmx_fmfm_kernels.h; the batch flow is stateful_epoch's (fmx_sgd.hip) with k_fmfm_sums and
// k_fmfm_gemm_t in place of k_rowsums, k_fmfm_apply_seg as the owner and the two M kernels behind it.
#include "fmx_internal.h"
#include "fmx_fmfm_kernels.h"

void fmfm_free(fmx_handle h) {
  FmfmState& fm = h->fmfm;
  fmx_dev_free(fm.m); fmx_dev_free(fm.nm); fmx_dev_free(fm.MM32); fmx_dev_free(fm.scratch);
  fm = FmfmState();
}

static uint32_t fmfm_wp(fmx_handle h) { return (h->num_groups * (uint32_t)h->KP + 15u) / 16u * 16u; }

// what every fmx_fmfm_* entry point refuses whatever the session's state
static int fmfm_check_handle(fmx_handle h, const char* who) {
  if (h->cfg.shard_world > 1 || h->comm || (h->group && !h->owns_group))
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", who);
  if (h->num_groups > FMFM_MAX_FIELDS)
    return fail(h, FMX_E_UNSUPPORTED, "%s: %u fields, at most %u are supported", who, h->num_groups, FMFM_MAX_FIELDS);
  if (h->cfg.num_factor < 1 || h->cfg.num_factor > (int)FMFM_MAX_FACTORS)
    return fail(h, FMX_E_UNSUPPORTED, "%s: num_factor %d, 1 .. %u are supported", who, h->cfg.num_factor, FMFM_MAX_FACTORS);
  if (fmfm_wp(h) > FMFM_MAX_WP)
    return fail(h, FMX_E_UNSUPPORTED, "%s: %u fields x %d padded factors are %u columns, at most %u are supported", who, h->num_groups, h->KP,
                fmfm_wp(h), FMFM_MAX_WP);
  if (h->sgda.reg) return fail(h, FMX_E_STATE, "%s: an SGDA session is open (call fmx_sgda_end first)", who);
  if (h->als.slot >= 0) return fail(h, FMX_E_STATE, "%s: an ALS / MCMC session is open (call fmx_als_end first)", who);
  return FMX_OK;
}
// ... and every one but _begin: the session, and the field count it was opened with
static int fmfm_check_session(fmx_handle h, const char* who) {
  int rc = fmfm_check_handle(h, who); if (rc) return rc;
  if (!h->fmfm.open) return fail(h, FMX_E_STATE, "%s before fmx_fmfm_begin", who);
  if (h->num_groups != h->fmfm.F)
    return fail(h, FMX_E_STATE, "%s: the session was opened with %u fields and the handle now has %u (fmx_set_groups): call fmx_fmfm_begin again",
                who, h->fmfm.F, h->num_groups);
  return FMX_OK;
}
static int fmfm_check_rows(fmx_handle h, int slot, const char* who) {
  const Slot& s = h->slots[slot];
  if (!s.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "%s: relations are not supported with the field-matrixed FM", who);
  if (s.weighted) return fail(h, FMX_E_UNSUPPORTED, "%s: slot %d has row weights (fmx_set_row_weights), which the field-matrixed FM does not take", who, slot);
  return FMX_OK;
}

#define FMFM_KP_SWITCH(KPV, ...)                                       \
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

// the pointers of a batch's scratch: S and T [nb][WP], D and L [nb], the M partials P [nsplit][WP][WP] (training only)
struct FmfmScratch { float* S; float* T; float* D; float* L; float* P; uint32_t nsplit; };
static uint32_t fmfm_nsplit(size_t nb) { return (uint32_t)std::min<size_t>(FMFM_MSPLIT, (nb + FMFM_MCHUNK - 1) / FMFM_MCHUNK); }
static size_t fmfm_scratch_floats(const fmx_handle h, size_t nb, bool train) {
  const size_t WP = h->fmfm.WP;
  return nb * (2 * WP + 2) + (train ? (size_t)fmfm_nsplit(nb) * WP * WP : 0);
}
static FmfmScratch fmfm_scratch(const fmx_handle h, size_t nb) {
  const size_t tile = nb * (size_t)h->fmfm.WP;
  float* p = h->fmfm.scratch;
  return FmfmScratch{p, p + tile, p + 2 * tile, p + 2 * tile + nb, p + 2 * tile + 2 * nb, fmfm_nsplit(nb)};
}
// the session's scratch holds a batch of nb rows (kept until fmx_fmfm_end; it only grows)
static int fmfm_ensure(fmx_handle h, size_t nb, bool train, hipStream_t st, const char* who) {
  FmfmState& fm = h->fmfm;
  const size_t floats = fmfm_scratch_floats(h, nb, train);
  if (floats <= fm.scratch_floats) return FMX_OK;
  HIPCHK(h, hipStreamSynchronize(st));
  fmx_dev_free(fm.scratch); fm.scratch = nullptr; fm.scratch_floats = 0;
  const hipError_t e = fmx_dev_alloc(&fm.scratch, floats * sizeof(float));
  if (e != hipSuccess) return fail(h, FMX_E_HIP, "%s: %zu bytes of scratch for a batch of %zu rows: %s", who, floats * sizeof(float), nb, hipGetErrorString(e));
  fm.scratch_floats = floats;
  return FMX_OK;
}

// S, D, L and rest[] of rows [row0, row0 + n) under the session's M; train: T too
static int fmfm_launch_rows(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n, float* rest, hipStream_t st, const FmfmScratch& sc, bool train) {
  const FmfmState& fm = h->fmfm;
  const uint32_t lds = ((fm.F * (uint32_t)h->KP + 3u) & ~3u) * (uint32_t)sizeof(float);
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, 16ull * (uint64_t)h->num_cu));     // one-wavefront workgroups
  FMFM_KP_SWITCH(h->KP, hipLaunchKernelGGL((k_fmfm_sums<KP>), dim3(grid), dim3(64), lds, st, s.ent, s.row_ptr, row0, n, h->tb, (const uint32_t*)h->grp,
                                           fm.F, fm.WP, h->cfg.k1, sc.S, sc.D, sc.L));
  HIPCHK(h, hipGetLastError());
  const uint32_t tiles = (n + FMFM_BM - 1) / FMFM_BM;
  const uint32_t ggrid = std::max<uint32_t>(1, std::min<uint32_t>(tiles, 8u * (uint32_t)h->num_cu));
  if (train) hipLaunchKernelGGL((k_fmfm_gemm_t<true>), dim3(ggrid), dim3(256), 0, st, (const float*)sc.S, (const float*)fm.MM32, (const float*)sc.D,
                                (const float*)sc.L, n, fm.WP, sc.T, rest);
  else hipLaunchKernelGGL((k_fmfm_gemm_t<false>), dim3(ggrid), dim3(256), 0, st, (const float*)sc.S, (const float*)fm.MM32, (const float*)sc.D,
                          (const float*)sc.L, n, fm.WP, (float*)nullptr, rest);
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// the whole slot's rest pass for predict_out / evaluate_out (RestFn): in pieces of at most 2^25 / WP rows (S of a piece: 128 MiB), one
// behind the other on the stream through the same scratch
static int fmfm_rest_pass(fmx_handle h, const Slot& s, float* rest, hipStream_t st) {
  const uint64_t piece = std::min<uint64_t>(std::max<uint64_t>(1024, (1ull << 25) / h->fmfm.WP), std::max<uint64_t>(1, s.n_rows));
  int rc = fmfm_ensure(h, piece, false, st, "fmx_fmfm_predict / _evaluate"); if (rc) return rc;
  const FmfmScratch sc = fmfm_scratch(h, piece);
  for (uint64_t r0 = 0; r0 < s.n_rows; r0 += piece) {
    rc = fmfm_launch_rows(h, s, r0, (uint32_t)std::min<uint64_t>(piece, s.n_rows - r0), rest + r0, st, sc, false);
    if (rc) return rc;
  }
  return FMX_OK;
}

// One epoch's state and its three steps per batch (StatefulSteps, called in this order on one stream).  sc is the CURRENT batch's view of
// the session's scratch: rows sets it, owner and after read it.  The views are laid out from the batch's own nb, and nothing is carried
// from one batch to the next in the buffer.  WP cannot change under a session: F is checked by every entry point and KP is the handle's.
struct FmfmEpoch { fmx_handle h; FmfmScratch sc; double eta_m; };
static int fmfm_step_rows(void* ctx, const Slot& s, uint64_t row0, uint32_t nb, float* rest, hipStream_t st) {
  FmfmEpoch& ep = *static_cast<FmfmEpoch*>(ctx);
  int rc = fmfm_ensure(ep.h, nb, true, st, "fmx_fmfm_epoch"); if (rc) return rc;
  ep.sc = fmfm_scratch(ep.h, nb);
  return fmfm_launch_rows(ep.h, s, row0, nb, rest, st, ep.sc, true);
}
static int fmfm_step_owner(void* ctx, const SegWork& sw, const Hyper& hy, hipStream_t st) {
  const FmfmEpoch& ep = *static_cast<FmfmEpoch*>(ctx);
  fmx_handle h = ep.h;
  const AdagradRule rule{{Tab{h->adapt.nv, h->adapt.nw, h->tb.rs, 1u}}, h->adapt.eta};
  const FmfmSums sum{ep.sc.T, h->grp, h->fmfm.WP};
  FMFM_KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_fmfm_apply_seg<KP, AdaptU<KP>::value>), ((uint64_t)sw.nseg + 63) / 64, st, sw, h->tb, rule, hy, sum));
  return FMX_OK;
}
static int fmfm_step_after(void* ctx, uint32_t nb, hipStream_t st) {
  const FmfmEpoch& ep = *static_cast<FmfmEpoch*>(ctx);
  fmx_handle h = ep.h;
  FmfmState& fm = h->fmfm;
  const FmfmScratch& sc = ep.sc;
  if (fm.F < 2) return FMX_OK;                                      // no block g < h: nothing is learned beside w and V
  const uint32_t nct = (fm.WP + FMFM_BN - 1) / FMFM_BN;
  hipLaunchKernelGGL(k_fmfm_mgrad, dim3(nct, nct, sc.nsplit), dim3(256), 0, st, (const float*)sc.S, (const float*)h->mult, nb, fm.WP, (uint32_t)h->KP,
                     fm.F, sc.P);
  hipLaunchKernelGGL(k_fmfm_mstep, dim3((fm.WP * fm.WP + 255) / 256), dim3(256), 0, st, (const float*)sc.P, sc.nsplit, fm.F, fm.k, (uint32_t)h->KP,
                     fm.WP, fm.m, fm.nm, fm.MM32, ep.eta_m, fm.reg_m);
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// M (host, [F][F][k][k]) into the session: the fp64 blocks and their padded fp32 copy
static int fmfm_put_m(fmx_handle h, const double* m) {
  FmfmState& fm = h->fmfm;
  HIPCHK(h, hipMemcpyAsync(fm.m, m, (size_t)fm.F * fm.F * fm.k * fm.k * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_fmfm_pad_m, dim3((fm.WP * fm.WP + 255) / 256), dim3(256), 0, h->stream, (const double*)fm.m, fm.F, fm.k, (uint32_t)h->KP, fm.WP, fm.MM32);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return FMX_OK;
}

extern "C" {

int fmx_fmfm_begin(fmx_handle h, const fmx_fmfm_opts* opts) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fmfm_begin"); if (_sr) return _sr; }
  if (!opts) return fail(h, FMX_E_ARG, "fmx_fmfm_begin: opts is NULL");
  if (opts->flags != 0) return fail(h, FMX_E_ARG, "fmx_fmfm_begin: flags must be 0");
  if (!(opts->learn_rate_m >= 0.0) || std::isinf(opts->learn_rate_m)) return fail(h, FMX_E_ARG, "fmx_fmfm_begin: learn_rate_m must be finite and >= 0 (0 = the AdaGrad session's eta)");
  if (!(opts->init_acc_m >= 0.0) || std::isinf(opts->init_acc_m)) return fail(h, FMX_E_ARG, "fmx_fmfm_begin: init_acc_m must be finite and >= 0 (0 = 1.0)");
  if (!(opts->reg_m >= 0.0) || std::isinf(opts->reg_m)) return fail(h, FMX_E_ARG, "fmx_fmfm_begin: reg_m must be finite and >= 0");
  int rc = fmfm_check_handle(h, "fmx_fmfm_begin"); if (rc) return rc;
  if (h->fwfm.open) return fail(h, FMX_E_STATE, "fmx_fmfm_begin: a field-weighted FM session is open (call fmx_fwfm_end first)");
  if (h->ffm.open) return fail(h, FMX_E_STATE, "fmx_fmfm_begin: a field-aware FM session is open (call fmx_ffm_end first)");
  if (h->hofm.open) return fail(h, FMX_E_STATE, "fmx_fmfm_begin: a third-order FM session is open (call fmx_hofm_end first)");
  if (h->dfm.open) return fail(h, FMX_E_STATE, "fmx_fmfm_begin: a DeepFM session is open (call fmx_dfm_end first)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  fmfm_free(h);
  FmfmState& fm = h->fmfm;
  fm.F = h->num_groups; fm.k = (uint32_t)h->cfg.num_factor; fm.WP = fmfm_wp(h);
  fm.eta_m = opts->learn_rate_m; fm.reg_m = opts->reg_m;
  fm.init_acc = opts->init_acc_m > 0.0 ? opts->init_acc_m : 1.0;
  const size_t kk = (size_t)fm.k * fm.k, all = (size_t)fm.F * fm.F * kk;
  hipError_t e = fmx_dev_alloc(&fm.m, all * sizeof(double));
  if (e == hipSuccess) e = fmx_dev_alloc(&fm.nm, all * sizeof(double));
  if (e == hipSuccess) e = fmx_dev_alloc(&fm.MM32, (size_t)fm.WP * fm.WP * sizeof(float));
  std::vector<double> eye(all, 0.0);
  const std::vector<double> acc(all, fm.init_acc);
  for (size_t blk = 0; blk < (size_t)fm.F * fm.F; blk++)
    for (uint32_t a = 0; a < fm.k; a++) eye[blk * kk + (size_t)a * fm.k + a] = 1.0;
  if (e == hipSuccess) e = hipMemcpy(fm.nm, acc.data(), all * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) { fmfm_free(h); return fail(h, FMX_E_HIP, "fmx_fmfm_begin: the field matrices: %s", hipGetErrorString(e)); }
  rc = fmfm_put_m(h, eye.data());
  if (rc) { fmfm_free(h); return rc; }
  fm.open = true;
  return FMX_OK;
}

int fmx_fmfm_set_m(fmx_handle h, const double* m) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fmfm_set_m"); if (_sr) return _sr; }
  if (!m) return fail(h, FMX_E_ARG, "fmx_fmfm_set_m: m is NULL");
  int rc = fmfm_check_session(h, "fmx_fmfm_set_m"); if (rc) return rc;
  const size_t F = h->fmfm.F, k = h->fmfm.k;
  for (size_t g = 0; g < F; g++)
    for (size_t q = 0; q < F; q++)
      for (size_t a = 0; a < k; a++)
        for (size_t b = 0; b < k; b++) {
          const double v = m[((g * F + q) * k + a) * k + b];
          if (!std::isfinite(v)) return fail(h, FMX_E_ARG, "fmx_fmfm_set_m: m[%zu][%zu][%zu][%zu] is not finite", g, q, a, b);
          if (g == q && v != (a == b ? 1.0 : 0.0))
            return fail(h, FMX_E_ARG, "fmx_fmfm_set_m: m[%zu][%zu] is not the identity: the diagonal blocks are not learned", g, g);
          if (v != m[((q * F + g) * k + b) * k + a])
            return fail(h, FMX_E_ARG, "fmx_fmfm_set_m: m[%zu][%zu] is not the transpose of m[%zu][%zu]", q, g, g, q);
        }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return fmfm_put_m(h, m);
}

int fmx_fmfm_get_m(fmx_handle h, double* m, double* n_m) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fmfm_get_m"); if (_sr) return _sr; }
  if (!m) return fail(h, FMX_E_ARG, "fmx_fmfm_get_m: m is NULL");
  int rc = fmfm_check_session(h, "fmx_fmfm_get_m"); if (rc) return rc;
  const size_t bytes = (size_t)h->fmfm.F * h->fmfm.F * h->fmfm.k * h->fmfm.k * sizeof(double);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(m, h->fmfm.m, bytes, hipMemcpyDeviceToHost));
  if (n_m) HIPCHK(h, hipMemcpy(n_m, h->fmfm.nm, bytes, hipMemcpyDeviceToHost));
  return FMX_OK;
}

int fmx_fmfm_predict(fmx_handle h, int slot, double* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fmfm_predict"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_fmfm_predict: out is NULL");
  int rc = fmfm_check_session(h, "fmx_fmfm_predict"); if (rc) return rc;
  rc = check_slot(h, slot, false); if (rc) return rc;
  rc = fmfm_check_rows(h, slot, "fmx_fmfm_predict"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  return predict_out(h, h->slots[slot], nullptr, out, fmfm_rest_pass);
}

int fmx_fmfm_evaluate(fmx_handle h, int slot, fmx_eval* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fmfm_evaluate"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_fmfm_evaluate: out is NULL");
  int rc = fmfm_check_session(h, "fmx_fmfm_evaluate"); if (rc) return rc;
  rc = check_slot(h, slot, true); if (rc) return rc;
  rc = fmfm_check_rows(h, slot, "fmx_fmfm_evaluate"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  memset(out, 0, sizeof(*out));
  out->rows = s.n_rows;
  if (s.n_rows == 0) return FMX_OK;
  return evaluate_out(h, s, nullptr, out, fmfm_rest_pass);
}

int fmx_fmfm_epoch(fmx_handle h, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fmfm_epoch"); if (_sr) return _sr; }
  int rc = fmfm_check_session(h, "fmx_fmfm_epoch"); if (rc) return rc;
  if (!h->adapt.nv) return fail(h, FMX_E_STATE, "fmx_fmfm_epoch needs an open AdaGrad session (fmx_adapt_begin)");
  rc = check_slot(h, slot, true); if (rc) return rc;
  rc = fmfm_check_rows(h, slot, "fmx_fmfm_epoch"); if (rc) return rc;
  FmfmEpoch ep{h, FmfmScratch{}, h->fmfm.eta_m > 0.0 ? h->fmfm.eta_m : (double)h->adapt.eta};
  return stateful_epoch_steps(h, slot, batch, w0_chunk, stats, StatefulSteps{&ep, fmfm_step_rows, fmfm_step_owner, fmfm_step_after});
}

int fmx_fmfm_end(fmx_handle h) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_fmfm_end"); if (_sr) return _sr; }
  if (!h->fmfm.open) return fail(h, FMX_E_STATE, "fmx_fmfm_end before fmx_fmfm_begin");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  fmfm_free(h);
  return FMX_OK;
}

}  // extern "C"
