// fmx_dfm.hip -- DeepFM's session, scoring and AdaGrad epoch (include/fmx.h "fmx_dfm_*").
// The kernels and their arithmetic are fmx_dfm_kernels.h; the batch flow is stateful_epoch's (fmx_sgd.hip) with k_fmfm_sums<KP, true>, k_dfm_gemm_h
// and k_dfm_gemm_z in place of k_rowsums, k_fmfm_apply_seg (unchanged, its sum rows R) as the owner and k_dfm_wgrad / k_dfm_netstep
// behind it.
#include "fmx_internal.h"
#include "fmx_dfm_kernels.h"

void dfm_free(fmx_handle h) {
  DfmState& dm = h->dfm;
  fmx_dev_free(dm.net64); fmx_dev_free(dm.acc64); fmx_dev_free(dm.net32); fmx_dev_free(dm.scratch);
  dm = DfmState();
}

static uint32_t dfm_wp(fmx_handle h) { return (h->num_groups * (uint32_t)h->KP + 15u) / 16u * 16u; }
static size_t dfm_net_count(const DfmState& dm) { return (size_t)dm.F * dm.k * dm.H + 2 * (size_t)dm.H; }

// what every fmx_dfm_* entry point refuses whatever the session's state
static int dfm_check_handle(fmx_handle h, const char* who) {
  if (h->cfg.shard_world > 1 || h->comm || (h->group && !h->owns_group))
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", who);
  if (h->num_groups > FMFM_MAX_FIELDS)
    return fail(h, FMX_E_UNSUPPORTED, "%s: %u fields, at most %u are supported", who, h->num_groups, FMFM_MAX_FIELDS);
  if (h->cfg.num_factor < 1 || h->cfg.num_factor > (int)FMFM_MAX_FACTORS)
    return fail(h, FMX_E_UNSUPPORTED, "%s: num_factor %d, 1 .. %u are supported", who, h->cfg.num_factor, FMFM_MAX_FACTORS);
  if (dfm_wp(h) > FMFM_MAX_WP)
    return fail(h, FMX_E_UNSUPPORTED, "%s: %u fields x %d padded factors are %u columns, at most %u are supported", who, h->num_groups, h->KP,
                dfm_wp(h), FMFM_MAX_WP);
  if (h->sgda.reg) return fail(h, FMX_E_STATE, "%s: an SGDA session is open (call fmx_sgda_end first)", who);
  if (h->als.slot >= 0) return fail(h, FMX_E_STATE, "%s: an ALS / MCMC session is open (call fmx_als_end first)", who);
  return FMX_OK;
}
// ... and every one but _begin: the session, and the field count it was opened with
static int dfm_check_session(fmx_handle h, const char* who) {
  int rc = dfm_check_handle(h, who); if (rc) return rc;
  if (!h->dfm.open) return fail(h, FMX_E_STATE, "%s before fmx_dfm_begin", who);
  if (h->num_groups != h->dfm.F)
    return fail(h, FMX_E_STATE, "%s: the session was opened with %u fields and the handle now has %u (fmx_set_groups): call fmx_dfm_begin again",
                who, h->dfm.F, h->num_groups);
  return FMX_OK;
}
static int dfm_check_rows(fmx_handle h, int slot, const char* who) {
  const Slot& s = h->slots[slot];
  if (!s.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "%s: relations are not supported with DeepFM", who);
  if (s.weighted) return fail(h, FMX_E_UNSUPPORTED, "%s: slot %d has row weights (fmx_set_row_weights), which DeepFM does not take", who, slot);
  return FMX_OK;
}

#define DFM_KP_SWITCH(KPV, ...)                                        \
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

// the fp32 copies inside net32
struct DfmNet32 { const float* W1p; const float* W1t; const float* b1p; const float* w2p; };
static DfmNet32 dfm_net32(const DfmState& dm) {
  const size_t wh = (size_t)dm.WP * dm.HP;
  return DfmNet32{dm.net32, dm.net32 + wh, dm.net32 + 2 * wh, dm.net32 + 2 * wh + dm.HP};
}

// the pointers of a batch's scratch: S [nb][WP], Stot [nb][KP], base [nb]; training only: R [nb][WP], A [nb][HP] and the partials
// P [nsplit][WP + 2][HP].  S, R and A come first: their rows are read as float4s (WP and HP are multiples of 16, the buffer is aligned).
struct DfmScratch { float* S; float* R; float* A; float* Stot; float* base; float* P; uint32_t nsplit; };
static uint32_t dfm_nsplit(size_t nb) { return (uint32_t)std::min<size_t>(FMFM_MSPLIT, (nb + FMFM_MCHUNK - 1) / FMFM_MCHUNK); }
static size_t dfm_scratch_floats(const fmx_handle h, size_t nb, bool train) {
  const DfmState& dm = h->dfm;
  return nb * ((train ? 2 * (size_t)dm.WP + dm.HP : (size_t)dm.WP) + (size_t)h->KP + 1) + (train ? (size_t)dfm_nsplit(nb) * (dm.WP + 2) * dm.HP : 0);
}
static DfmScratch dfm_scratch(const fmx_handle h, size_t nb, bool train) {
  const DfmState& dm = h->dfm;
  float* p = dm.scratch;
  DfmScratch sc{};
  sc.S = p; p += nb * dm.WP;
  if (train) { sc.R = p; p += nb * dm.WP; sc.A = p; p += nb * dm.HP; }
  sc.Stot = p; p += nb * (size_t)h->KP;
  sc.base = p; p += nb;
  if (train) { sc.P = p; sc.nsplit = dfm_nsplit(nb); }
  return sc;
}
// the session's scratch holds a batch of nb rows (kept until fmx_dfm_end; it only grows)
static int dfm_ensure(fmx_handle h, size_t nb, bool train, hipStream_t st, const char* who) {
  DfmState& dm = h->dfm;
  const size_t floats = dfm_scratch_floats(h, nb, train);
  if (floats <= dm.scratch_floats) return FMX_OK;
  HIPCHK(h, hipStreamSynchronize(st));
  fmx_dev_free(dm.scratch); dm.scratch = nullptr; dm.scratch_floats = 0;
  const hipError_t e = fmx_dev_alloc(&dm.scratch, floats * sizeof(float));
  if (e != hipSuccess) return fail(h, FMX_E_HIP, "%s: %zu bytes of scratch for a batch of %zu rows: %s", who, floats * sizeof(float), nb, hipGetErrorString(e));
  dm.scratch_floats = floats;
  return FMX_OK;
}

// S, Stot, base and rest[] of rows [row0, row0 + n) under the session's net; train: A and R too
static int dfm_launch_rows(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n, float* rest, hipStream_t st, const DfmScratch& sc, bool train) {
  const DfmState& dm = h->dfm;
  const DfmNet32 nt = dfm_net32(dm);
  const uint32_t lds = ((dm.F * (uint32_t)h->KP + 3u) & ~3u) * (uint32_t)sizeof(float);
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, 16ull * (uint64_t)h->num_cu));     // one-wavefront workgroups
  DFM_KP_SWITCH(h->KP, hipLaunchKernelGGL((k_fmfm_sums<KP, true>),dim3(grid), dim3(64), lds, st, s.ent, s.row_ptr, row0, n, h->tb, (const uint32_t*)h->grp,
                                          dm.F, dm.WP, h->cfg.k1, sc.S, sc.Stot, sc.base));
  HIPCHK(h, hipGetLastError());
  const uint32_t tiles = (n + FMFM_BM - 1) / FMFM_BM;
  const uint32_t ggrid = std::max<uint32_t>(1, std::min<uint32_t>(tiles, 8u * (uint32_t)h->num_cu));
  if (train) {
    hipLaunchKernelGGL((k_dfm_gemm_h<true>), dim3(ggrid), dim3(256), 0, st, (const float*)sc.S, nt.W1p, nt.b1p, nt.w2p, (const float*)sc.base, n, dm.WP,
                       dm.HP, sc.A, rest);
    hipLaunchKernelGGL(k_dfm_gemm_z, dim3(ggrid), dim3(256), 0, st, (const float*)sc.A, nt.w2p, nt.W1t, (const float*)sc.Stot, n, dm.WP, dm.HP,
                       (uint32_t)h->KP, dm.F * (uint32_t)h->KP, sc.R);
  } else {
    hipLaunchKernelGGL((k_dfm_gemm_h<false>), dim3(ggrid), dim3(256), 0, st, (const float*)sc.S, nt.W1p, nt.b1p, nt.w2p, (const float*)sc.base, n, dm.WP,
                       dm.HP, (float*)nullptr, rest);
  }
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// the whole slot's rest pass for predict_out / evaluate_out (RestFn): in pieces of at most 2^25 / WP rows (S of a piece: 128 MiB), one
// behind the other on the stream through the same scratch
static int dfm_rest_pass(fmx_handle h, const Slot& s, float* rest, hipStream_t st) {
  const uint64_t piece = std::min<uint64_t>(std::max<uint64_t>(1024, (1ull << 25) / h->dfm.WP), std::max<uint64_t>(1, s.n_rows));
  int rc = dfm_ensure(h, piece, false, st, "fmx_dfm_predict / _evaluate"); if (rc) return rc;
  const DfmScratch sc = dfm_scratch(h, piece, false);
  for (uint64_t r0 = 0; r0 < s.n_rows; r0 += piece) {
    rc = dfm_launch_rows(h, s, r0, (uint32_t)std::min<uint64_t>(piece, s.n_rows - r0), rest + r0, st, sc, false);
    if (rc) return rc;
  }
  return FMX_OK;
}

// One epoch's state and its three steps per batch (StatefulSteps, called in this order on one stream).  sc is the CURRENT batch's view of
// the session's scratch: rows sets it, owner and after read it.  The views are laid out from the batch's own nb, and nothing is carried
// from one batch to the next in the buffer.
struct DfmEpoch { fmx_handle h; DfmScratch sc; double eta; };
static int dfm_step_rows(void* ctx, const Slot& s, uint64_t row0, uint32_t nb, float* rest, hipStream_t st) {
  DfmEpoch& ep = *static_cast<DfmEpoch*>(ctx);
  int rc = dfm_ensure(ep.h, nb, true, st, "fmx_dfm_epoch"); if (rc) return rc;
  ep.sc = dfm_scratch(ep.h, nb, true);
  return dfm_launch_rows(ep.h, s, row0, nb, rest, st, ep.sc, true);
}
static int dfm_step_owner(void* ctx, const SegWork& sw, const Hyper& hy, hipStream_t st) {
  const DfmEpoch& ep = *static_cast<DfmEpoch*>(ctx);
  fmx_handle h = ep.h;
  const AdagradRule rule{{Tab{h->adapt.nv, h->adapt.nw, h->tb.rs, 1u}}, h->adapt.eta};
  const FmfmSums sum{ep.sc.R, h->grp, h->dfm.WP};
  DFM_KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_fmfm_apply_seg<KP, AdaptU<KP>::value>), ((uint64_t)sw.nseg + 63) / 64, st, sw, h->tb, rule, hy, sum));
  return FMX_OK;
}
static int dfm_step_after(void* ctx, uint32_t nb, hipStream_t st) {
  const DfmEpoch& ep = *static_cast<DfmEpoch*>(ctx);
  fmx_handle h = ep.h;
  DfmState& dm = h->dfm;
  const DfmScratch& sc = ep.sc;
  const uint32_t nct = (dm.HP + FMFM_BN - 1) / FMFM_BN, nrt = (dm.WP + FMFM_BN - 1) / FMFM_BN;
  hipLaunchKernelGGL(k_dfm_wgrad, dim3(nct, nrt + 2, sc.nsplit), dim3(256), 0, st, (const float*)sc.S, (const float*)sc.A, dfm_net32(dm).w2p,
                     (const float*)h->mult, nb, dm.WP, dm.HP, sc.P);
  hipLaunchKernelGGL(k_dfm_netstep, dim3(((dm.WP + 2) * dm.HP + 255) / 256), dim3(256), 0, st, (const float*)sc.P, sc.nsplit, dm.F, dm.k, (uint32_t)h->KP,
                     dm.WP, dm.H, dm.HP, dm.net64, dm.acc64, dm.net32, ep.eta, dm.reg);
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// the fp32 copies from net64 (after _begin and _set_net)
static int dfm_pad(fmx_handle h) {
  DfmState& dm = h->dfm;
  hipLaunchKernelGGL(k_dfm_pad_net, dim3(((dm.WP + 2) * dm.HP + 255) / 256), dim3(256), 0, h->stream, (const double*)dm.net64, dm.F, dm.k, (uint32_t)h->KP,
                     dm.WP, dm.H, dm.HP, dm.net32);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return FMX_OK;
}

extern "C" {

int fmx_dfm_begin(fmx_handle h, const fmx_dfm_opts* opts) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_dfm_begin"); if (_sr) return _sr; }
  if (!opts) return fail(h, FMX_E_ARG, "fmx_dfm_begin: opts is NULL");
  if (opts->flags != 0) return fail(h, FMX_E_ARG, "fmx_dfm_begin: flags must be 0");
  if (!(opts->learn_rate >= 0.0) || std::isinf(opts->learn_rate)) return fail(h, FMX_E_ARG, "fmx_dfm_begin: learn_rate must be finite and >= 0 (0 = the AdaGrad session's eta)");
  if (!(opts->init_acc >= 0.0) || std::isinf(opts->init_acc)) return fail(h, FMX_E_ARG, "fmx_dfm_begin: init_acc must be finite and >= 0 (0 = 1.0)");
  if (!(opts->reg >= 0.0) || std::isinf(opts->reg)) return fail(h, FMX_E_ARG, "fmx_dfm_begin: reg must be finite and >= 0");
  int rc = dfm_check_handle(h, "fmx_dfm_begin"); if (rc) return rc;
  if (opts->num_hidden < 1 || opts->num_hidden > DFM_MAX_HIDDEN)
    return fail(h, FMX_E_UNSUPPORTED, "fmx_dfm_begin: num_hidden %u, 1 .. %u are supported", opts->num_hidden, DFM_MAX_HIDDEN);
  if (h->fwfm.open) return fail(h, FMX_E_STATE, "fmx_dfm_begin: a field-weighted FM session is open (call fmx_fwfm_end first)");
  if (h->ffm.open) return fail(h, FMX_E_STATE, "fmx_dfm_begin: a field-aware FM session is open (call fmx_ffm_end first)");
  if (h->fmfm.open) return fail(h, FMX_E_STATE, "fmx_dfm_begin: a field-matrixed FM session is open (call fmx_fmfm_end first)");
  if (h->hofm.open) return fail(h, FMX_E_STATE, "fmx_dfm_begin: a third-order FM session is open (call fmx_hofm_end first)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dfm_free(h);
  DfmState& dm = h->dfm;
  dm.F = h->num_groups; dm.k = (uint32_t)h->cfg.num_factor; dm.WP = dfm_wp(h);
  dm.H = opts->num_hidden; dm.HP = (dm.H + 15u) / 16u * 16u;
  dm.eta = opts->learn_rate; dm.reg = opts->reg;
  dm.init_acc = opts->init_acc > 0.0 ? opts->init_acc : 1.0;
  const size_t all = dfm_net_count(dm);
  hipError_t e = fmx_dev_alloc(&dm.net64, all * sizeof(double));
  if (e == hipSuccess) e = fmx_dev_alloc(&dm.acc64, all * sizeof(double));
  if (e == hipSuccess) e = fmx_dev_alloc(&dm.net32, (2 * (size_t)dm.WP * dm.HP + 2 * (size_t)dm.HP) * sizeof(float));
  const std::vector<double> zero(all, 0.0), acc(all, dm.init_acc);
  if (e == hipSuccess) e = hipMemcpy(dm.net64, zero.data(), all * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dm.acc64, acc.data(), all * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) { dfm_free(h); return fail(h, FMX_E_HIP, "fmx_dfm_begin: the net: %s", hipGetErrorString(e)); }
  rc = dfm_pad(h);
  if (rc) { dfm_free(h); return rc; }
  dm.open = true;
  return FMX_OK;
}

int fmx_dfm_set_net(fmx_handle h, const double* W1, const double* b1, const double* w2) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_dfm_set_net"); if (_sr) return _sr; }
  if (!W1 || !b1 || !w2) return fail(h, FMX_E_ARG, "fmx_dfm_set_net: W1, b1 or w2 is NULL");
  int rc = dfm_check_session(h, "fmx_dfm_set_net"); if (rc) return rc;
  const DfmState& dm = h->dfm;
  const size_t nw = (size_t)dm.F * dm.k * dm.H;
  std::vector<double> all(W1, W1 + nw);
  all.insert(all.end(), b1, b1 + dm.H);
  all.insert(all.end(), w2, w2 + dm.H);
  for (size_t i = 0; i < all.size(); i++)
    if (!std::isfinite(all[i])) return fail(h, FMX_E_ARG, "fmx_dfm_set_net: %s[%zu] is not finite", i < nw ? "W1" : i < nw + dm.H ? "b1" : "w2",
                                            i < nw ? i : (i - nw) % dm.H);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(dm.net64, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice));
  return dfm_pad(h);
}

int fmx_dfm_get_net(fmx_handle h, double* W1, double* b1, double* w2, double* n_W1, double* n_b1, double* n_w2) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_dfm_get_net"); if (_sr) return _sr; }
  int rc = dfm_check_session(h, "fmx_dfm_get_net"); if (rc) return rc;
  const DfmState& dm = h->dfm;
  const size_t nw = (size_t)dm.F * dm.k * dm.H;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  double* const out[6] = {W1, b1, w2, n_W1, n_b1, n_w2};
  for (int i = 0; i < 6; i++) {
    const double* src = (i < 3 ? dm.net64 : dm.acc64) + (i % 3 == 0 ? 0 : i % 3 == 1 ? nw : nw + dm.H);
    if (out[i]) HIPCHK(h, hipMemcpy(out[i], src, (i % 3 == 0 ? nw : (size_t)dm.H) * sizeof(double), hipMemcpyDeviceToHost));
  }
  return FMX_OK;
}

int fmx_dfm_predict(fmx_handle h, int slot, double* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_dfm_predict"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_dfm_predict: out is NULL");
  int rc = dfm_check_session(h, "fmx_dfm_predict"); if (rc) return rc;
  rc = check_slot(h, slot, false); if (rc) return rc;
  rc = dfm_check_rows(h, slot, "fmx_dfm_predict"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  return predict_out(h, h->slots[slot], nullptr, out, dfm_rest_pass);
}

int fmx_dfm_evaluate(fmx_handle h, int slot, fmx_eval* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_dfm_evaluate"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_dfm_evaluate: out is NULL");
  int rc = dfm_check_session(h, "fmx_dfm_evaluate"); if (rc) return rc;
  rc = check_slot(h, slot, true); if (rc) return rc;
  rc = dfm_check_rows(h, slot, "fmx_dfm_evaluate"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  memset(out, 0, sizeof(*out));
  out->rows = s.n_rows;
  if (s.n_rows == 0) return FMX_OK;
  return evaluate_out(h, s, nullptr, out, dfm_rest_pass);
}

int fmx_dfm_epoch(fmx_handle h, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_dfm_epoch"); if (_sr) return _sr; }
  int rc = dfm_check_session(h, "fmx_dfm_epoch"); if (rc) return rc;
  if (!h->adapt.nv) return fail(h, FMX_E_STATE, "fmx_dfm_epoch needs an open AdaGrad session (fmx_adapt_begin)");
  rc = check_slot(h, slot, true); if (rc) return rc;
  rc = dfm_check_rows(h, slot, "fmx_dfm_epoch"); if (rc) return rc;
  DfmEpoch ep{h, DfmScratch{}, h->dfm.eta > 0.0 ? h->dfm.eta : (double)h->adapt.eta};
  return stateful_epoch_steps(h, slot, batch, w0_chunk, stats, StatefulSteps{&ep, dfm_step_rows, dfm_step_owner, dfm_step_after});
}

int fmx_dfm_end(fmx_handle h) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_dfm_end"); if (_sr) return _sr; }
  if (!h->dfm.open) return fail(h, FMX_E_STATE, "fmx_dfm_end before fmx_dfm_begin");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dfm_free(h);
  return FMX_OK;
}

}  // extern "C"
