// fmx_hofm.hip -- the third-order FM's session, scoring and AdaGrad epoch (include/fmx.h "fmx_hofm_*").
// The kernels and their arithmetic are fmx_hofm_kernels.h; the batch flow is stateful_epoch's (fmx_sgd.hip) with k_hofm_rows in place of
// k_rowsums and k_hofm_apply_seg as the owner.  The session owns no parameters: w, V and the accumulators are the handle's tables, and
// the session only says which columns of a row are third-order factors.
#include "fmx_internal.h"
#include "fmx_hofm_kernels.h"

void hofm_free(fmx_handle h) {
  fmx_dev_free(h->hofm.scratch);
  h->hofm = HofmState();
}

// what every fmx_hofm_* entry point refuses whatever the session's state
static int hofm_check_handle(fmx_handle h, const char* who) {
  if (h->cfg.shard_world > 1 || h->comm || (h->group && !h->owns_group))
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", who);
  if (h->cfg.num_factor < 1 || h->cfg.num_factor > 1024)
    return fail(h, FMX_E_UNSUPPORTED, "%s: num_factor %d, 1 .. 1024 (pairwise + third-order factors) are supported", who, h->cfg.num_factor);
  if (h->sgda.reg) return fail(h, FMX_E_STATE, "%s: an SGDA session is open (call fmx_sgda_end first)", who);
  if (h->als.slot >= 0) return fail(h, FMX_E_STATE, "%s: an ALS / MCMC session is open (call fmx_als_end first)", who);
  return FMX_OK;
}
static int hofm_check_session(fmx_handle h, const char* who) {
  int rc = hofm_check_handle(h, who); if (rc) return rc;
  if (!h->hofm.open) return fail(h, FMX_E_STATE, "%s before fmx_hofm_begin", who);
  return FMX_OK;
}
static int hofm_check_rows(fmx_handle h, int slot, const char* who) {
  const Slot& s = h->slots[slot];
  if (!s.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "%s: relations are not supported with the third-order FM", who);
  if (s.weighted) return fail(h, FMX_E_UNSUPPORTED, "%s: slot %d has row weights (fmx_set_row_weights), which the third-order FM does not take", who, slot);
  return FMX_OK;
}

// rest[] of rows [row0, row0 + n); H != nullptr: the training form, which also leaves the batch's H and P rows
static int hofm_launch_rows(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n, float* rest, float* H, float* P, hipStream_t st) {
  const HofmState& hs = h->hofm;
  if (H) { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_hofm_rows<KP, true>), n, st, s.ent, s.row_ptr, row0, n, h->tb, h->cfg.k1, hs.k2, hs.RW, hs.c0, rest, H, P)); }
  else   { KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_hofm_rows<KP, false>), n, st, s.ent, s.row_ptr, row0, n, h->tb, h->cfg.k1, hs.k2, hs.RW, hs.c0, rest,
                                             (float*)nullptr, (float*)nullptr)); }
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// the whole slot's rest pass for predict_out / evaluate_out (RestFn)
static int hofm_rest_pass(fmx_handle h, const Slot& s, float* rest, hipStream_t st) { return hofm_launch_rows(h, s, 0, s.n_rows, rest, nullptr, nullptr, st); }

// One epoch's steps per batch (StatefulSteps, called in this order on one stream): rows fills the session's scratch -- H [rows][RW], then
// P [rows][RW - c0] -- sized for the largest batch seen (the first of an epoch) and kept until _end; owner reads it.  Nothing follows.
static int hofm_step_rows(void* ctx, const Slot& s, uint64_t row0, uint32_t nb, float* rest, hipStream_t st) {
  fmx_handle h = static_cast<fmx_handle>(ctx);
  HofmState& hs = h->hofm;
  if (nb > hs.scratch_rows) {
    HIPCHK(h, hipStreamSynchronize(st));
    fmx_dev_free(hs.scratch); hs.scratch = nullptr; hs.scratch_rows = 0;
    const size_t bytes = (size_t)nb * (2u * hs.RW - hs.c0) * sizeof(float);
    const hipError_t e = fmx_dev_alloc(&hs.scratch, bytes);
    if (e != hipSuccess) return fail(h, FMX_E_HIP, "fmx_hofm_epoch: %zu bytes of scratch for a batch of %u rows: %s", bytes, nb, hipGetErrorString(e));
    hs.scratch_rows = nb;
  }
  return hofm_launch_rows(h, s, row0, nb, rest, hs.scratch, hs.scratch + hs.scratch_rows * hs.RW, st);
}
static int hofm_step_owner(void* ctx, const SegWork& sw, const Hyper& hy, hipStream_t st) {
  fmx_handle h = static_cast<fmx_handle>(ctx);
  const HofmState& hs = h->hofm;
  const AdagradRule rule{{Tab{h->adapt.nv, h->adapt.nw, h->tb.rs, 1u}}, h->adapt.eta};
  const HofmSums sum{hs.scratch, hs.scratch + hs.scratch_rows * hs.RW, hs.k2, hs.c0, hs.RW};
  KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_hofm_apply_seg<KP, HofmOwnerU<KP>::value>), ((uint64_t)sw.nseg + 63) / 64, st, sw, h->tb, rule, hy, sum));
  return FMX_OK;
}

extern "C" {

int fmx_hofm_begin(fmx_handle h, const fmx_hofm_opts* opts) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_hofm_begin"); if (_sr) return _sr; }
  if (!opts) return fail(h, FMX_E_ARG, "fmx_hofm_begin: opts is NULL");
  if (opts->flags != 0) return fail(h, FMX_E_ARG, "fmx_hofm_begin: flags must be 0");
  int rc = hofm_check_handle(h, "fmx_hofm_begin"); if (rc) return rc;
  if (h->fwfm.open) return fail(h, FMX_E_STATE, "fmx_hofm_begin: a field-weighted FM session is open (call fmx_fwfm_end first)");
  if (h->ffm.open) return fail(h, FMX_E_STATE, "fmx_hofm_begin: a field-aware FM session is open (call fmx_ffm_end first)");
  if (h->fmfm.open) return fail(h, FMX_E_STATE, "fmx_hofm_begin: a field-matrixed FM session is open (call fmx_fmfm_end first)");
  if (h->dfm.open) return fail(h, FMX_E_STATE, "fmx_hofm_begin: a DeepFM session is open (call fmx_dfm_end first)");
  if (opts->num_factor3 > (uint32_t)h->cfg.num_factor)
    return fail(h, FMX_E_ARG, "fmx_hofm_begin: num_factor3 %u exceeds num_factor %d: create the handle with num_factor = pairwise + third-order factors",
                opts->num_factor3, h->cfg.num_factor);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  hofm_free(h);
  HofmState& hs = h->hofm;
  hs.k3 = opts->num_factor3; hs.k2 = (uint32_t)h->cfg.num_factor - hs.k3;
  hs.RW = std::min<uint32_t>(h->tb.rs, (uint32_t)h->KP);          // the floats of a row that the owner's lane map covers
  const uint32_t vec = h->KP >= 64 ? (uint32_t)h->KP / 64u : 1u;  // Map<KP>::VEC: the lane map's granularity
  hs.c0 = hs.k2 / vec * vec;                                      // <= k2 <= num_factor <= RW
  hs.open = true;
  return FMX_OK;
}

int fmx_hofm_predict(fmx_handle h, int slot, double* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_hofm_predict"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_hofm_predict: out is NULL");
  int rc = hofm_check_session(h, "fmx_hofm_predict"); if (rc) return rc;
  rc = check_slot(h, slot, false); if (rc) return rc;
  rc = hofm_check_rows(h, slot, "fmx_hofm_predict"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  return predict_out(h, h->slots[slot], nullptr, out, hofm_rest_pass);
}

int fmx_hofm_evaluate(fmx_handle h, int slot, fmx_eval* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_hofm_evaluate"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_hofm_evaluate: out is NULL");
  int rc = hofm_check_session(h, "fmx_hofm_evaluate"); if (rc) return rc;
  rc = check_slot(h, slot, true); if (rc) return rc;
  rc = hofm_check_rows(h, slot, "fmx_hofm_evaluate"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  memset(out, 0, sizeof(*out));
  out->rows = s.n_rows;
  if (s.n_rows == 0) return FMX_OK;
  return evaluate_out(h, s, nullptr, out, hofm_rest_pass);
}

int fmx_hofm_epoch(fmx_handle h, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_hofm_epoch"); if (_sr) return _sr; }
  int rc = hofm_check_session(h, "fmx_hofm_epoch"); if (rc) return rc;
  if (!h->adapt.nv) return fail(h, FMX_E_STATE, "fmx_hofm_epoch needs an open AdaGrad session (fmx_adapt_begin)");
  rc = check_slot(h, slot, true); if (rc) return rc;
  rc = hofm_check_rows(h, slot, "fmx_hofm_epoch"); if (rc) return rc;
  return stateful_epoch_steps(h, slot, batch, w0_chunk, stats, StatefulSteps{h, hofm_step_rows, hofm_step_owner, nullptr});
}

int fmx_hofm_end(fmx_handle h) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_hofm_end"); if (_sr) return _sr; }
  if (!h->hofm.open) return fail(h, FMX_E_STATE, "fmx_hofm_end before fmx_hofm_begin");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  hofm_free(h);
  return FMX_OK;
}

}  // extern "C"
