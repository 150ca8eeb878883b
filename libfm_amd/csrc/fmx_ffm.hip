// fmx_ffm.hip -- the field-aware FM's session, scoring and AdaGrad epoch (include/fmx.h "fmx_ffm_*").
// The kernels and their arithmetic are fmx_ffm_kernels.h; the batch flow is stateful_epoch's (fmx_sgd.hip) with k_ffm_rows in place of
// k_rowsums and k_ffm_apply_seg as the owner.  The session owns no parameters: w, V and the accumulators are the handle's tables.
#include "fmx_internal.h"
#include "fmx_ffm_kernels.h"

void ffm_free(fmx_handle h) {
  fmx_dev_free(h->ffm.scratch);
  h->ffm = FfmState();
}

// what every fmx_ffm_* entry point refuses whatever the session's state
static int ffm_check_handle(fmx_handle h, const char* who) {
  if (h->cfg.shard_world > 1 || h->comm || (h->group && !h->owns_group))
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", who);
  if (h->num_groups > FFM_MAX_FIELDS)
    return fail(h, FMX_E_UNSUPPORTED, "%s: %u fields, at most %u are supported", who, h->num_groups, FFM_MAX_FIELDS);
  if (h->cfg.num_factor < 1 || h->cfg.num_factor > 1024)
    return fail(h, FMX_E_UNSUPPORTED, "%s: num_factor %d, 1 .. 1024 (fields x latent factors) are supported", who, h->cfg.num_factor);
  if (h->sgda.reg) return fail(h, FMX_E_STATE, "%s: an SGDA session is open (call fmx_sgda_end first)", who);
  if (h->als.slot >= 0) return fail(h, FMX_E_STATE, "%s: an ALS / MCMC session is open (call fmx_als_end first)", who);
  return FMX_OK;
}
// ... and every one but _begin: the session, and the field count it was opened with
static int ffm_check_session(fmx_handle h, const char* who) {
  int rc = ffm_check_handle(h, who); if (rc) return rc;
  if (!h->ffm.open) return fail(h, FMX_E_STATE, "%s before fmx_ffm_begin", who);
  if (h->num_groups != h->ffm.F)
    return fail(h, FMX_E_STATE, "%s: the session was opened with %u fields and the handle now has %u (fmx_set_groups): call fmx_ffm_begin again",
                who, h->ffm.F, h->num_groups);
  return FMX_OK;
}
static int ffm_check_rows(fmx_handle h, int slot, const char* who) {
  const Slot& s = h->slots[slot];
  if (!s.blocks.empty()) return fail(h, FMX_E_UNSUPPORTED, "%s: relations are not supported with the field-aware FM", who);
  if (s.weighted) return fail(h, FMX_E_UNSUPPORTED, "%s: slot %d has row weights (fmx_set_row_weights), which the field-aware FM does not take", who, slot);
  return FMX_OK;
}

// rest[] of rows [row0, row0 + n); Qt != nullptr: the training form, which also leaves the batch's transposed tiles
template <int KP, bool TRAIN>
static int ffm_launch_rows_kp(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n, float* rest, float* Qt, hipStream_t st) {
  const FfmState& fs = h->ffm;
  auto kfn = k_ffm_rows<KP, TRAIN>;
  if (!h->lds_raised.count((const void*)kfn)) {                   // (the limit is per-device state: once per handle and kernel)
    HIPCHK(h, hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fs.lds_max));
    h->lds_raised.insert((const void*)kfn);
  }
  // one-wavefront workgroups: as many as the tiles leave room for on the device at once, never more than the work
  const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>(16, fs.lds_max / fs.lds));
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, per_cu * (uint64_t)h->num_cu));
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(64), fs.lds, st, s.ent, s.row_ptr, row0, n, h->tb, (const uint32_t*)h->grp, fs.F, fs.kf, fs.LD, fs.RW,
                     h->cfg.k1, rest, Qt);
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}
static int ffm_launch_rows(fmx_handle h, const Slot& s, uint64_t row0, uint32_t n, float* rest, float* Qt, hipStream_t st) {
  if (Qt) { KP_SWITCH(h->KP, return (ffm_launch_rows_kp<KP, true>(h, s, row0, n, rest, Qt, st))); }
  else    { KP_SWITCH(h->KP, return (ffm_launch_rows_kp<KP, false>(h, s, row0, n, rest, nullptr, st))); }
  return FMX_OK;
}

// the whole slot's rest pass for predict_out / evaluate_out (RestFn)
static int ffm_rest_pass(fmx_handle h, const Slot& s, float* rest, hipStream_t st) { return ffm_launch_rows(h, s, 0, s.n_rows, rest, nullptr, st); }

// One epoch's steps per batch (StatefulSteps, called in this order on one stream): rows fills the session's scratch Qt [nb][F][RW],
// sized for the largest batch seen (the first of an epoch) and kept until _end; owner reads it.  Nothing follows the owner.
static int ffm_step_rows(void* ctx, const Slot& s, uint64_t row0, uint32_t nb, float* rest, hipStream_t st) {
  fmx_handle h = static_cast<fmx_handle>(ctx);
  FfmState& fs = h->ffm;
  if (nb > fs.scratch_rows) {
    HIPCHK(h, hipStreamSynchronize(st));
    fmx_dev_free(fs.scratch); fs.scratch = nullptr; fs.scratch_rows = 0;
    const size_t bytes = (size_t)nb * fs.F * fs.RW * sizeof(float);
    const hipError_t e = fmx_dev_alloc(&fs.scratch, bytes);
    if (e != hipSuccess) return fail(h, FMX_E_HIP, "fmx_ffm_epoch: %zu bytes of scratch for a batch of %u rows: %s", bytes, nb, hipGetErrorString(e));
    fs.scratch_rows = nb;
  }
  return ffm_launch_rows(h, s, row0, nb, rest, fs.scratch, st);
}
static int ffm_step_owner(void* ctx, const SegWork& sw, const Hyper& hy, hipStream_t st) {
  fmx_handle h = static_cast<fmx_handle>(ctx);
  const FfmState& fs = h->ffm;
  const AdagradRule rule{{Tab{h->adapt.nv, h->adapt.nw, h->tb.rs, 1u}}, h->adapt.eta};
  const FfmSums sum{fs.scratch, h->grp, fs.kf, fs.RW, fs.F * fs.RW};
  KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_ffm_apply_seg<KP, AdaptU<KP>::value>), ((uint64_t)sw.nseg + 63) / 64, st, sw, h->tb, rule, hy, sum));
  return FMX_OK;
}

extern "C" {

int fmx_ffm_begin(fmx_handle h, const fmx_ffm_opts* opts) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_ffm_begin"); if (_sr) return _sr; }
  if (!opts) return fail(h, FMX_E_ARG, "fmx_ffm_begin: opts is NULL");
  if (opts->flags != 0) return fail(h, FMX_E_ARG, "fmx_ffm_begin: flags must be 0");
  int rc = ffm_check_handle(h, "fmx_ffm_begin"); if (rc) return rc;
  if (h->fwfm.open) return fail(h, FMX_E_STATE, "fmx_ffm_begin: a field-weighted FM session is open (call fmx_fwfm_end first)");
  if (h->fmfm.open) return fail(h, FMX_E_STATE, "fmx_ffm_begin: a field-matrixed FM session is open (call fmx_fmfm_end first)");
  if (h->hofm.open) return fail(h, FMX_E_STATE, "fmx_ffm_begin: a third-order FM session is open (call fmx_hofm_end first)");
  if (h->dfm.open) return fail(h, FMX_E_STATE, "fmx_ffm_begin: a DeepFM session is open (call fmx_dfm_end first)");
  const uint32_t F = h->num_groups, kf = opts->num_latent;
  if (kf < 1 || (uint64_t)F * kf != (uint64_t)h->cfg.num_factor)
    return fail(h, FMX_E_ARG, "fmx_ffm_begin: num_factor %d is not %u fields x %u latent factors: create the handle with num_factor = fields x latent",
                h->cfg.num_factor, F, kf);
  const uint32_t LD = ffm_row_stride(F * kf, kf);
  const size_t lds = (size_t)F * LD * sizeof(float);
  const size_t lds_max = std::min<size_t>(FFM_MAX_LDS, h->prop.maxSharedMemoryPerMultiProcessor);
  if (lds > lds_max)
    return fail(h, FMX_E_UNSUPPORTED, "fmx_ffm_begin: the field tile of %u fields x %u floats takes %zu bytes of LDS, at most %zu are supported", F, LD, lds, lds_max);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ffm_free(h);
  FfmState& fs = h->ffm;
  fs.F = F; fs.kf = kf; fs.LD = LD; fs.lds = (uint32_t)lds; fs.lds_max = (uint32_t)lds_max;
  fs.RW = std::min<uint32_t>(h->tb.rs, (uint32_t)h->KP);          // the floats of a row that the owner's lane map covers
  fs.open = true;
  return FMX_OK;
}

int fmx_ffm_predict(fmx_handle h, int slot, double* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_ffm_predict"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_ffm_predict: out is NULL");
  int rc = ffm_check_session(h, "fmx_ffm_predict"); if (rc) return rc;
  rc = check_slot(h, slot, false); if (rc) return rc;
  rc = ffm_check_rows(h, slot, "fmx_ffm_predict"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  return predict_out(h, h->slots[slot], nullptr, out, ffm_rest_pass);
}

int fmx_ffm_evaluate(fmx_handle h, int slot, fmx_eval* out) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_ffm_evaluate"); if (_sr) return _sr; }
  if (!out) return fail(h, FMX_E_ARG, "fmx_ffm_evaluate: out is NULL");
  int rc = ffm_check_session(h, "fmx_ffm_evaluate"); if (rc) return rc;
  rc = check_slot(h, slot, true); if (rc) return rc;
  rc = ffm_check_rows(h, slot, "fmx_ffm_evaluate"); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[slot];
  memset(out, 0, sizeof(*out));
  out->rows = s.n_rows;
  if (s.n_rows == 0) return FMX_OK;
  return evaluate_out(h, s, nullptr, out, ffm_rest_pass);
}

int fmx_ffm_epoch(fmx_handle h, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats* stats) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_ffm_epoch"); if (_sr) return _sr; }
  int rc = ffm_check_session(h, "fmx_ffm_epoch"); if (rc) return rc;
  if (!h->adapt.nv) return fail(h, FMX_E_STATE, "fmx_ffm_epoch needs an open AdaGrad session (fmx_adapt_begin)");
  rc = check_slot(h, slot, true); if (rc) return rc;
  rc = ffm_check_rows(h, slot, "fmx_ffm_epoch"); if (rc) return rc;
  return stateful_epoch_steps(h, slot, batch, w0_chunk, stats, StatefulSteps{h, ffm_step_rows, ffm_step_owner, nullptr});
}

int fmx_ffm_end(fmx_handle h) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_ffm_end"); if (_sr) return _sr; }
  if (!h->ffm.open) return fail(h, FMX_E_STATE, "fmx_ffm_end before fmx_ffm_begin");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ffm_free(h);
  return FMX_OK;
}

}  // extern "C"
