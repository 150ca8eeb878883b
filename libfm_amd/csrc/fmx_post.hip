// fmx_post.hip -- the posterior accumulator of a slot (include/fmx.h "fmx_post_*"): the three prediction
// vectors of fm_learn_mcmc_simultaneous on the device.  The scores come from slot_scores like fmx_evaluate_ex's; one fused pass
// (k_post_accum) adds the draw and carries the reference's metrics of all three vectors; fmx_post_evaluate_ex builds 64-bit keys of
// one vector's means (k_post_key) and hands them and its counts to the finish of fmx_evaluate_ex (eval_ex_finish, fmx_eval.hip).
// The group entry points are in fmx_comm.hip, next to fmx_group_evaluate_ex.
#include "fmx_internal.h"
#include "fmx_post_kernels.h"

#include <limits>

namespace {

struct PostScratch {                         // freed on every path out of the call
  void* part = nullptr;                      // block partials + results
  unsigned long long* keys = nullptr;
  double* tmp = nullptr;
  ~PostScratch() { fmx_dev_free(part); fmx_dev_free(keys); fmx_dev_free(tmp); }
};

const double kNaN = std::numeric_limits<double>::quiet_NaN();

PostArgs post_args(fmx_handle h, const Slot& s, int add_w0) {
  const PostAcc& pa = *s.post;
  PostArgs a;
  a.min_target = h->cfg.min_target; a.max_target = h->cfg.max_target;
  a.r_all = a.r_late = 0.0;
  a.n_rows = s.n_rows;
  a.eval_rows = pa.eval_rows ? pa.eval_rows : s.n_rows;
  a.task = h->cfg.task; a.add_w0 = add_w0; a.k0 = h->cfg.k0;
  a.late = 0;
  return a;
}

void metric_nan(fmx_post_metric* m) {
  m->rows = m->nan_rows = m->correct = 0;
  m->rmse = m->mae = m->accuracy = m->ll_ref = kNaN;
}

}  // namespace

void free_post(Slot& s) {
  if (!s.post) return;
  fmx_dev_free(s.post->sum_all); fmx_dev_free(s.post->sum_late); fmx_dev_free(s.post->last);
  delete s.post;
  s.post = nullptr;
}

// the slot checks of every entry point (fmx_evaluate_ex's) + "fmx_post_begin was called"
int post_check(fmx_handle h, const char* who, int slot, bool need_begin) {
  const int rc = eval_ex_check_slot(h, who, slot);
  if (rc) return rc;
  if (need_begin && !h->slots[slot].post) return fail(h, FMX_E_STATE, "%s: slot %d has no accumulator (call fmx_post_begin first)", who, slot);
  return FMX_OK;
}

int post_begin_impl(fmx_handle h, const char* who, int slot, const fmx_post_opts* opts) {
  fmx_post_opts o = {5u, 0u, 0u, 0u};
  if (opts) o = *opts;
  if (o.flags != 0) return fail(h, FMX_E_ARG, "%s: flags must be 0 (got %u)", who, o.flags);
  int rc = post_check(h, who, slot, false);
  if (rc) return rc;
  Slot& s = h->slots[slot];
  if (o.eval_rows > s.n_rows) return fail(h, FMX_E_ARG, "%s: eval_rows %u > %u rows", who, o.eval_rows, s.n_rows);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  free_post(s);
  PostAcc* pa = new PostAcc();
  s.post = pa;
  const size_t n = std::max<uint32_t>(s.n_rows, 1);
  hipError_t er = fmx_dev_alloc(&pa->sum_all, n * 8);
  if (er == hipSuccess) er = fmx_dev_alloc(&pa->sum_late, n * 8);
  if (er == hipSuccess) er = fmx_dev_alloc(&pa->last, n * 4);
  if (er == hipSuccess) er = hipMemsetAsync(pa->sum_all, 0, n * 8, h->stream);
  if (er == hipSuccess) er = hipMemsetAsync(pa->sum_late, 0, n * 8, h->stream);
  if (er == hipSuccess) er = hipMemsetAsync(pa->last, 0, n * 4, h->stream);
  if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  if (er != hipSuccess) { free_post(s); return fail(h, FMX_E_HIP, "%s: %s", who, hipGetErrorString(er)); }
  pa->burn_in = o.burn_in; pa->eval_rows = o.eval_rows;
  return FMX_OK;
}

// One draw from n = s.n_rows scores that are already on h's device, on h->stream: score[e] is `rest` (add_w0 = 1) or the finished
// y-hat (add_w0 = 0).  The caller has recorded h->ev0 where the call's device work began.  An empty slot counts the draw only.
int post_accum_scores(fmx_handle h, Slot& s, const float* score, int add_w0, fmx_post_stats* out) {
  PostAcc& pa = *s.post;
  const bool late = pa.draws >= pa.burn_in;
  const uint64_t draws = pa.draws + 1, late_draws = pa.late_draws + (late ? 1 : 0);
  fmx_post_stats st;
  memset(&st, 0, sizeof(st));
  st.draws = draws; st.late_draws = late_draws;
  for (auto& m : st.m) metric_nan(&m);
  if (s.n_rows == 0) {
    pa.draws = draws; pa.late_draws = late_draws;
    if (out) *out = st;
    return FMX_OK;
  }
  PostArgs a = post_args(h, s, add_w0);
  a.r_all = 1.0 / (double)draws;
  a.r_late = late_draws ? 1.0 / (double)late_draws : 0.0;
  a.late = late ? 1 : 0;
  const uint32_t nblk = evalx_grid(s.n_rows);
  constexpr int ND = 3 * POST_ND, NC = 3 * POST_NC;
  PostScratch sc;
  // [nblk][ND] doubles, [nblk][NC] counts, then the ND + NC results
  HIPCHK(h, fmx_dev_alloc(&sc.part, ((size_t)nblk + 1) * (ND + NC) * 8));
  double* dpart = (double*)sc.part;
  unsigned long long* cpart = (unsigned long long*)sc.part + (size_t)nblk * ND;
  double* dres = (double*)sc.part + (size_t)nblk * (ND + NC);
  unsigned long long* cres = (unsigned long long*)dres + ND;
  hipLaunchKernelGGL(k_post_accum, dim3(nblk), dim3(256), 0, h->stream, score, (const float*)s.target, a, (const double*)h->w0,
                     pa.sum_all, pa.sum_late, pa.last, dpart, cpart);
  hipLaunchKernelGGL(k_post_final, dim3(1), dim3(64), 0, h->stream, (const double*)dpart, (const unsigned long long*)cpart, nblk, ND, NC, dres, cres);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  struct { double d[ND]; unsigned long long c[NC]; } res;
  HIPCHK(h, hipMemcpyAsync(&res, dres, sizeof(res), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  pa.draws = draws; pa.late_draws = late_draws;                       // (the sums hold the draw from here on)
  const double rows = (double)a.eval_rows;
  for (int q = 0; q < 3; q++) {
    if (q == (int)FMX_POST_LATE && late_draws == 0) continue;
    fmx_post_metric& m = st.m[q];
    m.rows = a.eval_rows; m.nan_rows = res.c[POST_NC * q]; m.correct = res.c[POST_NC * q + 1];
    m.rmse = m.mae = m.accuracy = m.ll_ref = 0.0;
    if (h->cfg.task == FMX_TASK_REGRESSION) {
      m.rmse = std::sqrt(res.d[POST_ND * q] / rows);                  // :287-288
      m.mae = res.d[POST_ND * q + 1] / rows;
    } else {
      m.accuracy = (double)m.correct / rows;                          // :307-308
      m.ll_ref = -res.d[POST_ND * q] / rows;
    }
  }
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  st.device_seconds = ms * 1e-3;
  if (out) *out = st;
  return FMX_OK;
}

int post_evaluate_impl(fmx_handle h, const char* who, int slot, uint32_t which, fmx_eval_ex* out) {
  if (!out) return fail(h, FMX_E_ARG, "%s: out is NULL", who);
  if (which > FMX_POST_LATE) return fail(h, FMX_E_ARG, "%s: which = %u (FMX_POST_THIS, _ALL or _LATE)", who, which);
  int rc = post_check(h, who, slot, true);
  if (rc) return rc;
  const Slot& s = h->slots[slot];
  const PostAcc& pa = *s.post;
  eval_ex_empty(out);
  const uint64_t count = (which == FMX_POST_LATE) ? pa.late_draws : pa.draws;
  if (s.n_rows == 0 || count == 0) return FMX_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const PostArgs a = post_args(h, s, 0);
  const uint32_t n = a.eval_rows;
  const bool cls = (h->cfg.task == FMX_TASK_CLASSIFICATION);
  const uint32_t nblk = evalx_grid(n);
  PostScratch sc;
  // [nblk][3] doubles, [nblk][4] counts, then 3 doubles, 4 counts and the AUC numerator
  HIPCHK(h, fmx_dev_alloc(&sc.part, ((size_t)nblk * 7 + 8) * 8));
  double* dpart = (double*)sc.part;
  unsigned long long* cpart = (unsigned long long*)sc.part + (size_t)nblk * 3;
  double* dres = (double*)sc.part + (size_t)nblk * 7;
  unsigned long long* cres = (unsigned long long*)dres + 3;
  if (cls) HIPCHK(h, fmx_dev_alloc(&sc.keys, (size_t)n * 8));
  const double* src = (which == FMX_POST_ALL) ? pa.sum_all : (which == FMX_POST_LATE) ? pa.sum_late : nullptr;
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  hipLaunchKernelGGL(k_post_key, dim3(nblk), dim3(256), 0, h->stream, src, (const float*)pa.last, 1.0 / (double)count, (const float*)s.target, a,
                     dpart, cpart, sc.keys);
  hipLaunchKernelGGL(k_post_final, dim3(1), dim3(64), 0, h->stream, (const double*)dpart, (const unsigned long long*)cpart, nblk, 3, 4, dres, cres);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemsetAsync(cres + 4, 0, 8, h->stream));
  struct { double d[3]; unsigned long long c[4]; } res;
  HIPCHK(h, hipMemcpyAsync(&res, dres, sizeof(res), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));                        // the counts decide whether anything is sorted
  out->rows = n; out->nan_rows = res.c[1];
  if (cls && res.c[3]) return fail(h, FMX_E_STATE, "%s: %llu means lie below +0 (their bit patterns do not order them)", who, res.c[3]);
  return eval_ex_finish(h, n, res.d, res.c[0], res.c[1], res.c[2], sc.keys, 64, cres + 4, out);
}

int post_get_impl(fmx_handle h, const char* who, int slot, uint32_t which, double* out, uint64_t* draws) {
  if (which > FMX_POST_LATE) return fail(h, FMX_E_ARG, "%s: which = %u (FMX_POST_THIS, _ALL or _LATE)", who, which);
  const int rc = post_check(h, who, slot, true);
  if (rc) return rc;
  const Slot& s = h->slots[slot];
  const PostAcc& pa = *s.post;
  if (draws) *draws = (which == FMX_POST_ALL) ? pa.draws : (which == FMX_POST_LATE) ? pa.late_draws : (pa.draws ? 1 : 0);
  if (!out || s.n_rows == 0) return FMX_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)s.n_rows * 8;
  if (which != FMX_POST_THIS) {
    HIPCHK(h, hipMemcpyAsync(out, which == FMX_POST_ALL ? pa.sum_all : pa.sum_late, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FMX_OK;
  }
  if (pa.draws == 0) { memset(out, 0, bytes); return FMX_OK; }
  PostScratch sc;
  HIPCHK(h, fmx_dev_alloc(&sc.tmp, bytes));
  hipLaunchKernelGGL(k_post_this, dim3(evalx_grid(s.n_rows)), dim3(256), 0, h->stream, (const float*)pa.last, post_args(h, s, 0), sc.tmp);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(out, sc.tmp, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return FMX_OK;
}

int post_end_impl(fmx_handle h, const char* who, int slot) {
  const int rc = post_check(h, who, slot, true);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  free_post(h->slots[slot]);
  return FMX_OK;
}

#define POST_NO_SHARD(h, who)                                                                                            \
  do {                                                                                                                   \
    if (!(h)) return FMX_E_ARG;                                                                                          \
    if ((h)->cfg.shard_world > 1) return fail((h), FMX_E_UNSUPPORTED, "%s on a feature shard: use fmx_group_post_*", who); \
  } while (0)

extern "C" {

int fmx_post_begin(fmx_handle h, int slot, const fmx_post_opts* opts) {
  static const char who[] = "fmx_post_begin";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_post_begin"); if (_sr) return _sr; }
  POST_NO_SHARD(h, who);
  return post_begin_impl(h, who, slot, opts);
}

int fmx_post_accumulate(fmx_handle h, int slot, fmx_post_stats* out) {
  static const char who[] = "fmx_post_accumulate";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_post_accumulate"); if (_sr) return _sr; }
  POST_NO_SHARD(h, who);
  int rc = post_check(h, who, slot, true);
  if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[slot];
  const float* rest = nullptr;
  if (s.n_rows) {
    rc = slot_scores(h, s, nullptr, false, &rest);
    if (rc) return rc;
  }
  return post_accum_scores(h, s, rest, 1, out);
}

int fmx_post_evaluate_ex(fmx_handle h, int slot, uint32_t which, fmx_eval_ex* out) {
  static const char who[] = "fmx_post_evaluate_ex";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_post_evaluate_ex"); if (_sr) return _sr; }
  POST_NO_SHARD(h, who);
  return post_evaluate_impl(h, who, slot, which, out);
}

int fmx_post_get(fmx_handle h, int slot, uint32_t which, double* out, uint64_t* draws) {
  static const char who[] = "fmx_post_get";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_post_get"); if (_sr) return _sr; }
  POST_NO_SHARD(h, who);
  return post_get_impl(h, who, slot, which, out, draws);
}

int fmx_post_end(fmx_handle h, int slot) {
  static const char who[] = "fmx_post_end";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_post_end"); if (_sr) return _sr; }
  POST_NO_SHARD(h, who);
  return post_end_impl(h, who, slot);
}

}  // extern "C"
