// fmx_post_kernels.h -- kernels of the per-slot posterior accumulator (fmx_post.hip; include/fmx.h "fmx_post_*"):
// the three prediction vectors of fm_learn_mcmc_simultaneous (pred_this, pred_sum_all, pred_sum_all_but5) kept on the device.
//
// k_post_accum   grid-stride over the rows: adds the new draw to the two fp64 sums, keeps the fp32 draw, and carries the block
//                partials of the reference's metrics (_evaluate / _evaluate_class) of all three vectors.
// k_post_key     the same row walk without writing: the means of ONE of the three vectors, their loss / count partials and one
//                64-bit sort key per row for the rank pipeline of fmx_evaluate_ex (fmx_eval.hip: eval_ex_rank).
// k_post_final   one wavefront sums the block partials in a fixed order (k_evalx_final for any number of columns).
// k_post_this    the fp64 image of the fp32 last draw (fmx_post_get of FMX_POST_THIS).
//
// The grids are evalx_grid(n_rows); every fp64 sum runs lane -> wavefront (xor butterfly) -> block (wave order) -> blocks
// (k_post_final), as in fmx_eval_kernels.h: two identical call sequences are bit-identical.  No float atomics, no workgroup waits
// for another, no LDS beyond the block reduction.
#pragma once
#include "fmx_eval_kernels.h"
#include "fmx_als_kernels.h"

namespace fmx {

struct PostArgs {
  double   min_target, max_target;  // the config's doubles (fm_learn_mcmc_simultaneous.h:132-133)
  double   r_all, r_late;           // 1.0 / draws and 1.0 / late_draws AFTER this draw (:216-217: a product, not a division)
  uint32_t n_rows, eval_rows;       // the metrics cover the rows [0, eval_rows)
  int      task, add_w0, k0;
  int      late;                    // this draw counts into the late sum (draws before it >= burn_in)
};

constexpr int POST_ND = 2;          // fp64 partials per vector: {sum err^2, sum |err|} (regression) or {sum ll term, unused}
constexpr int POST_NC = 2;          // counts per vector: {NaN means, correct}

// min / max that let a NaN through (what numpy's minimum / maximum do; fmin / fmax would return the bound)
__device__ __forceinline__ double post_clamp(double p, double lo, double hi) { return (p != p) ? p : fmax(lo, fmin(hi, p)); }

// what a draw adds to the sums (v) and what FMX_POST_THIS is (t), from the fp32 raw y-hat
__device__ __forceinline__ void post_draw(float p, const PostArgs& a, double& t, double& v) {
  if (a.task == 0) { t = (double)p; v = post_clamp(t, a.min_target, a.max_target); }
  else { t = v = ref_cdf_gaussian((double)p); }
}

// one row of _evaluate (:272-289) / _evaluate_class (:291-309) for the mean m
__device__ __forceinline__ void post_metric_row(double m, float y, const PostArgs& a, double& d0, double& d1,
                                                unsigned long long& n_nan, unsigned long long& n_ok) {
  n_nan += (m != m) ? 1u : 0u;
  if (a.task == 0) {
    const double err = post_clamp(m, a.min_target, a.max_target) - (double)y;
    d0 += err * err; d1 += fabs(err);
  } else {
    n_ok += ((m >= 0.5 && y > 0.f) || (m < 0.5 && y < 0.f)) ? 1u : 0u;
    const double w = ((double)y + 1.0) * 0.5;
    double pll = m;
    if (pll > 0.99) pll = 0.99;
    if (pll < 0.01) pll = 0.01;
    d0 += w * log10(pll) + (1.0 - w) * log10(1.0 - pll);               // (ll_ref is minus this sum over the rows)
  }
}

// block reduction of ND fp64 and NC integer accumulators into dpart[ND * block + q] / cpart[NC * block + q]
template <int ND, int NC>
__device__ __forceinline__ void post_block_reduce(double (&d)[ND], unsigned long long (&c)[NC], double* __restrict__ dpart,
                                                  unsigned long long* __restrict__ cpart) {
  __shared__ double dred[ND][4];
  __shared__ unsigned long long cred[NC][4];
  const uint32_t w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < ND; q++) { const double s = wave_sum_d(d[q]); if ((threadIdx.x & 63u) == 0) dred[q][w] = s; }
#pragma unroll
  for (int q = 0; q < NC; q++) { const unsigned long long s = wave_sum_u64(c[q]); if ((threadIdx.x & 63u) == 0) cred[q][w] = s; }
  __syncthreads();
  if (threadIdx.x < ND) {
    double s = 0;
    for (int i = 0; i < 4; i++) s += dred[threadIdx.x][i];
    dpart[ND * blockIdx.x + threadIdx.x] = s;
  }
  if (threadIdx.x < NC) {
    unsigned long long s = 0;
    for (int i = 0; i < 4; i++) s += cred[threadIdx.x][i];
    cpart[NC * blockIdx.x + threadIdx.x] = s;
  }
}

// score[e] is `rest` (add_w0 = 1) or the finished y-hat (add_w0 = 0: the group path).  Partials of block b:
// dpart[6 * b + 2 * which + {0, 1}], cpart[6 * b + 2 * which + {0: NaN means, 1: correct}].  Before the first late draw the late sum is
// neither read nor written and its partials stay 0.
static __global__ void __launch_bounds__(256)
k_post_accum(const float* __restrict__ score, const float* __restrict__ target, PostArgs a, const double* __restrict__ w0_ptr,
             double* __restrict__ sum_all, double* __restrict__ sum_late, float* __restrict__ last,
             double* __restrict__ dpart, unsigned long long* __restrict__ cpart) {
  const float w0 = (a.add_w0 && a.k0) ? (float)(*w0_ptr) : 0.f;
  double d[3 * POST_ND] = {0, 0, 0, 0, 0, 0};
  unsigned long long c[3 * POST_NC] = {0, 0, 0, 0, 0, 0};
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < a.n_rows; e += gridDim.x * blockDim.x) {
    const float p = a.add_w0 ? w0 + score[e] : score[e];               // (exactly k_yhat / k_eval: what fmx_predict returns)
    double t, v;
    post_draw(p, a, t, v);
    const double sa = sum_all[e] + v;
    sum_all[e] = sa;
    double sl = 0;
    if (a.late) { sl = sum_late[e] + v; sum_late[e] = sl; }
    last[e] = p;
    if (e < a.eval_rows) {
      const float y = target[e];
      post_metric_row(t, y, a, d[0], d[1], c[0], c[1]);
      post_metric_row(sa * a.r_all, y, a, d[2], d[3], c[2], c[3]);
      if (a.late) post_metric_row(sl * a.r_late, y, a, d[4], d[5], c[4], c[5]);
    }
  }
  post_block_reduce<3 * POST_ND, 3 * POST_NC>(d, c, dpart, cpart);
}

// The means of one vector over the rows [0, a.eval_rows): src64 (a sum, times r) or, when it is nullptr, the fp32 last draw.
// Partials of block b: dpart[3 * b + {0: sum err^2, 1: sum |err|, 2: sum of -ln(mean or 1 - mean)}],
// cpart[4 * b + {0: pos, 1: NaN means, 2: correct, 3: means below +0}]; keys (classification only): (bits(mean) << 1) | label -- the
// means are sums of values in [0, 1] started from +0, so their bit pattern orders them and fits 63 bits; cpart[.. + 3] counts the
// rows where that fails (the caller refuses instead of sorting them).
static __global__ void __launch_bounds__(256)
k_post_key(const double* __restrict__ src64, const float* __restrict__ last, double r, const float* __restrict__ target, PostArgs a,
           double* __restrict__ dpart, unsigned long long* __restrict__ cpart, unsigned long long* __restrict__ keys) {
  double d[3] = {0, 0, 0};
  unsigned long long c[4] = {0, 0, 0, 0};
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < a.eval_rows; e += gridDim.x * blockDim.x) {
    double m;
    if (src64) m = src64[e] * r;
    else { double v; post_draw(last[e], a, m, v); }
    const float y = target[e];
    c[1] += (m != m) ? 1u : 0u;
    if (a.task == 0) {
      const double err = post_clamp(m, a.min_target, a.max_target) - (double)y;
      d[0] += err * err; d[1] += fabs(err);
    } else {
      const bool pos = (y >= 0);                                       // fm_learn.h:118
      c[0] += pos ? 1u : 0u;
      c[2] += ((m >= 0.5 && y > 0.f) || (m < 0.5 && y < 0.f)) ? 1u : 0u;
      d[2] += pos ? -log(m) : -log(1.0 - m);
      const unsigned long long b = (unsigned long long)__double_as_longlong(m);
      c[3] += ((b >> 63) && m == m) ? 1u : 0u;
      keys[e] = (b << 1) | (pos ? 1ull : 0ull);
    }
  }
  post_block_reduce<3, 4>(d, c, dpart, cpart);
}

// one wavefront: lane l sums the blocks l, l + 64, ... in order, then the butterfly.  dout[nd], cout[nc]
static __global__ void __launch_bounds__(64)
k_post_final(const double* __restrict__ dpart, const unsigned long long* __restrict__ cpart, uint32_t nblk, int nd, int nc,
             double* __restrict__ dout, unsigned long long* __restrict__ cout) {
  for (int q = 0; q < nd; q++) {
    double d = 0;
    for (uint32_t b = threadIdx.x; b < nblk; b += 64) d += dpart[(size_t)nd * b + q];
    d = wave_sum_d(d);
    if (threadIdx.x == 0) dout[q] = d;
  }
  for (int q = 0; q < nc; q++) {
    unsigned long long c = 0;
    for (uint32_t b = threadIdx.x; b < nblk; b += 64) c += cpart[(size_t)nc * b + q];
    c = wave_sum_u64(c);
    if (threadIdx.x == 0) cout[q] = c;
  }
}

static __global__ void __launch_bounds__(256)
k_post_this(const float* __restrict__ last, PostArgs a, double* __restrict__ out) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < a.n_rows; e += gridDim.x * blockDim.x) {
    double t, v;
    post_draw(last[e], a, t, v);
    out[e] = t;
  }
}

}  // namespace fmx
