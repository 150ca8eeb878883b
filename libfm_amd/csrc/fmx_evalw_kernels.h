// fmx_evalw_kernels.h -- kernels of fmx_evaluate_weighted (fmx_weighted.hip): the weighted log loss, accuracy,
// RMSE and MAE of a slot, on the pattern of k_evalx_score / k_evalx_final (fmx_eval_kernels.h).
//
// k_evalw_score    grid-stride over the rows: the weighted sums as BLOCK PARTIALS (no float atomics).
// k_evalw_final    one wavefront sums the block partials in a fixed order.
// The grid is evalx_grid(n_rows): two calls with unchanged parameters are bit-identical.  No workgroup waits for another.
#pragma once
#include "fmx_eval_kernels.h"

namespace fmx {

// ----------------------------------------------------------------------------------------------
// fmx_evaluate_weighted: with c_e the row's weight, p, s and l(z) as in k_evalx_score,
//   dpart[EVALW_SUMS * b + {0: sum c, 1: sum c [target >= 0], 2: sum c [target < 0], 3: sum c [correct], 4: sum c l(s p),
//                           5: sum c err^2, 6: sum c |err|}],  cpart[b] = NaN scores (classification)
// every term in fp64; a row of weight 0 adds exactly 0 to every sum (also where l is +inf or the score NaN).  Sums 1 .. 4 are
// classification's, 5 and 6 regression's; the others stay 0.  lane -> wavefront (xor butterfly) -> block (wave order) -> blocks.
// ----------------------------------------------------------------------------------------------
constexpr int EVALW_SUMS = 7;

static __global__ void __launch_bounds__(256)
k_evalw_score(const float* __restrict__ rest, const float* __restrict__ target, const float* __restrict__ weight, uint32_t n_rows, Hyper h,
              const double* __restrict__ w0_ptr, uint32_t link, double* __restrict__ dpart, unsigned long long* __restrict__ cpart) {
  __shared__ double dred[EVALW_SUMS][4];
  __shared__ unsigned long long cred[4];
  const float w0 = h.k0 ? (float)(*w0_ptr) : 0.f;
  double d[EVALW_SUMS];
#pragma unroll
  for (int q = 0; q < EVALW_SUMS; q++) d[q] = 0.0;
  unsigned long long nn = 0;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_rows; e += gridDim.x * blockDim.x) {
    const float p = w0 + rest[e];                                    // (exactly k_evalx_score: what fmx_predict returns)
    const float y = target[e];
    const float cf = weight[e];
    const double c = (double)cf;
    d[0] += c;
    if (h.task == 0) {
      if (cf != 0.f) {
        const float pc = fmaxf(h.min_target, fminf(h.max_target, p));  // fm_learn.h:138-139
        const double err = (double)pc - (double)y;
        d[5] += c * (err * err); d[6] += c * fabs(err);
      }
    } else {
      const bool pos = (y >= 0);                                     // fm_learn.h:118
      nn += (p != p) ? 1u : 0u;
      if (cf != 0.f) {
        if (pos) d[1] += c; else d[2] += c;
        if (((p >= 0) && (y >= 0)) || ((p < 0) && (y < 0))) d[3] += c;
        d[4] += c * evalx_loss(pos ? (double)p : -(double)p, link);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < EVALW_SUMS; q++) d[q] = wave_sum_d(d[q]);
  nn = wave_sum_u64(nn);
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (int q = 0; q < EVALW_SUMS; q++) dred[q][w] = d[q];
    cred[w] = nn;
  }
  __syncthreads();
  if (threadIdx.x < EVALW_SUMS) {
    const uint32_t q = threadIdx.x;
    double s = 0;
    for (int i = 0; i < 4; i++) s += dred[q][i];
    dpart[EVALW_SUMS * blockIdx.x + q] = s;
  }
  if (threadIdx.x == 64) cpart[blockIdx.x] = (cred[0] + cred[1]) + (cred[2] + cred[3]);
}

// one wavefront: lane l sums the blocks l, l + 64, ... in order, then the butterfly.  dout[EVALW_SUMS], cout[1]
static __global__ void __launch_bounds__(64)
k_evalw_final(const double* __restrict__ dpart, const unsigned long long* __restrict__ cpart, uint32_t nblk,
              double* __restrict__ dout, unsigned long long* __restrict__ cout) {
  for (int q = 0; q < EVALW_SUMS; q++) {
    double d = 0;
    for (uint32_t b = threadIdx.x; b < nblk; b += 64) d += dpart[EVALW_SUMS * b + q];
    d = wave_sum_d(d);
    if (threadIdx.x == 0) dout[q] = d;
  }
  unsigned long long c = 0;
  for (uint32_t b = threadIdx.x; b < nblk; b += 64) c += cpart[b];
  c = wave_sum_u64(c);
  if (threadIdx.x == 0) cout[0] = c;
}

}  // namespace fmx
