// fmx_eval_kernels.h -- kernels of fmx_evaluate_ex (fmx_eval.hip): exact AUC and log loss of a slot.
//
// k_evalx_score   grid-stride over the rows: p = w0 + rest, the loss term, the regression terms and the counts as BLOCK PARTIALS
//                 (no float atomics), and on classification handles one sort key per row.
// k_evalx_final   one wavefront sums the block partials in a fixed order.
// EvalxIsNeg / EvalxHead   what the two library scans read from the sorted keys: "is a negative" and "index of the position if it
//                 heads a run of equal scores, else 0".
// k_evalx_ranksum over the sorted keys and the two scans: every positive adds negbefore[i] + negbefore[run head of i].
//
// Both grids are a fixed function of n_rows (evalx_grid), every fp64 sum runs lane -> wavefront (xor butterfly) -> block (wave
// order) -> blocks (k_evalx_final): two calls with unchanged parameters are bit-identical.  No workgroup waits for another.
#pragma once
#include "fmx_kernels.h"

namespace fmx {

constexpr uint32_t EVALX_BLOCKS = 2048;      // cap of the grids (256 CUs x 8 workgroups of 256 threads); longer slots grid-stride
inline uint32_t evalx_grid(uint32_t n_rows) { return n_rows < EVALX_BLOCKS * 256u ? (n_rows + 255u) / 256u : EVALX_BLOCKS; }
constexpr int EVALX_KEY_BITS = 33;           // label in bit 0, the order-preserving image of the score in bits 1 .. 32

// the loss of one row, z = s * p in fp64 (fmx.h: FMX_LINK_*)
__device__ __forceinline__ double evalx_loss(double z, uint32_t link) {
  if (link == 0u) return fmax(-z, 0.0) + log1p(exp(-fabs(z)));
  return -log(0.5 * erfc(-z / sqrt(2.0)));                          // +inf where erfc underflows (z below about -38)
}

// order-preserving image of a float: negatives have all their bits flipped, the others their sign bit.  -0 is mapped on +0
// first (float comparison: +0 == -0).
__device__ __forceinline__ uint32_t evalx_key32(float p) {
  const float pz = (p == 0.f) ? 0.f : p;
  const uint32_t b = __float_as_uint(pz);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// partials of block b: dpart[3 * b + {0: sum err^2, 1: sum |err|, 2: sum loss}], cpart[3 * b + {0: pos, 1: NaN scores, 2: correct}]
// add_w0 = 0: `rest` already holds the finished y-hat (fmx_predict_finish: the group path)
static __global__ void __launch_bounds__(256)
k_evalx_score(const float* __restrict__ rest, const float* __restrict__ target, uint32_t n_rows, Hyper h, int add_w0,
              const double* __restrict__ w0_ptr, uint32_t link, double* __restrict__ dpart, unsigned long long* __restrict__ cpart,
              unsigned long long* __restrict__ keys) {
  __shared__ double dred[3][4];
  __shared__ unsigned long long cred[3][4];
  const float w0 = (add_w0 && h.k0) ? (float)(*w0_ptr) : 0.f;
  double se = 0, ae = 0, ls = 0;
  unsigned long long np = 0, nn = 0, nc = 0;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_rows; e += gridDim.x * blockDim.x) {
    const float p = add_w0 ? w0 + rest[e] : rest[e];                 // (exactly k_yhat / k_eval: what fmx_predict returns)
    const float y = target[e];
    if (h.task == 0) {
      const float pc = fmaxf(h.min_target, fminf(h.max_target, p));  // fm_learn.h:138-139
      const double err = (double)pc - (double)y;
      se += err * err; ae += fabs(err);
    } else {
      const bool pos = (y >= 0);                                     // fm_learn.h:118
      np += pos ? 1u : 0u;
      nn += (p != p) ? 1u : 0u;
      nc += (((p >= 0) && (y >= 0)) || ((p < 0) && (y < 0))) ? 1u : 0u;
      ls += evalx_loss(pos ? (double)p : -(double)p, link);
      keys[e] = ((unsigned long long)evalx_key32(p) << 1) | (pos ? 1ull : 0ull);
    }
  }
  se = wave_sum_d(se); ae = wave_sum_d(ae); ls = wave_sum_d(ls);
  np = wave_sum_u64(np); nn = wave_sum_u64(nn); nc = wave_sum_u64(nc);
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) { dred[0][w] = se; dred[1][w] = ae; dred[2][w] = ls; cred[0][w] = np; cred[1][w] = nn; cred[2][w] = nc; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const uint32_t q = threadIdx.x;
    double d = 0; unsigned long long c = 0;
    for (int i = 0; i < 4; i++) { d += dred[q][i]; c += cred[q][i]; }
    dpart[3 * blockIdx.x + q] = d; cpart[3 * blockIdx.x + q] = c;
  }
}

// one wavefront: lane l sums the blocks l, l + 64, ... in order, then the butterfly.  dout[3], cout[3]
static __global__ void __launch_bounds__(64)
k_evalx_final(const double* __restrict__ dpart, const unsigned long long* __restrict__ cpart, uint32_t nblk,
              double* __restrict__ dout, unsigned long long* __restrict__ cout) {
  for (int q = 0; q < 3; q++) {
    double d = 0; unsigned long long c = 0;
    for (uint32_t b = threadIdx.x; b < nblk; b += 64) { d += dpart[3 * b + q]; c += cpart[3 * b + q]; }
    d = wave_sum_d(d); c = wave_sum_u64(c);
    if (threadIdx.x == 0) { dout[q] = d; cout[q] = c; }
  }
}

// the inputs of the two scans, read straight from the sorted keys (no flag arrays).  Inside a run of equal scores the negatives
// (label bit 0) come first.
struct EvalxIsNeg { __host__ __device__ __forceinline__ uint32_t operator()(unsigned long long k) const { return (uint32_t)(~k & 1ull); } };
struct EvalxHead {                            // i if position i heads a run of equal scores, else 0 (position 0 heads its run with 0 anyway)
  const unsigned long long* ks;
  __host__ __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return (i > 0 && (ks[i] >> 1) != (ks[i - 1] >> 1)) ? i : 0u; }
};

// negbefore[i] = negatives at sorted positions < i, runhead[i] = first position of i's run of equal scores.  A positive at i has
// negbefore[i] negatives with a score <= its own (those of its run all precede it) and negbefore[runhead[i]] with a score < its
// own: together 2 * below + equal.  Integer sum: exact in any order, so one 64-bit atomic per block.
static __global__ void __launch_bounds__(256)
k_evalx_ranksum(const unsigned long long* __restrict__ ks, const uint32_t* __restrict__ negbefore, const uint32_t* __restrict__ runhead,
                uint32_t n, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long red[4];
  unsigned long long s = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    if (ks[i] & 1ull) s += (unsigned long long)negbefore[i] + (unsigned long long)negbefore[runhead[i]];
  s = wave_sum_u64(s);
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = (red[0] + red[1]) + (red[2] + red[3]);
    if (t) atomicAdd(out, t);
  }
}

}  // namespace fmx
