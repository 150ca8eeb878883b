// fmx_ftrl_kernels.h -- the kernels of FTRL-proximal with L1 on the minibatch rule (include/fmx.h "fmx_ftrl_*")
// and the zero count of the parameter tables (fmx_param_sparsity).
//
// Steps 1 and 2 of a batch are AdaGrad's (k_rowsums -> launch_scan, fmx_adapt_kernels.h).  Step 3 is k_ftrl_apply_seg: one owner per
// (batch, feature) segment sums the segment's gradient from the batch-start row WITHOUT a regularisation term
//     g_w  = sum_occ mult_e x                  g_vf = sum_occ mult_e (S_ef x - v_jf x x)
// and takes the proximal step with the coordinate's own z and n
//     n' = fmaf(g, g, n);   da = sqrtf(n') - sqrtf(n)  (= sigma alpha);   z' = z + g - da (1 / alpha) theta
//     D' = (beta + sqrtf(n')) (1 / alpha) + l2;   theta' = |z'| <= l1 ? +0 : -(z' - copysign(l1, z')) / D'
// in fp32, with the correctly rounded division and square root hipcc emits by default (no rsqrt).  theta is READ, not reconstructed
// from (z, n): fmx_set_params may have moved it.  A coordinate whose theta, z and g are 0 (the padding of a row) stays +0.
//
// Shape: the owner block is stateful_seg_block (fmx_adapt_kernels.h) with FtrlRule below: the rule carries two state tables, z then n,
// as Tabs with V's row stride, keeps L2 out of the gradient, and steps a factor with (l1_v, l2_v) and a linear weight with (l1_w, l2_w).
// Everything that decides the bits of the gradient sum -- the round structure, the first-occurrence seed, the occurrence tail (seg_tail,
// fmx_kernels.h) -- is the code AdaGrad and the plain rule run.  No atomics, no LDS: one owner per segment, two runs are bit-identical.
#pragma once
#include "fmx_adapt_kernels.h"

namespace fmx {

// the rule's constants as the kernels take them (fmx_ftrl_begin computes them once)
struct FtrlHyper { float inv_alpha, beta, l1_w, l1_v, l2_w, l2_v; };

// segment groups per round: the resource report per KP is in DESIGN.md section 18 (zero scratch for every KP)
template <int KP> struct FtrlU { static constexpr int value = (KP <= 64) ? 8 : (KP <= 256) ? 4 : (KP <= 512) ? 2 : 1; };

// one coordinate's proximal step; nn and zz come back for the stores
__device__ __forceinline__ float ftrl_step(float theta, float z, float n, float g, float inv_alpha, float beta, float l1, float l2,
                                           float& zz, float& nn) {
  nn = fmaf(g, g, n);
  const float r1 = sqrtf(nn);
  const float da = r1 - sqrtf(n);
  zz = z + g - da * inv_alpha * theta;
  const float D = (beta + r1) * inv_alpha + l2;
  return (fabsf(zz) <= l1) ? 0.f : -(zz - copysignf(l1, zz)) / D;
}

// FTRL-proximal: two tables (z, then n), no L2 in the gradient (it lives in the proximal step), l1 / l2 per parameter kind
struct FtrlRule {
  static constexpr int NT = 2;
  static constexpr bool REG = false;
  Tab st[NT]; FtrlHyper fh;
  __device__ __forceinline__ float step_v(float g, float theta, float (&s)[NT]) const {
    return ftrl_step(theta, s[0], s[1], g, fh.inv_alpha, fh.beta, fh.l1_v, fh.l2_v, s[0], s[1]);
  }
  __device__ __forceinline__ float step_w(float g, float theta, float (&s)[NT]) const {
    return ftrl_step(theta, s[0], s[1], g, fh.inv_alpha, fh.beta, fh.l1_w, fh.l2_w, s[0], s[1]);
  }
};

template <int KP, int U>
__global__ void __launch_bounds__(256)
k_ftrl_apply_seg(const SegWork sw, const Tab tb, const FtrlRule rule, Hyper h) {
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t blk = wave0 * 64u; blk < sw.nseg; blk += nwaves * 64u) stateful_seg_block<FtrlRule, KP, U>(sw, blk, tb, rule, h);
}

// the start state (fmx_ftrl_begin): n = init_acc and z0 = -theta0 D0 - sgn(theta0) l1 with D0 = (beta + sqrt(init_acc)) / alpha + l2, the z
// at which the closed form returns theta0; theta0 = 0 (padding included) gives z0 = 0.  `count` elements of stride 1 (the whole V
// table, padding included) or `count` linear weights `tstride` floats apart.
// One coordinate's z0 is ftrl_start: the checkpoint's sparse criterion (k_ckpt_flag_ftrl, fmx_ckpt_kernels.h) asks whether a stored
// z is still this value, bit for bit, so both call the one function.
__device__ __forceinline__ float ftrl_start(float t, float D0, float l1) {
  const float sg = (t > 0.f) ? l1 : (t < 0.f) ? -l1 : 0.f;
  return -t * D0 - sg;
}

static __global__ void __launch_bounds__(256) k_ftrl_init(const float* __restrict__ theta, size_t tstride, float* __restrict__ z,
                                                          float* __restrict__ n, uint64_t count, float D0, float l1, float init_acc) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    z[i] = ftrl_start(theta[i * tstride], D0, l1);
    n[i] = init_acc;
  }
}

// zero counts of the parameter tables (fmx_param_sparsity).  L lanes (a power of two <= 64) share a feature and stride over its k
// factors, 64 / L features per wavefront round; `== 0.0f` decides (-0 counts, NaN does not); only f < k is looked at.
// out[0] += w_j == 0, out[1] += zero factors, out[2] += rows whose k factors are all zero, out[3] += such rows with (w_j == 0 or !k1).
// Integer sums only (one 64-bit atomic per counter and wavefront), so the order is free.
static __global__ void __launch_bounds__(256) k_param_sparsity(Tab tb, uint64_t n, int k, int k1, uint32_t L,
                                                               unsigned long long* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u, grp = lane / L, sub = lane % L, rpw = 64u / L;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  unsigned long long c[4] = {0ull, 0ull, 0ull, 0ull};
  for (uint64_t r0 = wave * rpw; r0 < n; r0 += nwaves * rpw) {          // (uniform per wavefront: the ballot below sees all 64 lanes)
    const uint64_t j = r0 + grp;
    bool nonzero = false;
    if (j < n) {
      for (uint32_t f = sub; f < (uint32_t)k; f += L) {
        if (tb.V[j * tb.rs + f] == 0.0f) c[1]++; else nonzero = true;
      }
    }
    const unsigned long long bal = __ballot(nonzero);
    const unsigned long long mine = (L == 64u) ? bal : ((bal >> (grp * L)) & ((1ull << L) - 1ull));
    if (j < n && sub == 0) {
      const bool wz = tb.w[j * tb.ws] == 0.0f;
      if (wz) c[0]++;
      if (mine == 0ull) { c[2]++; if (wz || !k1) c[3]++; }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {
    unsigned long long v = c[q];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0 && v) atomicAdd(out + q, v);
  }
}

}  // namespace fmx
