// fmx_adapt_kernels.h -- the owner block of the optimisers that keep per-coordinate state on the minibatch rule, and AdaGrad as its
// first rule (include/fmx.h "fmx_adapt_*"; FTRL, the second rule, is fmx_ftrl_kernels.h).
//
// Steps 1 and 2 of a batch are the batch rule's own (k_rowsums -> launch_scan: row sums from the batch-start parameters, the bias
// recurrence in micro-chunks, one multiplier per example).  Step 3 is stateful_seg_block: one owner per (batch, feature) segment sums
// the segment's gradient from the batch-start row -- the sum the plain rule multiplies by lr (apply_seg_block, fmx_kernels.h) --
//     g_w  = sum_occ mult_e x                        [+ nocc regw w_j]
//     g_vf = sum_occ mult_e (S_ef x - v_jf x x)      [+ nocc regv v_jf]
// and hands every coordinate's sum, its theta and its state to the rule's step.  A rule is a small struct passed by value to the kernel:
//     NT        how many state tables ride along (1 or 2), as Tabs `st[NT]` with V's row stride (.V the rows, .w the linear weights'
//               array, .rs = tb.rs, .ws = 1), so row_ld / row_st mask the lanes beyond a row for every table;
//     REG       whether the bracketed L2 term belongs to the gradient;
//     step_v / step_w (g, theta, s[NT])   one factor's / one linear weight's step: returns the new theta, s becomes the new state.
// AdaGrad keeps n and takes
//     n' = fmaf(g, g, n);   theta' = theta - eta g / sqrtf(n')
// in fp32, with the correctly rounded division and square root hipcc emits by default (no rsqrt: the cost hides under the gathers).
// The accumulators start at init_acc > 0, so n' > 0 and no epsilon is needed; |theta' - theta| < eta whatever the batch sums.
//
// Shape: the dense form of apply_seg_block without seg_idx, cdesc or PRE2.  A wavefront owns 64 consecutive segments (descriptors, first
// occurrence and its multiplier lane-parallel); U segment groups per round, each group's V row, state rows, w_j, the state of w_j and
// first S row requested together before anything is used; further occurrences added in occurrence order by seg_tail, the one tail the
// plain rule's block walks too.  No atomics, no LDS: one owner per segment, two runs are bit-identical.
#pragma once
#include "fmx_kernels.h"

namespace fmx {

template <class R, int KP, int U>
__device__ __forceinline__ void stateful_seg_block(const SegWork& sw, uint32_t blk, const Tab tb, const R& rule, const Hyper& h) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR, EPI = Map<KP>::EPI, NT = R::NT;
  const uint32_t lane = threadIdx.x & 63u, g = lane / LPR, f = lane % LPR;
  const TEntry* __restrict__ t_ent = sw.t_ent;
  const float* __restrict__ S = sw.S;
  const float* __restrict__ mult = sw.mult;
  const uint32_t cnt = min(64u, sw.nseg - blk);
  uint32_t jl = 0, al = 0, bl = 0, el = 0; float xl = 0.f, ml = 0.f;
  if (lane < cnt) {
    const uint32_t s = blk + lane;
    jl = sw.seg_feat[s];
    al = sw.seg_rel[s];
    bl = (s + 1 < sw.nseg_batch) ? sw.seg_rel[s + 1] : sw.batch_nnz;
    const TEntry te = load_stream8(t_ent + al);
    el = te.e; xl = te.x;
    ml = mult[el];
  }
  for (uint32_t i = 0; i < cnt; i += EPI * U) {
    float v0[U][VEC], s0[U][NT][VEC], sf[U][VEC];
    float wv0[U], sw0[U][NT];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t idx = i + u * EPI + g;
      const uint32_t j = bcast_u32<EPI>(jl, idx & 63u);
      const uint32_t e = bcast_u32<EPI>(el, idx & 63u);
      wv0[u] = 0.f;
#pragma unroll
      for (int t = 0; t < NT; t++) sw0[u][t] = 1.f;               // (never read where it is not loaded: the load and the use share one guard)
      if (idx < cnt) {
        if (h.k1 && f == 0) {
          wv0[u] = tb.w[(size_t)j * tb.ws];
#pragma unroll
          for (int t = 0; t < NT; t++) sw0[u][t] = rule.st[t].w[j];
        }
        row_ld<VEC, 8>(tb, (size_t)j, f * VEC, v0[u]);
#pragma unroll
        for (int t = 0; t < NT; t++) row_ld<VEC, 8>(rule.st[t], (size_t)j, f * VEC, s0[u][t]);
        load_vec<VEC>(S + (size_t)e * KP + f * VEC, sf[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t idx = i + u * EPI + g;
      const uint32_t j = bcast_u32<EPI>(jl, idx & 63u);
      const uint32_t a = bcast_u32<EPI>(al, idx & 63u);
      const uint32_t b = bcast_u32<EPI>(bl, idx & 63u);
      const float x = bcast_f32<EPI>(xl, idx & 63u);               // (cross-lane reads run with every lane enabled: outside the guard)
      const float m = bcast_f32<EPI>(ml, idx & 63u);
      if (idx < cnt) {
        float G[VEC]; float A, Gw;
        const float mx = m * x;
#pragma unroll
        for (int v = 0; v < VEC; v++) G[v] = mx * sf[u][v];
        A = mx * x; Gw = mx;
        seg_tail<KP>(t_ent, S, mult, a + 1, b, lane, f, G, A, Gw);
        const float nocc = (float)(b - a);
        float nv[VEC];
#pragma unroll
        for (int v = 0; v < VEC; v++) {
          const float vv = v0[u][v];
          float gr, s[NT];
          if constexpr (R::REG) gr = G[v] - vv * A + nocc * h.regv * vv;
          else gr = G[v] - vv * A;
#pragma unroll
          for (int t = 0; t < NT; t++) s[t] = s0[u][t][v];
          nv[v] = rule.step_v(gr, vv, s);
#pragma unroll
          for (int t = 0; t < NT; t++) s0[u][t][v] = s[t];
        }
        row_st<VEC, 8>(tb, (size_t)j, f * VEC, nv);
#pragma unroll
        for (int t = 0; t < NT; t++) row_st<VEC, 8>(rule.st[t], (size_t)j, f * VEC, s0[u][t]);
        if (h.k1 && f == 0) {
          const float wv = wv0[u];
          float gr;
          if constexpr (R::REG) gr = Gw + nocc * h.regw * wv;
          else gr = Gw;
          tb.w[(size_t)j * tb.ws] = rule.step_w(gr, wv, sw0[u]);
#pragma unroll
          for (int t = 0; t < NT; t++) rule.st[t].w[j] = sw0[u][t];
        }
      }
    }
  }
}

// AdaGrad: one table (the accumulators n), L2 inside the gradient, the same step for factors and linear weights
struct AdagradRule {
  static constexpr int NT = 1;
  static constexpr bool REG = true;
  Tab st[NT]; float eta;
  __device__ __forceinline__ float step_v(float gr, float theta, float (&s)[NT]) const {
    s[0] = fmaf(gr, gr, s[0]);
    return theta - eta * gr / sqrtf(s[0]);
  }
  __device__ __forceinline__ float step_w(float gr, float theta, float (&s)[NT]) const { return step_v(gr, theta, s); }
};

// segment groups per round: the resource report per KP is in DESIGN.md section 17 (zero scratch for every KP)
template <int KP> struct AdaptU { static constexpr int value = (KP <= 64) ? 8 : (KP <= 256) ? 4 : 2; };

template <int KP, int U>
__global__ void __launch_bounds__(256)
k_adapt_apply_seg(const SegWork sw, const Tab tb, const AdagradRule rule, Hyper h) {
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t blk = wave0 * 64u; blk < sw.nseg; blk += nwaves * 64u) stateful_seg_block<AdagradRule, KP, U>(sw, blk, tb, rule, h);
}

// every accumulator of a session back to its start value (fmx_adapt_begin)
static __global__ void __launch_bounds__(256) k_adapt_fill(float* __restrict__ p, uint64_t n, float value) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = value;
}

}  // namespace fmx
