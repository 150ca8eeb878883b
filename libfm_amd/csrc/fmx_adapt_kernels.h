// fmx_adapt_kernels.h -- the owner kernel of AdaGrad on the minibatch rule (include/fmx.h "fmx_adapt_*").
//
// Steps 1 and 2 of a batch are the batch rule's own (k_rowsums -> launch_scan: row sums from the batch-start parameters, the bias
// recurrence in micro-chunks, one multiplier per example).  Step 3 is this kernel: one owner per (batch, feature) segment sums the
// segment's gradient from the batch-start row -- the sum the plain rule multiplies by lr (apply_seg_block, fmx_kernels.h) --
//     g_w  = sum_occ mult_e x                        + nocc regw w_j
//     g_vf = sum_occ mult_e (S_ef x - v_jf x x)      + nocc regv v_jf
// and takes the AdaGrad step with the feature's own accumulators
//     n' = fmaf(g, g, n);   theta' = theta - eta g / sqrtf(n')
// in fp32, with the correctly rounded division and square root hipcc emits by default (no rsqrt: the cost hides under the gathers).
// The accumulators start at init_acc > 0, so n' > 0 and no epsilon is needed; |theta' - theta| < eta whatever the batch sums.
//
// Shape: the dense form of apply_seg_block without seg_idx, cdesc or PRE2.  A wavefront owns 64 consecutive segments (descriptors, first
// occurrence and its multiplier lane-parallel); U segment groups per round, each group's V row, accumulator row, w_j, n_w[j] and first S
// row requested together before anything is used; further occurrences added in occurrence order by the same tail scheme.  The
// accumulator table has V's row stride (Tab `ac`: ac.V = n_v, ac.w = n_w, ac.rs = tb.rs, ac.ws = 1), so row_ld / row_st mask the lanes
// beyond a row for both tables.  No atomics, no LDS: one owner per segment, two runs are bit-identical.
#pragma once
#include "fmx_kernels.h"

namespace fmx {

// segment groups per round: the resource report per KP is in DESIGN.md section 17 (zero scratch for every KP <= 128)
template <int KP> struct AdaptU { static constexpr int value = (KP <= 64) ? 8 : (KP <= 256) ? 4 : 2; };

template <int KP, int U>
__device__ __forceinline__ void adapt_seg_block(const SegWork& sw, uint32_t blk, const Tab tb, const Tab ac, const Hyper& h, const float eta) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR, EPI = Map<KP>::EPI;
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
    float v0[U][VEC], n0[U][VEC], sf[U][VEC];
    float wv0[U], nw0[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t idx = i + u * EPI + g;
      const uint32_t j = bcast_u32<EPI>(jl, idx & 63u);
      const uint32_t e = bcast_u32<EPI>(el, idx & 63u);
      wv0[u] = 0.f; nw0[u] = 1.f;
      if (idx < cnt) {
        if (h.k1 && f == 0) { wv0[u] = tb.w[(size_t)j * tb.ws]; nw0[u] = ac.w[j]; }
        row_ld<VEC, 8>(tb, (size_t)j, f * VEC, v0[u]);
        row_ld<VEC, 8>(ac, (size_t)j, f * VEC, n0[u]);
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
        uint32_t i2 = a + 1;
        // further occurrences, added in occurrence order (apply_seg_block's tail scheme)
        if constexpr (EPI == 1) {
          // one row per wave-wide load: 64 descriptors and their multipliers lane-parallel, the S rows TL at a time, broadcast by v_readlane
          constexpr int TL = (VEC == 1) ? 16 : 8;
          for (uint32_t base = i2; base < b; base += 64) {
            const uint32_t cc = min(64u, b - base);
            TEntry te; te.e = 0; te.x = 0.f; float tm = 0.f;
            if (lane < cc) { te = load_stream8(t_ent + base + lane); tm = mult[te.e]; }
            for (uint32_t q0 = 0; q0 < cc; q0 += TL) {
              float s2[TL][VEC];
#pragma unroll
              for (int q = 0; q < TL; q++) {
                const uint32_t e2 = bcast_u32<1>(te.e, (q0 + q) & 63u);
                if (q0 + q < cc) load_vec<VEC>(S + (size_t)e2 * KP + f * VEC, s2[q]);
                else {
#pragma unroll
                  for (int v = 0; v < VEC; v++) s2[q][v] = 0.f;
                }
              }
#pragma unroll
              for (int q = 0; q < TL; q++) {
                const float x2 = bcast_f32<1>(te.x, (q0 + q) & 63u), m2 = bcast_f32<1>(tm, (q0 + q) & 63u);
                if (q0 + q < cc) {
                  const float mx2 = m2 * x2;
#pragma unroll
                  for (int v = 0; v < VEC; v++) G[v] = fmaf(mx2, s2[q][v], G[v]);
                  A = fmaf(mx2, x2, A); Gw += mx2;
                }
              }
            }
          }
        } else {
          // several rows per wave-wide load (KP < 64): every lane group walks its own segment, TL occurrences at a time
          constexpr int TL = 8;
          for (; i2 < b; i2 += TL) {
            TEntry tt[TL]; float mm[TL]; float s2[TL][VEC];
#pragma unroll
            for (int q = 0; q < TL; q++) { tt[q].e = 0; tt[q].x = 0.f; if (i2 + q < b) tt[q] = t_ent[i2 + q]; }
#pragma unroll
            for (int q = 0; q < TL; q++) {
              mm[q] = 0.f;
              if (i2 + q < b) { mm[q] = mult[tt[q].e]; load_vec<VEC>(S + (size_t)tt[q].e * KP + f * VEC, s2[q]); }
              else {
#pragma unroll
                for (int v = 0; v < VEC; v++) s2[q][v] = 0.f;
              }
            }
#pragma unroll
            for (int q = 0; q < TL; q++) {
              if (i2 + q < b) {
                const float mx2 = mm[q] * tt[q].x;
#pragma unroll
                for (int v = 0; v < VEC; v++) G[v] = fmaf(mx2, s2[q][v], G[v]);
                A = fmaf(mx2, tt[q].x, A); Gw += mx2;
              }
            }
          }
        }
        const float nocc = (float)(b - a);
        float nv[VEC], nn[VEC];
#pragma unroll
        for (int v = 0; v < VEC; v++) {
          const float vv = v0[u][v];
          const float gr = G[v] - vv * A + nocc * h.regv * vv;
          nn[v] = fmaf(gr, gr, n0[u][v]);
          nv[v] = vv - eta * gr / sqrtf(nn[v]);
        }
        row_st<VEC, 8>(tb, (size_t)j, f * VEC, nv);
        row_st<VEC, 8>(ac, (size_t)j, f * VEC, nn);
        if (h.k1 && f == 0) {
          const float wv = wv0[u];
          const float gr = Gw + nocc * h.regw * wv;
          const float nw = fmaf(gr, gr, nw0[u]);
          ac.w[j] = nw;
          tb.w[(size_t)j * tb.ws] = wv - eta * gr / sqrtf(nw);
        }
      }
    }
  }
}

template <int KP, int U>
__global__ void __launch_bounds__(256)
k_adapt_apply_seg(const SegWork sw, const Tab tb, const Tab ac, Hyper h, float eta) {
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t blk = wave0 * 64u; blk < sw.nseg; blk += nwaves * 64u) adapt_seg_block<KP, U>(sw, blk, tb, ac, h, eta);
}

// every accumulator of a session back to its start value (fmx_adapt_begin)
static __global__ void __launch_bounds__(256) k_adapt_fill(float* __restrict__ p, uint64_t n, float value) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = value;
}

}  // namespace fmx
