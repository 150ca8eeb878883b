// fmx_hofm_kernels.h -- the third-order FM (the higher-order FM of Blondel et al., NIPS 2016, at order 3; include/fmx.h "fmx_hofm_*",
// DESIGN.md section 32).
//
//   y(x) = w0 + sum_j w_j x_j + sum_{c < k2} sum_{a<b} z_a z_b + sum_{c >= k2} sum_{a<b<d} z_a z_b z_d,      z_a = x_a v[j_a][c]
//
// A row of k2 + k3 factors: columns [0, k2) are the pairwise factors of the plain FM, columns [k2, k2 + k3) the third-order factors.
// With the power sums p_m[c] = sum_a z_a^m of an example, Newton's identities give the elementary symmetric sums per column:
//     E2 = 1/2 (p1^2 - p2)                    the pair term, and what the third-order gradient needs
//     E3 = 1/3 (E2 p1 - p1 p2 + p3)           = (p1^3 - 3 p1 p2 + 2 p3) / 6, the third-order term
//     dE3/dv[j_a][c] = x_a (E2 - z_a p1 + z_a^2)
// Over the occurrences of feature j in a batch (multiplier m, value x), with v = v[j][c]:
//     g = sum m x E2_e - v sum m x^2 p1_e + v^2 sum m x^3                                                    (c >= k2)
//     g = sum m x p1_e - v sum m x^2                                                                          (c <  k2, the plain FM)
// so an occurrence brings TWO rows in the third-order columns (E2_e and p1_e) where the pair columns bring one (p1_e).
//
// No matrix instructions: there is no dense product here.  An example costs nnz rows gathered against 3 multiply-adds per third-order
// element; the kernel is bound by the gather like k_rowsums.  No LDS: the three power sums of a lane's VEC columns live in registers.
// No float atomics: one wavefront per example, one owner per segment, every lane in a fixed order -- two runs give the same bits.
// With k3 = 0 every expression a pair column passes through is k_rowsums' and stateful_seg_block's own, in the same order: the epoch
// then leaves fmx_adapt_epoch's parameters bit for bit.
#pragma once
#include "fmx_adapt_kernels.h"

namespace fmx {

// ----------------------------------------------------------------------------------------------
// k_hofm_rows: one wavefront per example, grid-strided (k_rowsums' launch shape).
//   1. the row's V rows and w_j arrive through the Tab / row_ld lane map with row_sums_gather's rounds (U rounds of EPI rows in flight).
//      Lane (g, f) holds columns [f VEC, f VEC + VEC) of the entries of lane group g.  The split into pair and third-order columns is per
//      COLUMN: t3 = (column >= k2), so a lane whose VEC columns straddle k2 is mixed.  A pair column adds z into p1 and z^2 into the
//      lane's one scalar sq (k_rowsums' arithmetic); a third-order column adds z, z^2, z^3 into p1, p2, p3 of its column.  p3 is never
//      formed for a pair column, and neither is a per-column p2.
//   2. p1, p2, p3 are summed over the EPI lane groups (KP < 64), and the lanes of group 0 form per column
//          pair column:   hv = p1,             part += 1/2 p1^2            (- 1/2 sq was taken with lin, per lane)
//          third order:   hv = E2,             part += E3
//      in column order; then the DPP reduction of k_rowsums leaves rest_e.
//   3. TRAIN stores H_e = hv (RW floats: p1 in the pair columns, E2 in the third-order columns) and P_e = p1 of the columns [c0, RW)
//      alone, c0 = k2 rounded down to VEC (the lane map's granularity): RW + (RW - c0) floats of scratch per example.  The padding
//      columns [k2 + k3, RW) hold zeros in V, so every sum there is zero and so is their gradient.
// ----------------------------------------------------------------------------------------------
// rounds in flight: k_rowsums' 8, and 4 from 512 columns on, where the three sums of VEC columns leave room for no more (the order of
// every sum is the entries' order whatever U is)
template <int KP> struct HofmU { static constexpr int value = (KP <= 256) ? RowsF32::Lanes<KP>::U : 4; };

template <int KP, bool TRAIN>
__global__ void __launch_bounds__(256)
k_hofm_rows(const Entry* __restrict__ ent, const uint64_t* __restrict__ row_ptr, uint64_t row0, uint32_t n_rows, const Tab tb, int k1,
            uint32_t k2, uint32_t RW, uint32_t c0, float* __restrict__ rest, float* __restrict__ H, float* __restrict__ P) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR, EPI = Map<KP>::EPI, U = HofmU<KP>::value;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = lane / LPR, f = lane % LPR;
  const uint32_t col0 = f * VEC;
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t e = wave0; e < n_rows; e += nwaves) {
    const uint64_t a = row_ptr[row0 + e];
    const uint32_t size = (uint32_t)(row_ptr[row0 + e + 1] - a);
    const Entry* __restrict__ re = ent + a;
    float sum[VEC], p2[VEC], p3[VEC], sq = 0.f, lin = 0.f;
#pragma unroll
    for (int v = 0; v < VEC; v++) { sum[v] = 0.f; p2[v] = 0.f; p3[v] = 0.f; }
    for (uint32_t base = 0; base < size; base += 64) {
      const uint32_t cnt = min(64u, size - base);
      Entry en; en.id = 0; en.value = 0.f;
      if (lane < cnt) {
        en = load_stream8(re + base + lane);
        if (k1) lin += load_w(tb.w + (size_t)en.id * tb.ws) * en.value;
      }
      for (uint32_t i = 0; i < cnt; i += EPI * U) {
        float vr[U][VEC]; float xs[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const uint32_t idx = i + u * EPI + g;
          const uint32_t id = bcast_u32<EPI>(en.id, idx & 63u);
          xs[u] = bcast_f32<EPI>(en.value, idx & 63u);
          if (idx < cnt) {
            row_ld<VEC, 4>(tb, (size_t)id, col0, vr[u]);
          } else {
            xs[u] = 0.f;
#pragma unroll
            for (int v = 0; v < VEC; v++) vr[u][v] = 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
          for (int v = 0; v < VEC; v++) {
            const float d = vr[u][v] * xs[u];
            sum[v] += d;
            const bool t3 = col0 + (uint32_t)v >= k2;
            const float dp = t3 ? 0.f : d, d3 = t3 ? d : 0.f;        // (fmaf(0, 0, s) is s: the other kind's sums stay as they are)
            sq = fmaf(dp, dp, sq);
            p2[v] = fmaf(d3, d3, p2[v]);
            p3[v] = fmaf(d3 * d3, d3, p3[v]);
          }
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      sum[v] = subgroup_allsum<LPR>(sum[v]);
      p2[v] = subgroup_allsum<LPR>(p2[v]);
      p3[v] = subgroup_allsum<LPR>(p3[v]);
    }
    float part = lin - 0.5f * sq;
    if (lane < LPR) {
      float hv[VEC];
#pragma unroll
      for (int v = 0; v < VEC; v++) {
        const float e2 = 0.5f * fmaf(sum[v], sum[v], -p2[v]);
        const float e3 = fmaf(-sum[v], p2[v], fmaf(e2, sum[v], p3[v])) * (1.0f / 3.0f);
        if (col0 + (uint32_t)v >= k2) { hv[v] = e2; part += e3; }
        else { hv[v] = sum[v]; part = fmaf(0.5f * sum[v], sum[v], part); }
      }
      if (TRAIN && col0 < RW) {
        store_vec<VEC>(H + (size_t)e * RW + col0, hv);
        if (col0 >= c0) store_vec<VEC>(P + (size_t)e * (RW - c0) + (col0 - c0), sum);
      }
    }
    part = wave_sum_dpp(part);
    if (lane == 0) rest[e] = part;
  }
}

// ----------------------------------------------------------------------------------------------
// The owner of a (batch, feature) segment: stateful_seg_block with AdagradRule and a sum source with SECOND.  An occurrence in example e
// reads H_e through loads masked to the RW floats of a row, and -- the lanes from column c0 on -- P_e as its second row; seg_tail adds
// G = sum m x H_e, A = sum m x^2, G2 = sum m x^2 P_e and A3 = sum m x^3 in occurrence order.  The own term is v A in the pair columns
// and v G2 - v^2 A3 in the third-order columns (third()); a mixed lane holds both kinds.
// ----------------------------------------------------------------------------------------------
struct HofmStride {
  uint32_t rw;
  template <int KP> __device__ __forceinline__ size_t of() const { return (size_t)rw; }
  __device__ __forceinline__ bool live(uint32_t off) const { return off < rw; }
};
template <int VEC> struct HofmSecond {
  static constexpr bool ON = true;
  const float* P; uint32_t c0, rw;
  float G2[VEC]; float A3;
  __device__ __forceinline__ bool live(uint32_t off) const { return off >= c0 && off < rw; }
  __device__ __forceinline__ const float* row(uint32_t e, uint32_t off) const { return P + (size_t)e * (rw - c0) + (off - c0); }
};
struct HofmSums {
  static constexpr bool PLAIN = false, COLUMN_SELF = false, SECOND = true;
  template <int VEC> using Second = HofmSecond<VEC>;
  const float* Hs; const float* P;
  uint32_t k2, c0, rw;
  template <int KP> __device__ __forceinline__ const float* base(const float*, uint32_t) const { return Hs; }
  __device__ __forceinline__ HofmStride stride() const { return HofmStride{rw}; }
  template <int VEC> __device__ __forceinline__ HofmSecond<VEC> second() const {
    HofmSecond<VEC> s; s.P = P; s.c0 = c0; s.rw = rw; s.A3 = 0.f;
#pragma unroll
    for (int v = 0; v < VEC; v++) s.G2[v] = 0.f;
    return s;
  }
  __device__ __forceinline__ bool third(uint32_t col) const { return col >= k2; }
};

// segment groups per round: AdaptU's, and one at 1024 columns, where a group holds five rows of 16 floats per lane before its tail
template <int KP> struct HofmOwnerU { static constexpr int value = (KP <= 512) ? AdaptU<KP>::value : 1; };

template <int KP, int U>
__global__ void __launch_bounds__(256)
k_hofm_apply_seg(const SegWork sw, const Tab tb, const AdagradRule rule, Hyper h, const HofmSums sum) {
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t blk = wave0 * 64u; blk < sw.nseg; blk += nwaves * 64u) stateful_seg_block<AdagradRule, KP, U, HofmSums>(sw, blk, tb, rule, h, sum);
}

}  // namespace fmx
