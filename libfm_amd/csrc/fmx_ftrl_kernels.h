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
// Shape: adapt_seg_block's (a wavefront owns 64 consecutive dense segments; U segment groups per round, each group's V row, z row, n row,
// w_j, z_w[j], n_w[j] and first S row requested together before anything is used; further occurrences added in occurrence order by the
// same two tail schemes; cross-lane reads outside the idx < cnt guard).  The gradient accumulation is a second copy of
// adapt_seg_block's, not a shared inline: k_adapt_apply_seg stays textually what it was, so its resource table cannot move.  z and n
// have V's row stride (Tabs `zt`, `nt`: .V the rows, .w the linear weights' array, .rs = tb.rs, .ws = 1), so row_ld / row_st mask the
// lanes beyond a row for all three tables.  No atomics, no LDS: one owner per segment, two runs are bit-identical.
#pragma once
#include "fmx_kernels.h"

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

template <int KP, int U>
__device__ __forceinline__ void ftrl_seg_block(const SegWork& sw, uint32_t blk, const Tab tb, const Tab zt, const Tab nt, const Hyper& h,
                                               const FtrlHyper& fh) {
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
    float v0[U][VEC], z0[U][VEC], n0[U][VEC], sf[U][VEC];
    float wv0[U], zw0[U], nw0[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t idx = i + u * EPI + g;
      const uint32_t j = bcast_u32<EPI>(jl, idx & 63u);
      const uint32_t e = bcast_u32<EPI>(el, idx & 63u);
      wv0[u] = 0.f; zw0[u] = 0.f; nw0[u] = 0.f;
      if (idx < cnt) {
        if (h.k1 && f == 0) { wv0[u] = tb.w[(size_t)j * tb.ws]; zw0[u] = zt.w[j]; nw0[u] = nt.w[j]; }
        row_ld<VEC, 8>(tb, (size_t)j, f * VEC, v0[u]);
        row_ld<VEC, 8>(zt, (size_t)j, f * VEC, z0[u]);
        row_ld<VEC, 8>(nt, (size_t)j, f * VEC, n0[u]);
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
        // further occurrences, added in occurrence order (adapt_seg_block's two tail schemes, copied: see the head of this file)
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
        float nv[VEC], zz[VEC], nn[VEC];
#pragma unroll
        for (int v = 0; v < VEC; v++) {
          const float vv = v0[u][v];
          nv[v] = ftrl_step(vv, z0[u][v], n0[u][v], G[v] - vv * A, fh.inv_alpha, fh.beta, fh.l1_v, fh.l2_v, zz[v], nn[v]);
        }
        row_st<VEC, 8>(tb, (size_t)j, f * VEC, nv);
        row_st<VEC, 8>(zt, (size_t)j, f * VEC, zz);
        row_st<VEC, 8>(nt, (size_t)j, f * VEC, nn);
        if (h.k1 && f == 0) {
          float zw, nw;
          tb.w[(size_t)j * tb.ws] = ftrl_step(wv0[u], zw0[u], nw0[u], Gw, fh.inv_alpha, fh.beta, fh.l1_w, fh.l2_w, zw, nw);
          zt.w[j] = zw;
          nt.w[j] = nw;
        }
      }
    }
  }
}

template <int KP, int U>
__global__ void __launch_bounds__(256)
k_ftrl_apply_seg(const SegWork sw, const Tab tb, const Tab zt, const Tab nt, Hyper h, FtrlHyper fh) {
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t blk = wave0 * 64u; blk < sw.nseg; blk += nwaves * 64u) ftrl_seg_block<KP, U>(sw, blk, tb, zt, nt, h, fh);
}

// the start state (fmx_ftrl_begin): n = init_acc and z0 = -theta0 D0 - sgn(theta0) l1 with D0 = (beta + sqrt(init_acc)) / alpha + l2, the z
// at which the closed form returns theta0; theta0 = 0 (padding included) gives z0 = 0.  `count` elements of stride 1 (the whole V
// table, padding included) or `count` linear weights `tstride` floats apart.
static __global__ void __launch_bounds__(256) k_ftrl_init(const float* __restrict__ theta, size_t tstride, float* __restrict__ z,
                                                          float* __restrict__ n, uint64_t count, float D0, float l1, float init_acc) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const float t = theta[i * tstride];
    const float sg = (t > 0.f) ? l1 : (t < 0.f) ? -l1 : 0.f;
    z[i] = -t * D0 - sg;
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
