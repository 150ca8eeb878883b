// fmx_pair_rule_kernels.h -- the owner kernel of the pair epochs that step with an open session's per-coordinate rule
// (include/fmx.h "fmx_adapt_pair_epoch*", "fmx_ftrl_pair_epoch*") and the one owner launch both pair drivers
// (fmx_pair.hip, fmx_pairneg.hip) end in.
//
// A pair epoch in FMX_SGD_MINIBATCH is unchanged up to the owner: the same pairs and negatives, k_pair_sums / k_pn_sums, the same
// (batch, feature) bucketing.  k_pair_apply_rule then owns one segment per wavefront like k_pair_apply and walks it in the same
// order (pair_seg_walk below), so per coordinate
//     g = sum over the pairs t of the batch that contain j of (mult_t grad_tj [+ reg theta_j with R::REG])        (fp64, pair order)
// is the sum the plain rule multiplies by lr -- one regularisation term per distinct pair for AdaGrad, none for FTRL (L2 lives in
// its proximal step).  g32 = (float)g goes with the batch-start theta and the coordinate's state through rule.step_v / step_w
// (AdagradRule, fmx_adapt_kernels.h; FtrlRule, fmx_ftrl_kernels.h): the fp32 step of the pointwise sessions, on the session's own
// tables, so pointwise and pairwise epochs may alternate.
//
// Shape: lanes < LPR hold VEC factors each; the V row, the NT state rows, w_j and its state are requested before the walk starts and
// arrive under it; fp64 accumulators; the stores are theta' and the state, guarded by act && ff < k (the padding of a row is never
// read or written).  No LDS, no atomics: one owner per segment, two runs are bit-identical.
#pragma once
#include "fmx_internal.h"
#include "fmx_pair_kernels.h"
#include "fmx_ftrl_kernels.h"

namespace fmx {

// VEC floats of a row of V's layout for the lane that holds them: one vector access where all of them are factors (full), element
// by element along the edge of num_factor, nothing beyond it (the loads leave `fill`)
template <int VEC>
__device__ __forceinline__ void rule_row_ld(const float* __restrict__ p, bool full, bool act, int f0, int k, float fill, float (&out)[VEC]) {
  if (full) load_vec<VEC>(p, out);
  else {
#pragma unroll
    for (int v = 0; v < VEC; v++) out[v] = (act && f0 + v < k) ? p[v] : fill;
  }
}
template <int VEC>
__device__ __forceinline__ void rule_row_st(float* __restrict__ p, bool full, bool act, int f0, int k, const float (&in)[VEC]) {
  if (full) store_vec<VEC>(p, in);
  else {
#pragma unroll
    for (int v = 0; v < VEC; v++)
      if (act && f0 + v < k) p[v] = in[v];
  }
}

// the walk of one (batch, feature) segment: the entries tent[a .. b) of feature j in pair order.  Per pair the gradient of its entries,
// then aw / av += mult_t * grad_t [+ reg * theta_j(start) with REG: one regularisation term per distinct pair], fp64, from the
// batch-start w0j / v0[].  It is k_pair_apply's loop statement for statement (tags and S rows per ROWS as there).  k_pair_apply keeps
// its own copy: called from there, this function left the compiler another contraction of the last pair's mult * g + reg * theta
// (the product that is rounded before the fma changed sides), which can move the last bit of the plain rule's fp64 sum (DESIGN.md
// section 22).
template <int KP, int ROWS, bool REG>
__device__ __forceinline__ void pair_seg_walk(const TEntry* __restrict__ tent, uint32_t a, uint32_t b, const float* __restrict__ S,
                                              const double* __restrict__ mult, const Hyper& h, int k, uint32_t lane, bool act,
                                              const double (&v0)[Map<KP>::VEC], double w0j, double& aw_out, double (&av)[Map<KP>::VEC]) {
  constexpr int VEC = Map<KP>::VEC;
  constexpr uint32_t TAG_BITS = ROWS == 2 ? 1u : 2u, TAG_MASK = (1u << TAG_BITS) - 1u;
  static_assert(ROWS == 2 || ROWS == 3, "tags: x_a, x_b and optionally both");
  double gv[VEC];
#pragma unroll
  for (int v = 0; v < VEC; v++) { gv[v] = 0.0; av[v] = 0.0; }
  double gw = 0.0, aw = 0.0;
  uint32_t cur = tent[a].e >> TAG_BITS;
  for (uint32_t i = a; i < b; i++) {
    const TEntry te = tent[i];
    const uint32_t t = te.e >> TAG_BITS, side = te.e & TAG_MASK;
    if (t != cur) {                                        // the previous pair's gradient is complete
      const double mt = mult[cur];
      if constexpr (REG) aw += mt * gw + h.regw_d * w0j; else aw += mt * gw;
#pragma unroll
      for (int v = 0; v < VEC; v++) {
        if constexpr (REG) av[v] += mt * gv[v] + h.regv_d * v0[v]; else av[v] += mt * gv[v];
        gv[v] = 0.0;
      }
      gw = 0.0; cur = t;
    }
    const double x = (double)te.x;
    if (ROWS == 2 || side < 2u) gw = side ? gw - x : gw + x;
    const float* Sr = S + ((size_t)t * ROWS + side) * KP;
    const double xs = (ROWS == 3 && side == 2u) ? 0.0 : x;   // (v x x as (v x) x, as k_pair_apply)
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      const int ff = (int)(lane * VEC + v);
      const double sf = (act && ff < k) ? (double)Sr[ff] : 0.0;
      const double gr = sf * x - v0[v] * x * xs;
      gv[v] = (side == 1u) ? gv[v] - gr : gv[v] + gr;
    }
  }
  {
    const double mt = mult[cur];
    if constexpr (REG) aw += mt * gw + h.regw_d * w0j; else aw += mt * gw;
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      if constexpr (REG) av[v] += mt * gv[v] + h.regv_d * v0[v]; else av[v] += mt * gv[v];
    }
  }
  aw_out = aw;
}

// ROWS = 2: the stored pairs of fmx_pair.hip; 3: the query's entries once, tag 2 (fmx_pairneg.hip) -- as k_pair_apply
template <class R, int KP, int ROWS>
__global__ void __launch_bounds__(256)
k_pair_apply_rule(const TEntry* __restrict__ tent, const uint32_t* __restrict__ seg_head, const uint32_t* __restrict__ seg_feat,
                  uint32_t s0, uint32_t s1, const float* __restrict__ S, const double* __restrict__ mult, const Tab tb, const R rule,
                  Hyper h, int k) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR, NT = R::NT;
  const uint32_t lane = threadIdx.x & 63u;
  const bool act = lane < (uint32_t)LPR;
  const int f0 = (int)(lane * VEC);
  const bool full = act && f0 + VEC <= k;
  const uint32_t wave0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t s = s0 + wave0; s < s1; s += nwaves) {
    const uint32_t j = seg_feat[s], a = seg_head[s], b = seg_head[s + 1];
    const size_t ro = (size_t)j * tb.rs + (size_t)f0;          // (the state tables have V's row stride)
    float th[VEC], st[NT][VEC], wj = 0.f, sw[NT];
    rule_row_ld<VEC>(tb.V + ro, full, act, f0, k, 0.f, th);
#pragma unroll
    for (int t = 0; t < NT; t++) rule_row_ld<VEC>(rule.st[t].V + ro, full, act, f0, k, 1.f, st[t]);
#pragma unroll
    for (int t = 0; t < NT; t++) sw[t] = 1.f;                   // (never used where it is not loaded: the step shares the guard)
    if (h.k1) {
      wj = tb.w[(size_t)j * tb.ws];
#pragma unroll
      for (int t = 0; t < NT; t++) sw[t] = rule.st[t].w[j];
    }
    double v0[VEC], av[VEC], aw;
#pragma unroll
    for (int v = 0; v < VEC; v++) v0[v] = (double)th[v];
    pair_seg_walk<KP, ROWS, R::REG>(tent, a, b, S, mult, h, k, lane, act, v0, (double)wj, aw, av);
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      if (act && f0 + v < k) {
        float sv[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) sv[t] = st[t][v];
        th[v] = rule.step_v((float)av[v], th[v], sv);
#pragma unroll
        for (int t = 0; t < NT; t++) st[t][v] = sv[t];
      }
    }
    rule_row_st<VEC>(tb.V + ro, full, act, f0, k, th);
#pragma unroll
    for (int t = 0; t < NT; t++) rule_row_st<VEC>(rule.st[t].V + ro, full, act, f0, k, st[t]);
    if (h.k1 && lane == 0) {
      tb.w[(size_t)j * tb.ws] = rule.step_w((float)aw, wj, sw);
#pragma unroll
      for (int t = 0; t < NT; t++) rule.st[t].w[j] = sw[t];
    }
  }
}

}  // namespace fmx

// the owner launch of one batch's segments [s0, s1): what the plain and the rule epochs of a pair driver differ in
template <int ROWS>
inline int launch_pair_owner(fmx_handle h, PairRule r, const TEntry* tent, const uint32_t* seg_head, const uint32_t* seg_feat, uint32_t s0,
                             uint32_t s1, const float* S, const double* mult, const Hyper& hy, hipStream_t st) {
  const int k = h->cfg.num_factor;
  if (r == PAIR_ADAGRAD) {
    const AdagradRule rule{{Tab{h->adapt.nv, h->adapt.nw, h->tb.rs, 1u}}, h->adapt.eta};
    KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_pair_apply_rule<AdagradRule, KP, ROWS>), s1 - s0, st, tent, seg_head, seg_feat, s0, s1, S, mult, h->tb, rule, hy, k));
  } else if (r == PAIR_FTRL) {
    const FtrlState& fs = h->ftrl;
    const FtrlRule rule{{Tab{fs.zv, fs.zw, h->tb.rs, 1u}, Tab{fs.nv, fs.nw, h->tb.rs, 1u}}, FtrlHyper{fs.inv_alpha, fs.beta, fs.l1_w, fs.l1_v, fs.l2_w, fs.l2_v}};
    KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_pair_apply_rule<FtrlRule, KP, ROWS>), s1 - s0, st, tent, seg_head, seg_feat, s0, s1, S, mult, h->tb, rule, hy, k));
  } else {
    KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_pair_apply<KP, ROWS>), s1 - s0, st, tent, seg_head, seg_feat, s0, s1, S, mult, h->tb, hy, k));
  }
  return FMX_OK;
}
