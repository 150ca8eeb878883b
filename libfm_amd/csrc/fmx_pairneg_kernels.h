// fmx_pairneg_kernels.h -- BPR on query x candidate interactions with negatives drawn on the device (include/fmx.h, DESIGN.md
// section 12).  Pair p = t * n_neg + s of an epoch is (x_q ++ x_c+, x_q ++ x_c-) with q = q[t], c+ = c[t], c- = neg[p]: the rule
// is fm_pairSGD on those joined rows (fmx_pair_kernels.h), computed without writing them.
//
// k_neg_sample   one thread per pair: the counter hash, the bounded rejection loop, a binary search in the query's sorted
//                exclusion list; neg[p] and one forced count per workgroup (k_neg_forced_sum adds them).
// k_neg_pick     FMX_NEG_HARDEST: one wavefront per pair scores the first M accepted draws against fmx_topk's tables and keeps the
//                best (section 13); the attempt logic is k_neg_sample's (neg_attempt).
// k_pn_len       entries of pair p in the expanded stream: |x_q| + |x_c+| + |x_c-| (the query's entries ONCE).
// k_pn_keys      that stream keyed by (batch, feature); payload tag 0 = x_c+ (side a), 1 = x_c- (side b), 2 = x_q (both sides).
// k_pn_sums      one wavefront per pair: S_q, S_c+, S_c- gathered once each; d = (b_c+ - b_c-) + sum_f S_q[f] (S_c+[f] - S_c-[f]).
// apply          k_pair_apply<KP, 3> (fmx_pair_kernels.h): one wavefront per (batch, feature) segment; a tag-2 entry adds
//                (S_c+[f] - S_c-[f]) x to gv and nothing to gw (the two sides' x and v x x terms cancel).
// k_pn_eval      one wavefront per pair on a fixed grid, as k_pair_eval.
// JoinSrc        the row source of k_pair_seq (FMX_SGD_SEQUENTIAL): x_a = x_q ++ x_c+, x_b = x_q ++ x_c-.
#pragma once

#include "fmx_pair_kernels.h"

namespace fmx {

constexpr uint32_t NEG_ATTEMPTS = 16;           // FMX_NEG_ATTEMPTS
constexpr uint32_t NEG_MAX_BLOCKS = 2048;

// draw(seed, epoch, p, a): the pattern of unif_hash (fmx_als_kernels.h), an index in [0, C)
__host__ __device__ __forceinline__ uint32_t neg_draw(uint64_t seed, uint64_t epoch, uint64_t p, uint64_t a, uint64_t C) {
  const uint64_t u = mix64(seed ^ (epoch * 0x9E3779B97F4A7C15ULL) ^ (p * 0xD6E8FEB86659FD93ULL + a * 0xA24BAED4963EE407ULL + 0x9FB21C651E98DF25ULL));
#ifdef __HIP_DEVICE_COMPILE__
  return (uint32_t)__umul64hi(u, C);
#else
  return (uint32_t)(((unsigned __int128)u * C) >> 64);
#endif
}

// the interactions on the device: ex_ptr == nullptr: no exclusion lists
struct NegSrc { const uint32_t* q; const uint32_t* c; const uint64_t* ex_ptr; const uint32_t* ex_idx; uint64_t n; uint32_t n_cand; };

// one attempt of pair p: its draw, and whether it is accepted (neither the positive nor in the query's sorted exclusion list
// ex_idx[e0, e1): a lower-bound search).  The ONE copy of the hash and the search: k_neg_sample walks the attempts with it in one
// thread, k_neg_pick evaluates them side by side in 16 lanes.
__device__ __forceinline__ bool neg_attempt(const NegSrc& in, uint64_t seed, uint64_t epoch, uint64_t p, uint32_t a, uint32_t pos,
                                            uint64_t e0, uint64_t e1, uint32_t* draw) {
  const uint32_t d = neg_draw(seed, epoch, p, a, in.n_cand);
  *draw = d;
  if (d == pos) return false;
  if (e1 > e0) {
    uint64_t lo = e0, hi = e1;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (in.ex_idx[mid] < d) lo = mid + 1; else hi = mid;
    }
    if (lo < e1 && in.ex_idx[lo] == d) return false;
  }
  return true;
}

static __global__ void __launch_bounds__(256)
k_neg_sample(const NegSrc in, uint32_t n_neg, uint64_t seed, uint64_t epoch, uint32_t* __restrict__ neg, uint32_t* __restrict__ forced_part) {
  __shared__ uint32_t red[4];
  const uint64_t P = in.n * n_neg;
  uint32_t forced = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t t = p / n_neg;
    const uint32_t pos = in.c[t];
    uint64_t e0 = 0, e1 = 0;
    if (in.ex_ptr) { const uint32_t q = in.q[t]; e0 = in.ex_ptr[q]; e1 = in.ex_ptr[q + 1]; }
    uint32_t d = 0;
    bool ok = false;
    for (uint32_t a = 0; a < NEG_ATTEMPTS && !ok; a++) ok = neg_attempt(in, seed, epoch, p, a, pos, e0, e1, &d);
    neg[p] = d;                                               // all attempts rejected: the last draw as it is
    forced += ok ? 0u : 1u;
  }
  for (int o = 32; o > 0; o >>= 1) forced += (uint32_t)__shfl_xor((int)forced, o);
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = forced;
  __syncthreads();
  if (threadIdx.x == 0) forced_part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
static __global__ void k_neg_forced_sum(const uint32_t* __restrict__ part, uint32_t nblk, uint64_t* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;           // one wavefront (integers: any order gives the same sum)
  uint64_t s = 0;
  for (uint32_t i = threadIdx.x; i < nblk; i += 64) s += part[i];
  for (int o = 32; o > 0; o >>= 1) s += (uint64_t)__shfl_xor((long long)s, o);
  if (threadIdx.x == 0) *out = s;
}

// ---- FMX_NEG_HARDEST: the best-scoring of the first M accepted draws (include/fmx.h) ---------------------
// r(q, d) = b_d + sum_f S_q[f] S_d[f] from fmx_topk's tables (zero-padded [rows][KM] fp32 rows of 64-byte multiples, b [C]).
constexpr uint32_t NEG_PICK_MAX_BLOCKS = 2048;                 // x 4 wavefronts, one forced partial each
struct NegTabs { const float* Sq; const float* Sc; const float* bc; };

// sum over the GL = 4 / 8 / 16 consecutive lanes of a group inside one DPP row: the two quad butterflies of wave_sum_dpp, then the
// half-row and row mirrors.  Every step adds two values that are each other's partner, so all lanes of a group end with the same bits.
template <int GL> __device__ __forceinline__ float group_allsum_dpp(float x) {
  static_assert(GL == 4 || GL == 8 || GL == 16, "a group lies inside one DPP row");
#define FMX_DPP_ADD(ctrl) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, 0xf, 0xf, false))
  FMX_DPP_ADD(0xB1);                                           // quad_perm(1,0,3,2)
  FMX_DPP_ADD(0x4E);                                           // quad_perm(2,3,0,1)
  if constexpr (GL >= 8) FMX_DPP_ADD(0x141);                   // row_half_mirror: the other quad of the 8
  if constexpr (GL >= 16) FMX_DPP_ADD(0x140);                  // row_mirror: the other half of the row
#undef FMX_DPP_ADD
  return x;
}
// the total order of the pick: a number beats NaN, then the higher score, then the earlier attempt
__device__ __forceinline__ bool neg_better(float r1, uint32_t a1, float r2, uint32_t a2) {
  const bool n1 = r1 != r1, n2 = r2 != r2;
  if (n1 != n2) return n2;
  if (!n1 && r1 != r2) return r1 > r2;
  return a1 < a2;
}

// One wavefront per pair.  Lanes 0 .. 15 evaluate the 16 attempts side by side (neg_attempt); the ballot's first M set bits are the
// walk's accepted draws.  For scoring the wavefront is NG = 64 / GL groups of GL = min(16, KM / 4) lanes: a group takes one accepted
// draw at a time (the j-th accepted goes to group j mod NG), lane l of it loads float4 number v GL + l (v < KM / (4 GL)) of the
// candidate's row -- the group reads 256 contiguous bytes per step -- against the query's row, which the lane keeps in registers for
// the whole pair.  Two draws per group are in flight.  Group sums by DPP inside the row, the groups' (score, attempt) by xor
// shuffles under neg_better.  No LDS, no atomics; neg[p] and one forced count per wavefront are the only stores.
template <int KM>
__global__ void __launch_bounds__(256)
k_neg_pick(const NegSrc in, const NegTabs tb, uint32_t n_neg, uint32_t M, uint64_t seed, uint64_t epoch, uint32_t* __restrict__ neg,
           uint32_t* __restrict__ forced_part) {
  static_assert(KM >= 16 && KM % 16 == 0, "rows of 64-byte multiples");
  constexpr int GL = KM >= 64 ? 16 : KM / 4;
  constexpr int NG = 64 / GL;
  constexpr int NV = KM / (4 * GL);
  const uint32_t lane = threadIdx.x & 63u, g = lane / GL, l = lane % GL;
  const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t P = in.n * n_neg;
  uint32_t forced = 0;
  for (uint64_t p = wave0; p < P; p += nwaves) {
    const uint64_t t = p / n_neg;
    const uint32_t rq = in.q[t], pos = in.c[t];
    uint64_t e0 = 0, e1 = 0;
    if (in.ex_ptr) { e0 = in.ex_ptr[rq]; e1 = in.ex_ptr[rq + 1]; }
    float4 qv[NV];
    const float4* Q4 = reinterpret_cast<const float4*>(tb.Sq + (size_t)rq * KM) + l;
#pragma unroll
    for (int v = 0; v < NV; v++) qv[v] = Q4[v * GL];
    uint32_t d = 0;
    bool ok = false;
    if (lane < NEG_ATTEMPTS) ok = neg_attempt(in, seed, epoch, p, lane, pos, e0, e1, &d);
    const uint32_t mask = (uint32_t)__ballot(ok);              // bit a: attempt a accepted
    const uint32_t cnt = min((uint32_t)__popc(mask), M);       // the walk stops after the M-th accepted one
    uint32_t pick = NEG_ATTEMPTS - 1;                          // none accepted: the last draw as it is
    if (cnt == 0) {
      forced++;
    } else {
      const uint32_t a_first = (uint32_t)__ffs(mask) - 1u;
      auto nth = [&](uint32_t j) {                             // the attempt of the j-th accepted draw (j < cnt)
        uint32_t m = mask;
#pragma unroll
        for (uint32_t i = 0; i + 1 < NEG_ATTEMPTS; i++) if (i < j) m &= m - 1u;
        return (uint32_t)__ffs(m) - 1u;
      };
      auto score = [&](uint32_t a) {
        const uint32_t dr = (uint32_t)__shfl((int)d, (int)a);
        const float4* C4 = reinterpret_cast<const float4*>(tb.Sc + (size_t)dr * KM) + l;
        float acc = 0.f;
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const float4 c = C4[v * GL];
          acc = fmaf(qv[v].x, c.x, acc); acc = fmaf(qv[v].y, c.y, acc); acc = fmaf(qv[v].z, c.z, acc); acc = fmaf(qv[v].w, c.w, acc);
        }
        return tb.bc[dr] + group_allsum_dpp<GL>(acc);
      };
      float best = __uint_as_float(0x7FC00000u);               // (NaN, no attempt): loses to every scored draw
      uint32_t best_a = 255u;
      for (uint32_t j0 = 0; j0 < cnt; j0 += 2 * NG) {
        const uint32_t ja = j0 + g, jb = j0 + NG + g;
        const uint32_t aa = ja < cnt ? nth(ja) : a_first;      // (a lane without a draw of its own scores the first one again and drops it)
        if (j0 + NG < cnt) {                                   // wave-uniform: both rows' loads are issued before either is used
          const uint32_t ab = jb < cnt ? nth(jb) : a_first;
          const float ra = score(aa), rb = score(ab);
          if (ja < cnt && neg_better(ra, aa, best, best_a)) { best = ra; best_a = aa; }
          if (jb < cnt && neg_better(rb, ab, best, best_a)) { best = rb; best_a = ab; }
        } else {
          const float ra = score(aa);
          if (ja < cnt && neg_better(ra, aa, best, best_a)) { best = ra; best_a = aa; }
        }
      }
#pragma unroll
      for (int o = GL; o < 64; o <<= 1) {
        const float r2 = __shfl_xor(best, o);
        const uint32_t a2 = (uint32_t)__shfl_xor((int)best_a, o);
        if (neg_better(r2, a2, best, best_a)) { best = r2; best_a = a2; }
      }
      pick = best_a;
    }
    const uint32_t dn = (uint32_t)__shfl((int)d, (int)pick);
    if (lane == 0) neg[p] = dn;
  }
  if (lane == 0) forced_part[blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = forced;
}

// the two slots and the pairs of one epoch
struct JoinSrc {
  const Entry* qent; const uint64_t* qrp; const Entry* cent; const uint64_t* crp;
  const uint32_t* q; const uint32_t* c; const uint32_t* neg; uint32_t n_neg;
  struct Rows { uint64_t q0, p0, n0; uint32_t lq, lp, ma, m; };   // x_a = x_q ++ x_c+ (ma entries), x_b = x_q ++ x_c-
  __device__ __forceinline__ Rows rows(uint64_t p) const {
    const uint64_t t = p / n_neg;
    const uint32_t rq = q[t], rp = c[t], rn = neg[p];
    Rows r;
    r.q0 = qrp[rq]; r.p0 = crp[rp]; r.n0 = crp[rn];
    r.lq = (uint32_t)(qrp[rq + 1] - r.q0); r.lp = (uint32_t)(crp[rp + 1] - r.p0);
    r.ma = r.lq + r.lp; r.m = r.ma + r.lq + (uint32_t)(crp[rn + 1] - r.n0);
    return r;
  }
  __device__ __forceinline__ Entry at(const Rows& r, uint32_t i) const {
    if (i < r.lq) return qent[r.q0 + i];
    if (i < r.ma) return cent[r.p0 + (i - r.lq)];
    i -= r.ma;
    return (i < r.lq) ? qent[r.q0 + i] : cent[r.n0 + (i - r.lq)];
  }
};

static __global__ void __launch_bounds__(256)
k_pn_len(const JoinSrc in, uint64_t P, uint64_t* __restrict__ len) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t t = p / in.n_neg;
    const uint32_t rq = in.q[t], rp = in.c[t], rn = in.neg[p];
    len[p] = (in.qrp[rq + 1] - in.qrp[rq]) + (in.crp[rp + 1] - in.crp[rp]) + (in.crp[rn + 1] - in.crp[rn]);
  }
}

// ---- FMX_SGD_MINIBATCH ----------------------------------------------------------------------------------------------------
// sort keys (batch << fbits) | feature, payload (value bits << 32) | (pair in batch << 2 | tag) == TEntry in memory.  The radix sort
// is stable, so a segment lists its entries in pair order; inside a pair x_q, then x_c+, then x_c-, row order inside a row.
constexpr uint32_t PN_TAG_A = 0, PN_TAG_B = 1, PN_TAG_BOTH = 2;
static __global__ void __launch_bounds__(256)
k_pn_keys(const JoinSrc in, const uint64_t* __restrict__ off, uint64_t P, uint32_t B, uint32_t fbits, uint64_t* __restrict__ keys,
          uint64_t* __restrict__ vals) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t p = wave0; p < P; p += nwaves) {
    const uint64_t hi = (p / B) << fbits;
    const uint32_t pb_ = (uint32_t)(p % B) << 2;
    const uint64_t t = p / in.n_neg;
    uint64_t base = off[p];
    for (uint32_t part = 0; part < 3; part++) {
      const Entry* ent = part ? in.cent : in.qent;
      const uint64_t* rp = part ? in.crp : in.qrp;
      const uint32_t r = part == 0 ? in.q[t] : part == 1 ? in.c[t] : in.neg[p];
      const uint32_t tag = part == 0 ? PN_TAG_BOTH : part == 1 ? PN_TAG_A : PN_TAG_B;
      const uint64_t a = rp[r];
      const uint32_t m = (uint32_t)(rp[r + 1] - a);
      for (uint32_t i = lane; i < m; i += 64) {
        const Entry e = ent[a + i];
        keys[base + i] = hi | e.id;
        vals[base + i] = ((uint64_t)__float_as_uint(e.value) << 32) | (pb_ | tag);
      }
      base += m;
    }
  }
}

// d = y_a - y_b of the joined rows from the three rows' sums (a_q and w0 cancel); leaves S_q + S_c+, S_q + S_c-, S_c+ - S_c- of
// this lane's factors in sa / sb / sd (fp64)
template <int KP>
__device__ __forceinline__ double pn_diff(const JoinSrc& in, uint64_t p, const Tab& tb, int k, int k1, double (&sa)[Map<KP>::VEC],
                                          double (&sb)[Map<KP>::VEC], double (&sd)[Map<KP>::VEC]) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR;
  const uint32_t g = (threadIdx.x & 63u) / LPR;
  const uint64_t t = p / in.n_neg;
  const uint32_t rq = in.q[t], rp = in.c[t], rn = in.neg[p];
  const uint64_t q0 = in.qrp[rq], p0 = in.crp[rp], n0 = in.crp[rn];
  double sq[VEC];
  pair_row_sums<KP>(in.qent, q0, (uint32_t)(in.qrp[rq + 1] - q0), tb, k, sq);
  const double bp = pair_side<KP>(in.cent, p0, (uint32_t)(in.crp[rp + 1] - p0), tb, k, k1, sa);
  const double bn = pair_side<KP>(in.cent, n0, (uint32_t)(in.crp[rn + 1] - n0), tb, k, k1, sb);
  double cross = 0.0;
#pragma unroll
  for (int v = 0; v < VEC; v++) {
    sd[v] = sa[v] - sb[v];
    if (g == 0) cross += sq[v] * sd[v];
    sa[v] += sq[v]; sb[v] += sq[v];
  }
  return (bp - bn) + wave_sum_d(cross);
}

// S: [nb][3][KP] floats (S_a, S_b, S_c+ - S_c-), mult: [nb] doubles
template <int KP>
__global__ void __launch_bounds__(256)
k_pn_sums(const JoinSrc in, uint64_t p0, uint32_t nb, const Tab tb, int k, int k1, float* __restrict__ S, double* __restrict__ mult) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR;
  const uint32_t lane = threadIdx.x & 63u, g = lane / LPR, f = lane % LPR;
  const uint32_t wave0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t e = wave0; e < nb; e += nwaves) {
    double sa[VEC], sb[VEC], sd[VEC];
    const double d = pn_diff<KP>(in, p0 + e, tb, k, k1, sa, sb, sd);
    if (g == 0) {
      float* Sr = S + (size_t)e * 3 * KP + f * VEC;
#pragma unroll
      for (int v = 0; v < VEC; v++) { Sr[v] = (float)sa[v]; Sr[KP + v] = (float)sb[v]; Sr[2 * KP + v] = (float)sd[v]; }
    }
    if (lane == 0) mult[e] = pair_mult(d);
  }
}

// ---- evaluate: the fixed grid and block partials of k_pair_eval (k_pair_eval_final sums them in order) ---------------------
template <int KP>
__global__ void __launch_bounds__(256)
k_pn_eval(const JoinSrc in, uint64_t P, const Tab tb, int k, int k1, double* __restrict__ part) {
  constexpr int VEC = Map<KP>::VEC;
  __shared__ double red[2][4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + w;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  double cnt = 0.0, loss = 0.0;
  for (uint64_t p = wave0; p < P; p += nwaves) {
    double sa[VEC], sb[VEC], sd[VEC];
    const double d = pn_diff<KP>(in, p, tb, k, k1, sa, sb, sd);
    cnt += (d > 0.0) ? 1.0 : 0.0;
    loss += pair_loss(d);
  }
  if (lane == 0) { red[0][w] = cnt; red[1][w] = loss; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double c = 0.0, l = 0.0;
    for (int i = 0; i < 4; i++) { c += red[0][i]; l += red[1][i]; }
    part[2 * blockIdx.x] = c; part[2 * blockIdx.x + 1] = l;
  }
}

}  // namespace fmx
