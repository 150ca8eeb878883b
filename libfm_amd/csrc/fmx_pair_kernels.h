// fmx_pair_kernels.h -- pairwise ranking (BPR) around fm_pairSGD (/root/reference/src/fm_core/fm_sgd.h:53-126), restated.
//
// The learner (include/fmx.h): per pair (a, b), "row a preferred to row b",
//   d = y_a - y_b (fm_model.h:105-127 on both rows; w0 cancels), mult = -(1 - sigmoid(d)), then fm_pairSGD:
//   w0 -= reg0 * w0 (no learning rate); every DISTINCT feature j of the pair once, with one regularisation term:
//     w_j  -= lr * (mult * (sum of j's values in x_a - sum in x_b) + regw * w_j)
//     v_jf -= lr * (mult * (sum over x_a of S_a(f) x - v_jf x x  -  sum over x_b of S_b(f) x - v_jf x x) + regv * v_jf)
//   all from the parameters at the start of the pair.
//
// k_pair_seq    FMX_SGD_SEQUENTIAL: ONE workgroup walks the pairs in order (the parity instrument, like k_sequential_wg).
// k_pair_keys   FMX_SGD_MINIBATCH bucketing: the pair-expanded entry stream keyed by (batch, feature) for the radix sort.
// k_pair_sums   one wavefront per pair: both rows' factor sums (batch-start parameters) and the multiplier.
// k_pair_apply  one wavefront per (batch, feature) segment: the gradient summed in pair order, one regularisation term per
//               distinct pair, the feature's row written once (no atomics).
// k_pair_eval   one wavefront per pair: accuracy count and -ln sigmoid(d), block partials; k_pair_eval_final sums them in order.
#pragma once

#include "fmx_kernels.h"

namespace fmx {

// parameter access of the sequential kernel: agent-scope relaxed atomics bypass the per-CU L1, so the next pair reads what this
// pair wrote (the stores are drained by __threadfence before the workgroup barrier that ends the pair)
__device__ __forceinline__ float pair_ld(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pair_st(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one entry of x_a ++ x_b: nxt = the next entry of the same feature (-1: none), first = no earlier entry of the feature
// (the owner that updates it: grad_visited, fm_sgd.h:73-88, :106-121)
struct PairEnt { uint32_t id; float x; int32_t nxt; uint32_t first; };

constexpr int      PAIR_SEQ_THREADS = 256;
constexpr uint32_t PAIR_SEQ_LDS_ENT = 2048;       // pairs up to this many entries are merged in LDS, longer ones in a global buffer
constexpr int      PAIR_MAX_K = 1024;

// -ln sigmoid(d) without overflow
__device__ __forceinline__ double pair_loss(double d) { return d >= 0.0 ? log1p(exp(-d)) : -d + log1p(exp(d)); }
__device__ __forceinline__ double pair_mult(double d) { return -(1.0 - 1.0 / (1.0 + exp(-d))); }   // util.h:52

// where the sequential kernel takes a pair's rows from: Rows = what is read once per pair, at(r, i) = entry i of x_a ++ x_b
struct PairSlotSrc {                          // rows pa[t], pb[t] of one slot
  const Entry* ent; const uint64_t* row_ptr; const uint32_t* pa; const uint32_t* pb;
  struct Rows { uint64_t a0, b0; uint32_t ma, m; };
  __device__ __forceinline__ Rows rows(uint64_t t) const {
    const uint32_t ra = pa[t], rb = pb[t];
    Rows r;
    r.a0 = row_ptr[ra]; r.b0 = row_ptr[rb];
    r.ma = (uint32_t)(row_ptr[ra + 1] - r.a0); r.m = r.ma + (uint32_t)(row_ptr[rb + 1] - r.b0);
    return r;
  }
  __device__ __forceinline__ Entry at(const Rows& r, uint32_t i) const { return (i < r.ma) ? ent[r.a0 + i] : ent[r.b0 + (i - r.ma)]; }
};

template <class Src>
__global__ void __launch_bounds__(PAIR_SEQ_THREADS)
k_pair_seq(const Src src, uint64_t n_pairs, const Tab tb, Hyper h, int k, double* w0_ptr, PairEnt* gbuf, uint32_t use_lds) {
  __shared__ PairEnt lbuf[PAIR_SEQ_LDS_ENT];
  __shared__ double s_a[PAIR_MAX_K], s_b[PAIR_MAX_K];
  __shared__ double red[PAIR_SEQ_THREADS / 64];
  PairEnt* E = use_lds ? lbuf : gbuf;
  const uint32_t tid = threadIdx.x;
  double w0 = (h.k0 && tid == 0) ? *w0_ptr : 0.0;
  for (uint64_t t = 0; t < n_pairs; t++) {
    const typename Src::Rows pr = src.rows(t);
    const uint32_t ma = pr.ma, m = pr.m;
    for (uint32_t i = tid; i < m; i += PAIR_SEQ_THREADS) {
      const Entry e = src.at(pr, i);
      E[i].id = e.id; E[i].x = e.value;
    }
    __syncthreads();
    // grad_visited: the first entry of every feature owns it; the chain nxt visits its entries in x_a ++ x_b order (fm_sgd.h:67-72)
    for (uint32_t i = tid; i < m; i += PAIR_SEQ_THREADS) {
      const uint32_t id = E[i].id;
      uint32_t first = 1u;
      for (uint32_t q = 0; q < i; q++) if (E[q].id == id) { first = 0u; break; }
      int32_t nx = -1;
      for (uint32_t q = i + 1; q < m; q++) if (E[q].id == id) { nx = (int32_t)q; break; }
      E[i].nxt = nx; E[i].first = first;
    }
    // both predictions from the parameters at the start of the pair (fm_model.h:105-127), fp64
    double part = 0.0;
    for (int f = (int)tid; f < k; f += PAIR_SEQ_THREADS) {
      double sa = 0.0, qa = 0.0, sb = 0.0, qb = 0.0;
      for (uint32_t i = 0; i < ma; i++) {
        const double d = (double)pair_ld(tb.V + (size_t)E[i].id * tb.rs + f) * (double)E[i].x;
        sa += d; qa += d * d;
      }
      for (uint32_t i = ma; i < m; i++) {
        const double d = (double)pair_ld(tb.V + (size_t)E[i].id * tb.rs + f) * (double)E[i].x;
        sb += d; qb += d * d;
      }
      s_a[f] = sa; s_b[f] = sb;
      part += 0.5 * (sa * sa - qa) - 0.5 * (sb * sb - qb);
    }
    if (h.k1)
      for (uint32_t i = tid; i < m; i += PAIR_SEQ_THREADS) {
        const double l = (double)pair_ld(tb.w + (size_t)E[i].id * tb.ws) * (double)E[i].x;
        part += (i < ma) ? l : -l;
      }
    part = wave_sum_d(part);
    if ((tid & 63u) == 0) red[tid >> 6] = part;
    __syncthreads();                                           // (also publishes E's chains and s_a / s_b)
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < PAIR_SEQ_THREADS / 64; i++) d += red[i];
    const double mult = pair_mult(d);
    if (h.k0 && tid == 0) w0 = __dsub_rn(w0, __dmul_rn(h.reg0_d, w0));          // fm_sgd.h:56, no learning rate
    if (h.k1)                                                                  // fm_sgd.h:58-89
      for (uint32_t i = tid; i < m; i += PAIR_SEQ_THREADS) {
        if (!E[i].first) continue;
        double g = 0.0;
        for (int32_t q = (int32_t)i; q >= 0; q = E[q].nxt) g = ((uint32_t)q < ma) ? g + (double)E[q].x : g - (double)E[q].x;
        float* pw = tb.w + (size_t)E[i].id * tb.ws;
        const double wv = (double)pair_ld(pw);
        pair_st(pw, (float)(wv - h.lr_d * (mult * g + h.regw_d * wv)));
      }
    // fm_sgd.h:91-123: (entry, factor) flattened, factors fastest (one feature's row is one coalesced segment); a factor's gradient
    // reads v(f, j) at the start of the pair -- nothing else touches (j, f) here
    const uint64_t mk = (uint64_t)m * (uint64_t)k;
    for (uint64_t idx = tid; idx < mk; idx += PAIR_SEQ_THREADS) {
      const uint32_t i = (uint32_t)(idx / (uint64_t)k);
      const int f = (int)(idx - (uint64_t)i * (uint64_t)k);
      if (!E[i].first) continue;
      float* pv = tb.V + (size_t)E[i].id * tb.rs + f;
      const double v0 = (double)pair_ld(pv);
      double g = 0.0;
      for (int32_t q = (int32_t)i; q >= 0; q = E[q].nxt) {
        const double x = (double)E[q].x;
        if ((uint32_t)q < ma) g += s_a[f] * x - v0 * x * x;
        else                  g -= s_b[f] * x - v0 * x * x;
      }
      pair_st(pv, (float)(v0 - h.lr_d * (mult * g + h.regv_d * v0)));
    }
    __threadfence();                                           // this pair's stores are visible before the next pair reads
    __syncthreads();
  }
  if (h.k0 && tid == 0) *w0_ptr = w0;
}

// ---- FMX_SGD_MINIBATCH ----------------------------------------------------------------------------------------------------
// sort keys (batch << fbits) | feature, payload (value bits << 32) | (pair in batch << 1 | side) == TEntry in memory.  The radix
// sort is stable, so a segment lists its entries in pair order, x_a before x_b, row order inside a row.
static __global__ void __launch_bounds__(256)
k_pair_keys(const Entry* __restrict__ ent, const uint64_t* __restrict__ row_ptr, const uint32_t* __restrict__ pa,
            const uint32_t* __restrict__ pb, const uint64_t* __restrict__ off, uint64_t n_pairs, uint32_t B, uint32_t fbits,
            uint64_t* __restrict__ keys, uint64_t* __restrict__ vals) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t t = wave0; t < n_pairs; t += nwaves) {
    const uint64_t hi = (t / B) << fbits;
    const uint32_t tb_ = (uint32_t)(t % B) << 1;
    uint64_t base = off[t];
    for (uint32_t side = 0; side < 2; side++) {
      const uint32_t r = side ? pb[t] : pa[t];
      const uint64_t a = row_ptr[r];
      const uint32_t m = (uint32_t)(row_ptr[r + 1] - a);
      for (uint32_t i = lane; i < m; i += 64) {
        const Entry e = ent[a + i];
        keys[base + i] = hi | e.id;
        vals[base + i] = ((uint64_t)__float_as_uint(e.value) << 32) | (tb_ | side);
      }
      base += m;
    }
  }
}
// the feature of every segment
static __global__ void __launch_bounds__(256)
k_pair_seg_feat(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head, uint32_t nseg, uint32_t fbits, uint32_t* __restrict__ feat) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += gridDim.x * blockDim.x)
    feat[s] = (uint32_t)(keys[head[s]] & ((1ull << fbits) - 1ull));
}
// first segment of every batch (b = 0 .. n_batches): lower bound of b over the segments' batches
static __global__ void __launch_bounds__(256)
k_pair_batch_seg(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head, uint32_t nseg, uint32_t fbits,
                 uint32_t n_batches, uint32_t* __restrict__ batch_seg) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b <= n_batches; b += gridDim.x * blockDim.x) {
    uint32_t lo = 0, hi = nseg;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if ((uint64_t)(keys[head[mid]] >> fbits) < (uint64_t)b) lo = mid + 1; else hi = mid;
    }
    batch_seg[b] = lo;
  }
}

// one side of a pair on one wavefront: lane (g, f) of Map<KP> owns factors f*VEC .. f*VEC+VEC-1 of the entries i == g (mod EPI).
// Returns lin - 0.5 * sum of squares + 0.5 * sum_f S_f^2 (fp64, wave-uniform) and leaves the full S in sum[] of every lane.
template <int KP>
__device__ __forceinline__ double pair_side(const Entry* __restrict__ ent, uint64_t a, uint32_t m, const Tab& tb, int k, int k1, double (&sum)[Map<KP>::VEC]) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR, EPI = Map<KP>::EPI;
  const uint32_t lane = threadIdx.x & 63u, g = lane / LPR, f = lane % LPR;
  double sq = 0.0, lin = 0.0;
#pragma unroll
  for (int v = 0; v < VEC; v++) sum[v] = 0.0;
  for (uint32_t i = g; i < m; i += EPI) {
    const Entry e = ent[a + i];
    const double x = (double)e.value;
    const float* row = tb.V + (size_t)e.id * tb.rs;
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      const int ff = (int)(f * VEC + v);
      const double d = (ff < k) ? (double)row[ff] * x : 0.0;
      sum[v] += d; sq += d * d;
    }
    if (k1 && f == 0) lin += (double)tb.w[(size_t)e.id * tb.ws] * x;
  }
#pragma unroll
  for (int v = 0; v < VEC; v++)
    for (int o = LPR; o < 64; o <<= 1) sum[v] += __shfl_xor(sum[v], o);
  double s2 = 0.0;
  if (g == 0) {
#pragma unroll
    for (int v = 0; v < VEC; v++) s2 += sum[v] * sum[v];
  }
  return wave_sum_d(lin - 0.5 * sq + 0.5 * s2);
}

// the factor sums of one row alone (what pair_side leaves in sum[], without its scalar)
template <int KP>
__device__ __forceinline__ void pair_row_sums(const Entry* __restrict__ ent, uint64_t a, uint32_t m, const Tab& tb, int k, double (&sum)[Map<KP>::VEC]) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR, EPI = Map<KP>::EPI;
  const uint32_t lane = threadIdx.x & 63u, g = lane / LPR, f = lane % LPR;
#pragma unroll
  for (int v = 0; v < VEC; v++) sum[v] = 0.0;
  for (uint32_t i = g; i < m; i += EPI) {
    const Entry e = ent[a + i];
    const double x = (double)e.value;
    const float* row = tb.V + (size_t)e.id * tb.rs;
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      const int ff = (int)(f * VEC + v);
      sum[v] += (ff < k) ? (double)row[ff] * x : 0.0;
    }
  }
#pragma unroll
  for (int v = 0; v < VEC; v++)
    for (int o = LPR; o < 64; o <<= 1) sum[v] += __shfl_xor(sum[v], o);
}

// S: [nb][2][KP] floats (x_a's sums, then x_b's), mult: [nb] doubles
template <int KP>
__global__ void __launch_bounds__(256)
k_pair_sums(const Entry* __restrict__ ent, const uint64_t* __restrict__ row_ptr, const uint32_t* __restrict__ pa,
            const uint32_t* __restrict__ pb, uint64_t t0, uint32_t nb, const Tab tb, int k, int k1, float* __restrict__ S,
            double* __restrict__ mult) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR;
  const uint32_t lane = threadIdx.x & 63u, g = lane / LPR, f = lane % LPR;
  const uint32_t wave0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t e = wave0; e < nb; e += nwaves) {
    double d = 0.0;
    for (uint32_t side = 0; side < 2; side++) {
      const uint32_t r = side ? pb[t0 + e] : pa[t0 + e];
      const uint64_t a = row_ptr[r];
      double sum[VEC];
      const double y = pair_side<KP>(ent, a, (uint32_t)(row_ptr[r + 1] - a), tb, k, k1, sum);
      d = side ? d - y : y;
      if (g == 0) {
#pragma unroll
        for (int v = 0; v < VEC; v++) S[((size_t)e * 2 + side) * KP + f * VEC + v] = (float)sum[v];
      }
    }
    if (lane == 0) mult[e] = pair_mult(d);
  }
}

// owner apply: segment s = every entry of one feature j in one batch, in pair order.  Per pair the gradient of its entries, then
// acc += mult_t * grad_t + reg * theta_j(start) (one regularisation term per distinct pair); theta_j -= lr * acc.
// ROWS = sums rows per pair in S and tags an entry can carry: 2 = {x_a, x_b} (payload pair << 1 | tag); 3 adds tag 2, an entry that
// is in BOTH rows (fmx_pairneg_kernels.h: the query's entries, once): S row 2 holds S_a - S_b, so it adds S[2][f] x to gv and
// nothing to gw -- the two sides' x and v x x terms cancel (payload pair << 2 | tag).
template <int KP, int ROWS = 2>
__global__ void __launch_bounds__(256)
k_pair_apply(const TEntry* __restrict__ tent, const uint32_t* __restrict__ seg_head, const uint32_t* __restrict__ seg_feat,
             uint32_t s0, uint32_t s1, const float* __restrict__ S, const double* __restrict__ mult, const Tab tb, Hyper h, int k) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR;
  constexpr uint32_t TAG_BITS = ROWS == 2 ? 1u : 2u, TAG_MASK = (1u << TAG_BITS) - 1u;
  static_assert(ROWS == 2 || ROWS == 3, "tags: x_a, x_b and optionally both");
  const uint32_t lane = threadIdx.x & 63u;
  const bool act = lane < (uint32_t)LPR;
  const uint32_t wave0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t s = s0 + wave0; s < s1; s += nwaves) {
    const uint32_t j = seg_feat[s], a = seg_head[s], b = seg_head[s + 1];
    float* row = tb.V + (size_t)j * tb.rs;
    double v0[VEC], gv[VEC], av[VEC];
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      const int ff = (int)(lane * VEC + v);
      v0[v] = (act && ff < k) ? (double)row[ff] : 0.0;
      gv[v] = 0.0; av[v] = 0.0;
    }
    const double w0j = h.k1 ? (double)tb.w[(size_t)j * tb.ws] : 0.0;
    double gw = 0.0, aw = 0.0;
    uint32_t cur = tent[a].e >> TAG_BITS;
    for (uint32_t i = a; i < b; i++) {
      const TEntry te = tent[i];
      const uint32_t t = te.e >> TAG_BITS, side = te.e & TAG_MASK;
      if (t != cur) {                                        // the previous pair's gradient is complete
        const double mt = mult[cur];
        aw += mt * gw + h.regw_d * w0j;
#pragma unroll
        for (int v = 0; v < VEC; v++) { av[v] += mt * gv[v] + h.regv_d * v0[v]; gv[v] = 0.0; }
        gw = 0.0; cur = t;
      }
      const double x = (double)te.x;
      if (ROWS == 2 || side < 2u) gw = side ? gw - x : gw + x;
      const float* Sr = S + ((size_t)t * ROWS + side) * KP;
      const double xs = (ROWS == 3 && side == 2u) ? 0.0 : x;   // (v x x as (v x) x, the order it always had)
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
      aw += mt * gw + h.regw_d * w0j;
#pragma unroll
      for (int v = 0; v < VEC; v++) av[v] += mt * gv[v] + h.regv_d * v0[v];
    }
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      const int ff = (int)(lane * VEC + v);
      if (act && ff < k) row[ff] = (float)(v0[v] - h.lr_d * av[v]);
    }
    if (h.k1 && lane == 0) tb.w[(size_t)j * tb.ws] = (float)(w0j - h.lr_d * aw);
  }
}

// ---- evaluate -------------------------------------------------------------------------------------------------------------
// a FIXED grid (no occupancy-dependent size): wave w of block blk takes pairs w, w + nwaves, ...; part[blk] = {pairs with d > 0,
// sum of -ln sigmoid(d)} summed wave by wave in order
constexpr uint32_t PAIR_EVAL_BLOCKS = 1024;
template <int KP>
__global__ void __launch_bounds__(256)
k_pair_eval(const Entry* __restrict__ ent, const uint64_t* __restrict__ row_ptr, const uint32_t* __restrict__ pa,
            const uint32_t* __restrict__ pb, uint64_t n_pairs, const Tab tb, int k, int k1, double* __restrict__ part) {
  constexpr int VEC = Map<KP>::VEC;
  __shared__ double red[2][4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + w;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  double cnt = 0.0, loss = 0.0;
  for (uint64_t t = wave0; t < n_pairs; t += nwaves) {
    double sum[VEC];
    const uint64_t a = row_ptr[pa[t]], b = row_ptr[pb[t]];
    const double ya = pair_side<KP>(ent, a, (uint32_t)(row_ptr[pa[t] + 1] - a), tb, k, k1, sum);
    const double yb = pair_side<KP>(ent, b, (uint32_t)(row_ptr[pb[t] + 1] - b), tb, k, k1, sum);
    const double d = ya - yb;
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
static __global__ void k_pair_eval_final(const double* __restrict__ part, uint32_t nblk, double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double c = 0.0, l = 0.0;
    for (uint32_t i = 0; i < nblk; i++) { c += part[2 * i]; l += part[2 * i + 1]; }
    out[0] = c; out[1] = l;
  }
}

}  // namespace fmx
