// fmx_topk_kernels.h -- top-K retrieval of candidate rows per query row (fmx_topk).
//
// score(q, c) = a_q + b_c + sum_f S_q[f] S_c[f] is fm_model::predict (fm_model.h:105-127) of the joined row x_q ++ x_c; the factor
// sums S come from k_rowsums (sgd_partial_rows), k_topk_prep turns them into zero-padded [rows][KM] tables and the scalars a / b.
// The dot products run on the f32 matrix units (v_mfma_f32_16x16x4_f32: exact f32 products, one rounding per fma, a fixed k order),
// so a score does not depend on the tile or split that computes it.
//
// Order of the lists: (s1, c1) is BETTER than (s2, c2) when s1 > s2, or s1 == s2 and c1 < c2.  A NaN score is better than nothing;
// the padding entry (-inf, UINT32_MAX) is worse than every eligible candidate.  All candidates of one query are distinct, so every
// entry of a merged list has one rank: merges place an entry at (its index in its own list) + (entries of the other list better
// than it), found by binary search, with no sort network.
#pragma once

#include "fmx_kernels.h"

namespace fmx {

constexpr uint32_t TOPK_QB = 64;           // queries per workgroup: 4 wavefronts x 16 (one MFMA row block each)
constexpr uint32_t TOPK_CT = 64;           // candidates per tile: 4 MFMA column blocks of 16
constexpr uint32_t TOPK_NONE = 0xFFFFFFFFu;

struct TopkEnt { float s; uint32_t c; };

__device__ __forceinline__ bool tk_better(float s1, uint32_t c1, float s2, uint32_t c2) {
  return s1 > s2 || (s1 == s2 && c1 < c2);
}
// entries of the sorted list X[0, L) that are better than (s, c): the length of its prefix of better entries
__device__ __forceinline__ uint32_t tk_count_better(const TopkEnt* X, uint32_t L, float s, uint32_t c) {
  uint32_t lo = 0, hi = L;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const TopkEnt e = X[mid];
    if (tk_better(e.s, e.c, s, c)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// raw partial sums of n rows (S [n][KP], c [n] = k1 lin - 1/2 sum of squares) -> out [n][KM] (factors >= k zeroed) and
// scal[r] = (k0 w0) + (c_r + 1/2 sum_f S_rf^2).  One wavefront per row.
__global__ void __launch_bounds__(256)
k_topk_prep(const float* __restrict__ S, const float* __restrict__ c, uint32_t n, int KP, int k, int KM, int k0,
            const double* __restrict__ w0_ptr, float* __restrict__ out, float* __restrict__ scal) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  const float w0 = k0 ? (float)(*w0_ptr) : 0.f;
  for (uint32_t r = wave0; r < n; r += nwaves) {
    float half_sq = 0.f;
    for (int f = (int)lane; f < KM; f += 64) {
      const float v = (f < k && f < KP) ? S[(size_t)r * KP + f] : 0.f;
      out[(size_t)r * KM + f] = v;
      half_sq = fmaf(0.5f * v, v, half_sq);
    }
    half_sq = wave_sum(half_sq);
    if (lane == 0) scal[r] = w0 + (c[r] + half_sq);
  }
}

// Score and select.  Workgroup (blockIdx.x, blockIdx.y) = TOPK_QB queries x candidate split blockIdx.y ([c_begin, c_end), a
// multiple of TOPK_CT long).  Wavefront w owns queries 16w .. 16w + 15 of the block: its 16 x 64 tile is four 16x16 MFMA blocks,
// accumulated over the factors 16 at a time.  Lane l brings factor 16 ch + 4 (l >> 4) + t of query row l & 15 (A) and of candidate
// row l & 15 of each column block (B) to step t: both operands see the same k in every step, so the chain covers every factor once.
// C/D: lane l, register r = query 4 (l >> 4) + r, candidate l & 15.
// The epilogue keeps what beats the query's running K-th entry (thr) and is not excluded in a per-query LDS buffer; when a buffer
// may overflow with the next tile (or after the last tile) the block merges every buffer into the query's sorted list in global
// memory (two halves, ping-pong: par[q] says which holds the current list).
//   lists: [2][splits][nq_pad][K]; lens_out: [splits][nq_pad] valid entries; the list ends in half 0.
template <int KM, int BUF>
__global__ void __launch_bounds__(256)
k_topk_score(const float* __restrict__ Sq, const float* __restrict__ aq, uint32_t nq, uint32_t nq_pad,
             const float* __restrict__ Sc, const float* __restrict__ bc, uint32_t n_cand, uint32_t split_len, uint32_t splits,
             const uint64_t* __restrict__ ex_ptr, const uint32_t* __restrict__ ex_idx, uint32_t K,
             TopkEnt* __restrict__ lists, uint32_t* __restrict__ lens_out) {
  static_assert(KM % 16 == 0 && BUF > (int)TOPK_CT, "tile shape");
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  extern __shared__ __align__(16) unsigned char tk_lds[];
  TopkEnt* buf = reinterpret_cast<TopkEnt*>(tk_lds);                 // [QB][BUF] survivors of the tiles since the last merge
  TopkEnt* srt = buf + TOPK_QB * BUF;                                // [4][BUF] one wavefront's survivors, sorted
  TopkEnt* thr = srt + 4 * BUF;                                      // [QB] K-th entry of the query's list (padding while shorter)
  uint32_t* cnt = reinterpret_cast<uint32_t*>(thr + TOPK_QB);        // [QB]
  uint32_t* len = cnt + TOPK_QB;                                     // [QB]
  uint32_t* par = len + TOPK_QB;                                     // [QB]
  uint32_t* flag = par + TOPK_QB;                                    // merge requested

  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t q_blk = blockIdx.x * TOPK_QB;
  const uint32_t split = blockIdx.y;
  const uint64_t cb = (uint64_t)split * split_len;
  const uint32_t c_begin = (uint32_t)min<uint64_t>(cb, n_cand), c_end = (uint32_t)min<uint64_t>(cb + split_len, n_cand);
  const size_t half = (size_t)splits * nq_pad * K;
  TopkEnt* my_lists = lists + (size_t)split * nq_pad * K;
  for (uint32_t t = threadIdx.x; t < TOPK_QB; t += blockDim.x) {
    cnt[t] = 0; len[t] = 0; par[t] = 0; thr[t].s = -INFINITY; thr[t].c = TOPK_NONE;
  }
  if (threadIdx.x == 0) *flag = 0;
  __syncthreads();

  constexpr int NCH = KM / 16;
  constexpr bool AREG = KM <= 128;                                   // the wavefront's query rows stay in registers
  const uint32_t arow = q_blk + 16 * w + (lane & 15u);
  const uint32_t kq = 4 * (lane >> 4);
  const float4* Aq = reinterpret_cast<const float4*>(Sq + (size_t)arow * KM + kq);
  float4 areg[AREG ? NCH : 1];
  if constexpr (AREG) {
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) areg[ch] = Aq[ch * 4];
  }
  const uint32_t lq0 = 16 * w + 4 * (lane >> 4);                    // block-local query of register 0
  float a_ep[4];
#pragma unroll
  for (int r = 0; r < 4; r++) a_ep[r] = aq[q_blk + lq0 + r];

  for (uint32_t c0 = c_begin; c0 < c_end; c0 += TOPK_CT) {
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float4* Bc = reinterpret_cast<const float4*>(Sc + (size_t)(c0 + (lane & 15u)) * KM + kq);
#pragma unroll 8
    for (int ch = 0; ch < NCH; ch++) {
      float4 a;
      if constexpr (AREG) a = areg[ch]; else a = Aq[ch * 4];
      float4 b[4];
#pragma unroll
      for (int j = 0; j < 4; j++) b[j] = Bc[(size_t)j * 16 * (KM / 4) + ch * 4];
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[j].x, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[j].y, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[j].z, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[j].w, acc[j], 0, 0, 0);
    }
    // epilogue: survivors into the buffers
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t c = c0 + 16 * j + (lane & 15u);
      const float bj = bc[c];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t lq = lq0 + r, q = q_blk + lq;
        const float s = (a_ep[r] + bj) + acc[j][r];
        if (c >= c_end || q >= nq) continue;
        const TopkEnt t = thr[lq];
        if (!tk_better(s, c, t.s, t.c)) continue;
        if (ex_ptr) {                                                // binary search in the query's sorted exclusion list
          uint64_t lo = ex_ptr[q], hi = ex_ptr[q + 1];
          while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (ex_idx[mid] < c) lo = mid + 1; else hi = mid; }
          if (lo < ex_ptr[q + 1] && ex_idx[lo] == c) continue;
        }
        const uint32_t pos = atomicAdd(&cnt[lq], 1u);
        if (pos < (uint32_t)BUF) { buf[lq * BUF + pos].s = s; buf[lq * BUF + pos].c = c; }
        if (pos + 1 > (uint32_t)(BUF - TOPK_CT)) *flag = 1;
      }
    }
    __syncthreads();
    const bool merge = (*flag != 0) || (c0 + TOPK_CT >= c_end);
    __syncthreads();
    if (!merge) continue;
    // merge: wavefront w takes its 16 queries one after the other (every wavefront runs the same barriers)
    TopkEnt* ws = srt + w * BUF;
    for (int i = 0; i < 16; i++) {
      const uint32_t lq = 16 * w + i, q = q_blk + lq;
      const uint32_t n = min(cnt[lq], (uint32_t)BUF), L = len[lq], p = par[lq];
      const TopkEnt* B = buf + lq * BUF;
      for (uint32_t j = lane; j < n; j += 64) {                       // rank inside the buffer: its place in the sorted copy
        const TopkEnt e = B[j];
        uint32_t rank = 0;
        for (uint32_t m = 0; m < n; m++) rank += tk_better(B[m].s, B[m].c, e.s, e.c) ? 1u : 0u;
        ws[rank] = e;
      }
      __syncthreads();
      if (i == 0 && threadIdx.x == 0) *flag = 0;
      if (n > 0) {
        const TopkEnt* A = my_lists + (size_t)p * half + (size_t)q * K;
        TopkEnt* O = my_lists + (size_t)(p ^ 1u) * half + (size_t)q * K;
        for (uint32_t j = lane; j < L; j += 64) {
          const TopkEnt e = A[j];
          const uint32_t pos = j + tk_count_better(ws, n, e.s, e.c);
          if (pos < K) { O[pos] = e; if (pos == K - 1) thr[lq] = e; }
        }
        for (uint32_t j = lane; j < n; j += 64) {
          const TopkEnt e = ws[j];
          const uint32_t pos = j + tk_count_better(A, L, e.s, e.c);
          if (pos < K) { O[pos] = e; if (pos == K - 1) thr[lq] = e; }
        }
        if (lane == 0) { len[lq] = min(K, L + n); par[lq] = p ^ 1u; cnt[lq] = 0; }
      }
      __syncthreads();
    }
  }
  // the list of every query into half 0
  for (int i = 0; i < 16; i++) {
    const uint32_t lq = 16 * w + i, q = q_blk + lq;
    if (q >= nq) break;
    const uint32_t L = len[lq];
    if (par[lq]) {
      const TopkEnt* A = my_lists + half + (size_t)q * K;
      TopkEnt* O = my_lists + (size_t)q * K;
      for (uint32_t j = lane; j < L; j += 64) O[j] = A[j];
    }
    if (lane == 0) lens_out[(size_t)split * nq_pad + q] = L;
  }
}

// one merge round: the lists of splits 2p and 2p + 1 (in[], lens_in) -> list p (out[], lens_out); one wavefront per (query, p)
__global__ void __launch_bounds__(256)
k_topk_merge2(const TopkEnt* __restrict__ in, const uint32_t* __restrict__ lens_in, uint32_t s_in, uint32_t nq, uint32_t nq_pad,
              uint32_t K, TopkEnt* __restrict__ out, uint32_t* __restrict__ lens_out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s_out = (s_in + 1) / 2;
  const uint64_t n_work = (uint64_t)nq * s_out;
  const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t wi = wave0; wi < n_work; wi += nwaves) {
    const uint32_t p = (uint32_t)(wi / nq), q = (uint32_t)(wi % nq);
    const uint32_t sa = 2 * p, sb = 2 * p + 1;
    const TopkEnt* A = in + ((size_t)sa * nq_pad + q) * K;
    const uint32_t La = lens_in[(size_t)sa * nq_pad + q];
    const TopkEnt* B = in + ((size_t)(sb < s_in ? sb : sa) * nq_pad + q) * K;
    const uint32_t Lb = sb < s_in ? lens_in[(size_t)sb * nq_pad + q] : 0u;
    TopkEnt* O = out + ((size_t)p * nq_pad + q) * K;
    for (uint32_t j = lane; j < La; j += 64) {
      const TopkEnt e = A[j];
      const uint32_t pos = j + tk_count_better(B, Lb, e.s, e.c);
      if (pos < K) O[pos] = e;
    }
    for (uint32_t j = lane; j < Lb; j += 64) {
      const TopkEnt e = B[j];
      const uint32_t pos = j + tk_count_better(A, La, e.s, e.c);
      if (pos < K) O[pos] = e;
    }
    if (lane == 0) lens_out[(size_t)p * nq_pad + q] = min(K, La + Lb);
  }
}

// the final list of every query (split 0 of `lists`) -> idx [nq][K], score [nq][K], padded with (UINT32_MAX, -inf)
__global__ void __launch_bounds__(256)
k_topk_emit(const TopkEnt* __restrict__ lists, const uint32_t* __restrict__ lens, uint32_t nq, uint32_t K,
            uint32_t* __restrict__ idx, float* __restrict__ score) {
  const uint64_t total = (uint64_t)nq * K;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t q = (uint32_t)(t / K), j = (uint32_t)(t % K);
    if (j < lens[q]) { const TopkEnt e = lists[t]; idx[t] = e.c; score[t] = e.s; }
    else { idx[t] = TOPK_NONE; score[t] = -INFINITY; }
  }
}

}  // namespace fmx
