// fmx_rankq_kernels.h -- kernels of fmx_evaluate_rank (fmx_rankq.hip): tie-averaged NDCG / recall / precision
// at up to four cutoffs inside every query, over the sorted keys and scans fmx_evaluate_by_query leaves (fmx_evalq_kernels.h).
//
// k_rankq_bounds  grid-stride over the sorted positions: the last row of a query stores where its segment ends.
// k_rankq_top     one wavefront per query: walks the top min(rows_q, k_max) positions of the segment 64 at a step; the lane at the
//                 ascending tail of a tie run adds the run's terms; the query's sums meet in the xor butterfly, the means'
//                 numerators run wavefront (query order) -> BLOCK PARTIALS (no float atomics).
// k_rankq_final2  one wavefront sums the block partials in a fixed order.
//
// Every fp64 sum runs lane (step order) -> wavefront (xor butterfly) -> wavefront's queries (query order) -> block (wave order) ->
// blocks (k_rankq_final2) on a grid that is a fixed function of n_queries (rankq_grid): two calls with unchanged parameters are
// bit-identical.  One query never shares a wavefront with another, so nothing depends on a packing.  The wavefronts exchange
// nothing during the walk; LDS carries only the four wave sums of a block at its end, as in k_evalq_final.
#pragma once
#include "fmx_evalq_kernels.h"

namespace fmx {

constexpr int RANKQ_MAX_CUT = FMX_RANK_MAX_CUTOFFS;
constexpr int RANKQ_ND = 4 * RANKQ_MAX_CUT;       // per cutoff: sum hits_q, sum ndcg_q, sum recall_q, sum precision_q
constexpr int RANKQ_NC = RANKQ_MAX_CUT + 1;       // per cutoff: tied queries; then the relevant queries
inline uint32_t rankq_grid(uint32_t n_queries) { return n_queries < EVALX_BLOCKS * 4u ? (n_queries + 3u) / 4u : EVALX_BLOCKS; }

struct RankqCut { uint32_t n; uint32_t k[RANKQ_MAX_CUT]; };   // n cutoffs, strictly ascending: k[n - 1] is k_max

static __global__ void __launch_bounds__(256)
k_rankq_bounds(const unsigned long long* __restrict__ ks, uint32_t n, uint32_t* __restrict__ qend) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t q = (uint32_t)(ks[i] >> EVALQ_QID_SHIFT);
    if (i + 1 == n || (uint32_t)(ks[i + 1] >> EVALQ_QID_SHIFT) != q) qend[q] = i + 1;
  }
}

// The sort is ascending: the row at sorted position i of a query whose segment ends at e has the descending 0-based rank e - 1 - i.
// Lane l of step `off` holds the rank r = off + l, position i = e - 1 - r (consecutive lanes, consecutive addresses), for
// r < w = min(rows_q, k_max).  Position i is the ASCENDING TAIL of its tie run when it is the segment's last or its successor's
// key differs above the label bit; it then owns the run: a = r, b = e - runhead[i] (the head may lie below the window: the run's
// count is still whole), t = b - a, p = t - (negatives in [runhead[i], i]).  Every run that begins above a cutoff has its tail at a
// rank < K <= k_max, inside the window.  D[] has k_max + 1 entries, b' <= K <= k_max.
// Queries without a relevant row skip the walk (every term is 0); qend of a query without rows is never read.
// dcg_q / hits_q: nullptr or [n_queries][cut.n].  partials of block b: dpart[RANKQ_ND * b + 4 * j + {0: hits, 1: ndcg, 2: recall,
// 3: precision}], cpart[RANKQ_NC * b + {j: tied at cutoff j, RANKQ_MAX_CUT: relevant}]
static __global__ void __launch_bounds__(256)
k_rankq_top(const unsigned long long* __restrict__ ks, const uint32_t* __restrict__ negbefore, const uint32_t* __restrict__ runhead,
            const uint32_t* __restrict__ qend, const uint32_t* __restrict__ pos_q, const uint32_t* __restrict__ neg_q, uint32_t n_queries,
            RankqCut cut, const double* __restrict__ D, double* __restrict__ dcg_q, double* __restrict__ hits_q,
            double* __restrict__ dpart, unsigned long long* __restrict__ cpart) {
  __shared__ double dred[RANKQ_ND][4];
  __shared__ unsigned long long cred[RANKQ_NC][4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t k_max = cut.k[cut.n - 1];
  double sum[RANKQ_ND];                            // the wavefront's running sums (wave-uniform)
  unsigned long long cnt[RANKQ_NC];
#pragma unroll
  for (int j = 0; j < RANKQ_ND; j++) sum[j] = 0;
#pragma unroll
  for (int j = 0; j < RANKQ_NC; j++) cnt[j] = 0;
  for (uint64_t q = wave; q < n_queries; q += n_waves) {
    const uint32_t pos = pos_q[q], m = pos + neg_q[q];
    double hit[RANKQ_MAX_CUT], dcg[RANKQ_MAX_CUT];
    int tied[RANKQ_MAX_CUT];
#pragma unroll
    for (int j = 0; j < RANKQ_MAX_CUT; j++) { hit[j] = 0; dcg[j] = 0; tied[j] = 0; }
    if (pos) {
      const uint32_t e = qend[q], win = min(m, k_max);
      for (uint32_t off = 0; off < win; off += 64u) {
        const uint32_t r = off + lane;
        if (r < win) {
          const uint32_t i = e - 1u - r;
          const unsigned long long k = ks[i];
          if (r == 0 || (ks[i + 1] >> 1) != (k >> 1)) {
            const uint32_t rh = runhead[i];
            const uint32_t a = r, b = e - rh, t = b - a;
            const uint32_t p = t - (negbefore[i] + (uint32_t)(~k & 1ull) - negbefore[rh]);
            if (p) {
              const double Da = D[a];
#pragma unroll
              for (int j = 0; j < RANKQ_MAX_CUT; j++) {
                if (j < (int)cut.n && a < cut.k[j]) {
                  const uint32_t bb = min(b, cut.k[j]);
                  hit[j] += ((double)p * (double)(bb - a)) / (double)t;
                  dcg[j] += ((double)p * (D[bb] - Da)) / (double)t;
                  if (p < t) tied[j] = 1;
                }
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < RANKQ_MAX_CUT; j++) {
      if (j < (int)cut.n) {
        double hq = 0, dq = 0;
        if (pos) {                                 // (wave-uniform)
          hq = wave_sum_d(hit[j]); dq = wave_sum_d(dcg[j]);
          sum[4 * j + 0] += hq;
          sum[4 * j + 1] += dq / D[min(pos, cut.k[j])];
          sum[4 * j + 2] += hq / (double)pos;
          sum[4 * j + 3] += hq / (double)cut.k[j];
          if (__any(tied[j])) cnt[j] += 1;
        }
        if (lane == 0) {
          if (dcg_q) dcg_q[q * cut.n + j] = dq;
          if (hits_q) hits_q[q * cut.n + j] = hq;
        }
      }
    }
    if (pos) cnt[RANKQ_MAX_CUT] += 1;
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < RANKQ_ND; j++) dred[j][w] = sum[j];
#pragma unroll
    for (int j = 0; j < RANKQ_NC; j++) cred[j][w] = cnt[j];
  }
  __syncthreads();
  if (threadIdx.x < RANKQ_ND) dpart[RANKQ_ND * blockIdx.x + threadIdx.x] = ((dred[threadIdx.x][0] + dred[threadIdx.x][1]) + dred[threadIdx.x][2]) + dred[threadIdx.x][3];
  if (threadIdx.x < RANKQ_NC) cpart[RANKQ_NC * blockIdx.x + threadIdx.x] = cred[threadIdx.x][0] + cred[threadIdx.x][1] + cred[threadIdx.x][2] + cred[threadIdx.x][3];
}

// one wavefront: lane l sums the blocks l, l + 64, ... in order, then the butterfly.  dout[RANKQ_ND], cout[RANKQ_NC]
static __global__ void __launch_bounds__(64)
k_rankq_final2(const double* __restrict__ dpart, const unsigned long long* __restrict__ cpart, uint32_t nblk,
               double* __restrict__ dout, unsigned long long* __restrict__ cout) {
  for (int j = 0; j < RANKQ_ND; j++) {
    double d = 0;
    for (uint32_t b = threadIdx.x; b < nblk; b += 64) d += dpart[RANKQ_ND * b + j];
    d = wave_sum_d(d);
    if (threadIdx.x == 0) dout[j] = d;
  }
  for (int j = 0; j < RANKQ_NC; j++) {
    unsigned long long c = 0;
    for (uint32_t b = threadIdx.x; b < nblk; b += 64) c += cpart[RANKQ_NC * b + j];
    c = wave_sum_u64(c);
    if (threadIdx.x == 0) cout[j] = c;
  }
}

}  // namespace fmx
