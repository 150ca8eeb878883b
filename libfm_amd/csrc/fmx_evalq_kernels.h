// fmx_evalq_kernels.h -- kernels of fmx_evaluate_by_query (fmx_evalq.hip): the exact AUC inside every query.
//
// k_evalq_keys     grid-stride over the rows: one 64-bit sort key per row, the query id above fmx_evaluate_ex's 33-bit key.
// EvalqQHead       what the third library scan reads from the sorted keys: "index of the position if it heads a query, else 0"
//                  (the other two scans are fmx_evaluate_ex's: EvalxIsNeg, EvalxHead -- a query boundary breaks a run of equal
//                  `ks >> 1` by itself).
// k_evalq_ranksum  over the sorted positions, a contiguous chunk per wavefront: every positive adds its within-query rank terms; the
//                  segments of equal queries are reduced inside the wavefront with shuffles, ONE 64-bit integer atomic per
//                  (wavefront, query segment of its chunk).  The last row of a query stores the query's pos / neg counts (plain
//                  stores: nobody else writes them).
// k_evalq_final    grid-stride over the queries: auc_q, validity and the sums as BLOCK PARTIALS (no float atomics).
// k_evalq_final2   one wavefront sums the block partials in a fixed order.
//
// Only integers meet in atomics (an integer sum is exact in any order); every fp64 sum runs lane -> wavefront (xor butterfly) ->
// block (wave order) -> blocks (k_evalq_final2) on a grid that is a fixed function of n_queries: two calls with unchanged
// parameters are bit-identical.  No LDS exchange between wavefronts in k_evalq_ranksum, no workgroup waits for another.
#pragma once
#include "fmx_eval_kernels.h"

namespace fmx {

constexpr int EVALQ_QID_SHIFT = EVALX_KEY_BITS;          // the query id sits above the 33 bits of fmx_evaluate_ex's key
constexpr uint32_t EVALQ_NO_QUERY = 0xFFFFFFFFu;         // lanes past the last row (query ids are below 2^31)

// key = qid << 33 | evalx_key32(p) << 1 | label, p formed exactly as k_evalx_score forms it
static __global__ void __launch_bounds__(256)
k_evalq_keys(const float* __restrict__ rest, const float* __restrict__ target, const uint32_t* __restrict__ qid, uint32_t n_rows,
             Hyper h, int add_w0, const double* __restrict__ w0_ptr, unsigned long long* __restrict__ keys) {
  const float w0 = (add_w0 && h.k0) ? (float)(*w0_ptr) : 0.f;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_rows; e += gridDim.x * blockDim.x) {
    const float p = add_w0 ? w0 + rest[e] : rest[e];
    const unsigned long long pos = (target[e] >= 0) ? 1ull : 0ull;   // fm_learn.h:118
    keys[e] = ((unsigned long long)qid[e] << EVALQ_QID_SHIFT) | ((unsigned long long)evalx_key32(p) << 1) | pos;
  }
}

struct EvalqQHead {                           // i if position i heads its query, else 0 (position 0 heads its query with 0 anyway)
  const unsigned long long* ks;
  __host__ __device__ __forceinline__ uint32_t operator()(uint32_t i) const {
    return (i > 0 && (ks[i] >> EVALQ_QID_SHIFT) != (ks[i - 1] >> EVALQ_QID_SHIFT)) ? i : 0u;
  }
};

// negbefore / runhead as in k_evalx_ranksum, qhead[i] = first position of i's query.  A positive at i has
// negbefore[i] - negbefore[qhead[i]] negatives of its query with a score <= its own and negbefore[runhead[i]] - negbefore[qhead[i]]
// with a score < its own: together 2 * below + equal, inside the query.  Every wavefront of the grid owns ONE contiguous chunk of
// positions (a multiple of 64, the same for all) and walks it 64 positions at a step: consecutive lanes hold consecutive
// positions, so the lanes of one query are contiguous; a segmented inclusive scan (shuffles) leaves every segment's sum in its
// last lane, which adds it to num2_q[query].  The segment that reaches lane 63 is not added yet but carried into the next step,
// where it either goes on in lane 0 or is added then: one atomic per (wavefront, query segment of its chunk) -- a query of
// many rows costs its word (rows / chunk) atomics, not (rows / 64).  Every step runs with all 64 lanes (the bounds are the
// wavefront's), lanes past n carry EVALQ_NO_QUERY and 0.
// pos_q / neg_q: the last row of a query knows the query's first position and the negatives before both, so it stores the two
// counts itself -- no atomics, and a query without rows keeps the zeros the host put there.
static __global__ void __launch_bounds__(256)
k_evalq_ranksum(const unsigned long long* __restrict__ ks, const uint32_t* __restrict__ negbefore, const uint32_t* __restrict__ runhead,
                const uint32_t* __restrict__ qhead, uint32_t n, unsigned long long* __restrict__ num2_q,
                uint32_t* __restrict__ pos_q, uint32_t* __restrict__ neg_q) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t chunk = ((n + n_waves * 64u - 1u) / (n_waves * 64u)) * 64u;   // (n < 2^31 and n_waves * 64 <= 2^19: no overflow below)
  const uint32_t begin = wave * chunk, end = min(n, begin + chunk);
  uint32_t carry_q = EVALQ_NO_QUERY;            // the segment open at the end of the previous step (wavefront-uniform)
  unsigned long long carry_c = 0;
  for (uint32_t base = begin; base < end; base += 64u) {
    const uint32_t i = base + lane;
    uint32_t q = EVALQ_NO_QUERY;
    unsigned long long c = 0;
    if (i < n) {
      const unsigned long long k = ks[i];
      q = (uint32_t)(k >> EVALQ_QID_SHIFT);
      const uint32_t qh = qhead[i], nbq = negbefore[qh], nbi = negbefore[i];
      if (k & 1ull) c = (unsigned long long)(nbi - nbq) + (unsigned long long)(negbefore[runhead[i]] - nbq);
      if (i + 1 == n || (uint32_t)(ks[i + 1] >> EVALQ_QID_SHIFT) != q) {
        const uint32_t neg = nbi + (uint32_t)(~k & 1ull) - nbq;
        neg_q[q] = neg;
        pos_q[q] = (i + 1 - qh) - neg;
      }
    }
    if (lane == 0 && carry_c) {
      if (carry_q == q) c += carry_c;
      else atomicAdd(&num2_q[carry_q], carry_c);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long cu = __shfl_up(c, o);
      const uint32_t qu = __shfl_up(q, o);
      if (lane >= (uint32_t)o && qu == q) c += cu;
    }
    const uint32_t qn = __shfl_down(q, 1);
    if (lane != 63u && qn != q && c) atomicAdd(&num2_q[q], c);
    carry_q = __shfl(q, 63);
    carry_c = __shfl(c, 63);
  }
  if (lane == 0 && carry_c) atomicAdd(&num2_q[carry_q], carry_c);
}

// partials of block b: dpart[2 * b + {0: sum rows_q auc_q, 1: sum auc_q}] over the valid queries,
// cpart[6 * b + {0: valid, 1: one-class, 2: empty queries, 3: rows of the valid ones, 4: sum num2_q, 5: sum 2 pos_q neg_q}]
static __global__ void __launch_bounds__(256)
k_evalq_final(const unsigned long long* __restrict__ num2_q, const uint32_t* __restrict__ pos_q, const uint32_t* __restrict__ neg_q,
              uint32_t n_queries, double* __restrict__ dpart, unsigned long long* __restrict__ cpart) {
  __shared__ double dred[2][4];
  __shared__ unsigned long long cred[6][4];
  double d[2] = {0, 0};
  unsigned long long c[6] = {0, 0, 0, 0, 0, 0};
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_queries; q += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long p = pos_q[q], g = neg_q[q];
    if (p && g) {
      const unsigned long long num2 = num2_q[q];
      const double auc = (double)num2 / (2.0 * (double)p * (double)g);
      d[0] += (double)(p + g) * auc; d[1] += auc;
      c[0] += 1; c[3] += p + g; c[4] += num2; c[5] += 2ull * p * g;
    } else if (p + g) c[1] += 1;
    else c[2] += 1;
  }
  const uint32_t w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 2; j++) { d[j] = wave_sum_d(d[j]); if ((threadIdx.x & 63u) == 0) dred[j][w] = d[j]; }
#pragma unroll
  for (int j = 0; j < 6; j++) { c[j] = wave_sum_u64(c[j]); if ((threadIdx.x & 63u) == 0) cred[j][w] = c[j]; }
  __syncthreads();
  if (threadIdx.x < 2) dpart[2 * blockIdx.x + threadIdx.x] = ((dred[threadIdx.x][0] + dred[threadIdx.x][1]) + dred[threadIdx.x][2]) + dred[threadIdx.x][3];
  if (threadIdx.x < 6) cpart[6 * blockIdx.x + threadIdx.x] = cred[threadIdx.x][0] + cred[threadIdx.x][1] + cred[threadIdx.x][2] + cred[threadIdx.x][3];
}

// one wavefront: lane l sums the blocks l, l + 64, ... in order, then the butterfly.  dout[2], cout[6]
static __global__ void __launch_bounds__(64)
k_evalq_final2(const double* __restrict__ dpart, const unsigned long long* __restrict__ cpart, uint32_t nblk,
               double* __restrict__ dout, unsigned long long* __restrict__ cout) {
  for (int j = 0; j < 2; j++) {
    double d = 0;
    for (uint32_t b = threadIdx.x; b < nblk; b += 64) d += dpart[2 * b + j];
    d = wave_sum_d(d);
    if (threadIdx.x == 0) dout[j] = d;
  }
  for (int j = 0; j < 6; j++) {
    unsigned long long c = 0;
    for (uint32_t b = threadIdx.x; b < nblk; b += 64) c += cpart[6 * b + j];
    c = wave_sum_u64(c);
    if (threadIdx.x == 0) cout[j] = c;
  }
}

}  // namespace fmx
