// fmx_ckpt_kernels.h -- the device side of the binary checkpoint (include/fmx.h "fmx_checkpoint_*"; the host
// side is fmx_ckpt.hip, the byte layout fmx_ckpt_format.h).  Plain streaming kernels:
//
//   k_ckpt_rows<PACK>  one chunk of a section between a strided table and a contiguous staging buffer.  A section's row is `cols`
//                      floats: with `lin` the linear coordinate's value lin[row * ls] first, then tab[row * rs + c]; rows are
//                      r0 .. r0 + cnt - 1, or ids[r0 ..] (the sparse state: gather on save, scatter on load).  One thread per
//                      8-BYTE WORD of the chunk: it moves the word's two floats (the last word of a section of odd length carries
//                      32 zero bits) and adds the word's checksum term mix64(u ^ (i * GOLDEN)), i the word's index in the SECTION.
//                      The terms are summed per wavefront and one 64-bit integer atomic per wavefront adds them to *sum: a sum mod
//                      2^64 is independent of order, so the file does not depend on scheduling.  PACK = false reads the staging
//                      buffer -- what arrived in device memory -- and writes the table; the padding of a row is never touched.
//   k_ckpt_ids         the checksum of a u32 id list that is on the device, and its validation: strictly ascending, every id < n
//                      (*bad |= 1 otherwise).  A load runs it over the WHOLE list and reads *bad before any scatter by id starts.
//   k_ckpt_flag_*      flag[j] = 1 where feature j's state row is not what fmx_*_begin would reproduce from the parameters
//                      (AdaGrad: any of n_w, n_v[0 .. k) differs from init_acc; FTRL: any (z, n) differs from ftrl_start of its
//                      theta), bit for bit.  L lanes (a power of two <= 64) share a feature, as in k_param_sparsity.
//   k_ckpt_compact     ids[pos[j]] = j for the flagged rows, pos the exclusive scan of the flags: ascending by construction.
//
// The group form (fmx_group_checkpoint_*): the file is in GLOBAL feature order, every member of the group holds
// the rows of the features it owns, and no kernel dereferences another device's table -- staging buffers travel, tables do not.
//   k_ckpt_rows_shard<PACK>  k_ckpt_rows on one member: element e of the chunk belongs to global row ids ? ids[r0 + r] : r0 + r, and
//                      Shard::place says whether this member owns that row and where.  The filter is per 4-byte ELEMENT, not per
//                      word: a word of w (cols = 1) holds two features, a word of a state row with odd cols = k + 1 straddles two
//                      rows, and either pair may have two owners.  PACK = true writes the whole chunk, 0 where the row is someone
//                      else's (a complete chunk with holes) and forms no checksum: a word is not complete on one member.
//                      PACK = false stores the owned elements only; with sum != nullptr (the lead) it adds the terms of ALL words
//                      of the staging buffer -- what arrived in device memory -- as k_ckpt_rows<false> does.
//   k_ckpt_merge       on the lead: one thread per word ORs the members' chunks (the owners are disjoint, so OR is select), writes
//                      the pipe's staging buffer and adds the word's checksum term; one integer atomic per wavefront.
//   k_ckpt_global_ids  rows[i] = the global id of this member's local row rows[i] (Shard::global), in place.
#pragma once
#include "fmx_ftrl_kernels.h"

namespace fmx {

constexpr uint64_t CKPT_GOLDEN = 0x9E3779B97F4A7C15ULL;

// a wavefront's sum of 64-bit terms added to *sum by one atomic (every lane of the wavefront calls this)
__device__ __forceinline__ void ckpt_wave_add(unsigned long long term, unsigned long long* __restrict__ sum) {
  for (int off = 32; off > 0; off >>= 1) term += __shfl_down(term, off, 64);
  if ((threadIdx.x & 63u) == 0 && term) atomicAdd(sum, term);
}

// the strided tables of one section and which rows of them a chunk covers
struct CkptRows {
  float* tab; float* lin;          // tab: rows of rs floats (nullptr with cols_tab == 0); lin: the linear coordinates, ls apart, or nullptr
  uint32_t rs, ls, cols;           // cols = floats per row of the section = (lin ? 1 : 0) + the columns taken from tab
  const uint32_t* ids;             // nullptr: row r of the section is table row r
};

template <bool PACK>
__global__ void __launch_bounds__(256)
k_ckpt_rows(CkptRows t, uint64_t r0, uint32_t n_elems, uint64_t word0, unsigned long long* __restrict__ stage,
            unsigned long long* __restrict__ sum) {
  const uint32_t n_words = (n_elems + 1u) >> 1;
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t first = t.lin ? 1u : 0u;
  unsigned long long acc = 0ull;
  // (the trip count is uniform per wavefront up to the last round, where the lanes past n_words add 0: the shuffles see all 64 lanes)
  for (uint32_t w0 = blockIdx.x * blockDim.x; w0 < n_words; w0 += stride) {
    const uint32_t w = w0 + threadIdx.x;
    if (w < n_words) {
      unsigned long long u = PACK ? 0ull : stage[w];
      uint32_t half[2] = {(uint32_t)u, (uint32_t)(u >> 32)};
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const uint32_t e = 2u * w + (uint32_t)q;
        if (e < n_elems) {
          const uint32_t r = e / t.cols, c = e - r * t.cols;
          const uint64_t row = t.ids ? (uint64_t)t.ids[r0 + r] : r0 + r;
          float* p = (c < first) ? t.lin + row * t.ls : t.tab + row * t.rs + (c - first);
          if (PACK) half[q] = __float_as_uint(*p); else *p = __uint_as_float(half[q]);
        }
      }
      if (PACK) { u = (unsigned long long)half[0] | (unsigned long long)half[1] << 32; stage[w] = u; }
      acc += mix64(u ^ ((word0 + w) * CKPT_GOLDEN));
    }
  }
  ckpt_wave_add(acc, sum);
}

// (the two elements of a word share a row more often than not: the permutation is evaluated once for both then)
template <bool PACK>
__global__ void __launch_bounds__(256)
k_ckpt_rows_shard(CkptRows t, Shard sh, uint64_t r0, uint32_t n_elems, uint64_t word0, unsigned long long* __restrict__ stage,
                  unsigned long long* __restrict__ sum) {
  const uint32_t n_words = (n_elems + 1u) >> 1;
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t first = t.lin ? 1u : 0u;
  unsigned long long acc = 0ull;
  for (uint32_t w0 = blockIdx.x * blockDim.x; w0 < n_words; w0 += stride) {
    const uint32_t w = w0 + threadIdx.x;
    if (w < n_words) {
      unsigned long long u = PACK ? 0ull : stage[w];
      uint32_t half[2] = {(uint32_t)u, (uint32_t)(u >> 32)};
      uint32_t seen_r = 0xFFFFFFFFu, local = 0u;
      bool mine = false;
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const uint32_t e = 2u * w + (uint32_t)q;
        if (e < n_elems) {
          const uint32_t r = e / t.cols, c = e - r * t.cols;
          if (r != seen_r) {
            seen_r = r;
            mine = sh.place(t.ids ? t.ids[r0 + r] : (uint32_t)(r0 + r), &local);
          }
          if (mine) {
            float* p = (c < first) ? t.lin + (uint64_t)local * t.ls : t.tab + (uint64_t)local * t.rs + (c - first);
            if (PACK) half[q] = __float_as_uint(*p); else *p = __uint_as_float(half[q]);
          }
        }
      }
      if (PACK) stage[w] = (unsigned long long)half[0] | (unsigned long long)half[1] << 32;
      else acc += mix64(u ^ ((word0 + w) * CKPT_GOLDEN));
    }
  }
  if (!PACK && sum) ckpt_wave_add(acc, sum);                     // (sum is a kernel argument: the whole grid takes the same side)
}

struct CkptParts { const unsigned long long* p[16]; int n; };   // the members' chunks, all on the lead's device (a group has <= 16 members)

static __global__ void __launch_bounds__(256)
k_ckpt_merge(CkptParts parts, uint32_t n_words, uint64_t word0, unsigned long long* __restrict__ out, unsigned long long* __restrict__ sum) {
  const uint32_t stride = gridDim.x * blockDim.x;
  unsigned long long acc = 0ull;
  for (uint32_t w0 = blockIdx.x * blockDim.x; w0 < n_words; w0 += stride) {
    const uint32_t w = w0 + threadIdx.x;
    if (w < n_words) {
      unsigned long long u = 0ull;
      for (int i = 0; i < parts.n; i++) u |= parts.p[i][w];
      out[w] = u;
      acc += mix64(u ^ ((word0 + w) * CKPT_GOLDEN));
    }
  }
  ckpt_wave_add(acc, sum);
}

static __global__ void __launch_bounds__(256)
k_ckpt_global_ids(Shard sh, uint32_t* __restrict__ rows, uint64_t count) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) rows[i] = sh.global(rows[i]);
}

static __global__ void __launch_bounds__(256)
k_ckpt_ids(const uint32_t* __restrict__ ids, uint64_t count, uint64_t n, unsigned long long* __restrict__ sum, uint32_t* __restrict__ bad) {
  const uint64_t n_words = (count + 1) >> 1;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long acc = 0ull;
  bool wrong = false;
  for (uint64_t w0 = (uint64_t)blockIdx.x * blockDim.x; w0 < n_words; w0 += stride) {
    const uint64_t w = w0 + threadIdx.x;
    if (w < n_words) {
      const uint64_t e = 2 * w;
      const uint32_t a = ids[e];
      const bool two = e + 1 < count;
      const uint32_t b = two ? ids[e + 1] : 0u;
      wrong |= a >= n || (two && (b >= n || b <= a)) || (e > 0 && ids[e - 1] >= a);
      acc += mix64(((unsigned long long)a | (unsigned long long)b << 32) ^ (w * CKPT_GOLDEN));
    }
  }
  if (wrong) atomicOr(bad, 1u);
  ckpt_wave_add(acc, sum);
}

// the lanes of a feature's group agree on "differs" through a ballot; lane `sub == 0` of the group stores the flag
__device__ __forceinline__ void ckpt_flag_store(bool differs, uint64_t j, uint64_t n, uint32_t L, uint32_t grp, uint32_t sub, uint32_t* __restrict__ flag) {
  const unsigned long long bal = __ballot(differs);
  const unsigned long long mine = (L == 64u) ? bal : ((bal >> (grp * L)) & ((1ull << L) - 1ull));
  if (j < n && sub == 0) flag[j] = mine != 0ull ? 1u : 0u;
}

static __global__ void __launch_bounds__(256)
k_ckpt_flag_adagrad(const float* __restrict__ nw, const float* __restrict__ nv, uint32_t rs, uint64_t n, int k, uint32_t L, float init_acc,
                    uint32_t* __restrict__ flag) {
  const uint32_t lane = threadIdx.x & 63u, grp = lane / L, sub = lane % L, rpw = 64u / L;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint32_t want = __float_as_uint(init_acc);
  for (uint64_t r0 = wave * rpw; r0 < n; r0 += nwaves * rpw) {          // (uniform per wavefront: the ballot sees all 64 lanes)
    const uint64_t j = r0 + grp;
    bool differs = false;
    if (j < n) {
      if (sub == 0) differs = __float_as_uint(nw[j]) != want;
      for (uint32_t f = sub; f < (uint32_t)k; f += L) differs |= __float_as_uint(nv[j * rs + f]) != want;
    }
    ckpt_flag_store(differs, j, n, L, grp, sub, flag);
  }
}

static __global__ void __launch_bounds__(256)
k_ckpt_flag_ftrl(Tab tb, const float* __restrict__ zw, const float* __restrict__ zv, const float* __restrict__ nw, const float* __restrict__ nv,
                 uint64_t n, int k, uint32_t L, float D0_w, float l1_w, float D0_v, float l1_v, float init_acc, uint32_t* __restrict__ flag) {
  const uint32_t lane = threadIdx.x & 63u, grp = lane / L, sub = lane % L, rpw = 64u / L;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint32_t want_n = __float_as_uint(init_acc);
  for (uint64_t r0 = wave * rpw; r0 < n; r0 += nwaves * rpw) {
    const uint64_t j = r0 + grp;
    bool differs = false;
    if (j < n) {
      if (sub == 0)
        differs = __float_as_uint(zw[j]) != __float_as_uint(ftrl_start(tb.w[j * tb.ws], D0_w, l1_w)) || __float_as_uint(nw[j]) != want_n;
      for (uint32_t f = sub; f < (uint32_t)k; f += L) {
        const uint64_t i = j * tb.rs + f;
        differs |= __float_as_uint(zv[i]) != __float_as_uint(ftrl_start(tb.V[i], D0_v, l1_v)) || __float_as_uint(nv[i]) != want_n;
      }
    }
    ckpt_flag_store(differs, j, n, L, grp, sub, flag);
  }
}

static __global__ void __launch_bounds__(256)
k_ckpt_compact(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint64_t n, uint32_t* __restrict__ ids) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
    if (flag[j]) ids[pos[j]] = (uint32_t)j;
}

}  // namespace fmx
