// fmx_snap_kernels.h -- the device side of the serving snapshot file (include/fmx.h "fmx_compact_save"; the
// host side is fmx_snap.hip, the byte layout fmx_snap_format.h).  Plain streaming kernels beside those of the checkpoint:
//
//   k_snap_rows<T, PACK>  one chunk of a section between a snapshot table and a contiguous staging buffer.  A section's row is `cols`
//                         elements of type T (uint16_t: a bf16 factor row, cols = num_factor of the table's rs; uint32_t: the bf16
//                         snapshot's w; unsigned long long: the int8 blocks and the directory, taken as their 8-byte words) at
//                         tab[row * rs .. + cols); rows r0 .. of the table.  One thread per 8-BYTE WORD of the chunk: it moves the
//                         word's 8 / sizeof(T) elements (elements past the section's end are zero bits) and adds the word's
//                         checksum term mix64(u ^ (i * GOLDEN)), i the word's index in the SECTION, summed per wavefront and added
//                         by one 64-bit integer atomic (ckpt_wave_add): a sum mod 2^64 does not depend on the order.  PACK = false
//                         reads the staging buffer -- what arrived in device memory -- and writes the table; the padding of a row
//                         (columns cols .. rs) is never touched.
//   k_snap_dir_check      one pass over the rank directory of a pruned file, one thread per pair: base[0] == 0, base[j + 1] ==
//                         base[j] + popcount(bits[j]), no bit at or beyond n in the last word, base[last] + popcount(bits[last]) ==
//                         kept.  *bad |= 1 otherwise.  With all four every lookup (dir_slot) lands below `kept`: the bases ascend by
//                         the popcounts and end at kept.  A load reads *bad before the directory is handed to any scoring kernel.
#pragma once
#include "fmx_ckpt_kernels.h"

namespace fmx {

template <class T, bool PACK>
__global__ void __launch_bounds__(256)
k_snap_rows(T* __restrict__ tab, uint32_t rs, uint32_t cols, uint64_t r0, uint32_t n_elems, uint64_t word0,
            unsigned long long* __restrict__ stage, unsigned long long* __restrict__ sum) {
  constexpr uint32_t EPW = 8u / (uint32_t)sizeof(T), BITS = 8u * (uint32_t)sizeof(T);
  const uint32_t n_words = (n_elems + EPW - 1u) / EPW;
  const uint32_t stride = gridDim.x * blockDim.x;
  unsigned long long acc = 0ull;
  // (the trip count is uniform per wavefront up to the last round, where the lanes past n_words add 0: the shuffles see all 64 lanes)
  for (uint32_t w0 = blockIdx.x * blockDim.x; w0 < n_words; w0 += stride) {
    const uint32_t w = w0 + threadIdx.x;
    if (w < n_words) {
      unsigned long long u = PACK ? 0ull : stage[w];
#pragma unroll
      for (uint32_t q = 0; q < EPW; q++) {
        const uint32_t e = EPW * w + q;
        if (e < n_elems) {
          const uint32_t r = e / cols, c = e - r * cols;
          T* p = tab + (r0 + r) * (uint64_t)rs + c;
          if constexpr (EPW == 1u) { if (PACK) u = (unsigned long long)*p; else *p = (T)u; }
          else if (PACK) u |= (unsigned long long)*p << (BITS * q);
          else *p = (T)(u >> (BITS * q));
        }
      }
      if (PACK) stage[w] = u;
      acc += mix64(u ^ ((word0 + w) * CKPT_GOLDEN));
    }
  }
  ckpt_wave_add(acc, sum);
}

static __global__ void __launch_bounds__(256)
k_snap_dir_check(const uint2* __restrict__ dir, uint64_t nwords, uint64_t n, uint64_t kept, uint32_t* __restrict__ bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool wrong = false;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nwords; j += stride) {
    const uint2 p = dir[j];
    const uint64_t next = (uint64_t)p.y + (uint64_t)__popc(p.x);
    if (j == 0 && p.y != 0u) wrong = true;
    if (j + 1 < nwords) { if ((uint64_t)dir[j + 1].y != next) wrong = true; }
    else {
      const uint64_t tail = n - 32u * j;                            // ids of the last word: 1 .. 32
      if (tail < 32u && (p.x >> (uint32_t)tail) != 0u) wrong = true;
      if (next != kept) wrong = true;
    }
  }
  if (wrong) atomicOr(bad, 1u);
}

}  // namespace fmx
