// fmx_compact_kernels.h -- kernels of the bf16 serving snapshot (fmx_compact.hip; include/fmx.h "fmx_compact_*").
//
// k_compact_quant   one pass over V: the bf16 rows (same row stride in ELEMENTS, half the bytes) and the three numbers of
//                   fmx_compact_info as BLOCK PARTIALS (no float atomics).
// k_compact_final   one wavefront folds the block partials in a fixed order.
// RowsBf16          the snapshot as the row source of k_rowsums and k_fetch_rows (fmx_kernels.h): a lane map of its own (MapC) and
//                   the load of a bf16 row (row_ld_c).
//
// A bf16 is the upper half of an fp32 and widens back with a 16-bit shift, so what k_rowsums computes from RowsBf16 is
// fm_model::predict of the model (w0, w, q(V)) in the very code that scores the fp32 model: only the load differs.
#pragma once
#include "fmx_kernels.h"

namespace fmx {

// the snapshot's tables: V rows of rs bf16 (rs = the model's Tab::rs), w with stride 1
struct CTab { const uint16_t* V; const float* w; uint32_t rs; };

// fp32 bit pattern -> bf16 bit pattern: round to nearest, ties to even, on bit 16; a NaN keeps its sign and upper payload and gets the
// quiet bit.  +-0, +-inf and subnormals follow the bit rule; a finite value above bf16's largest carries into the exponent: +-inf.
__host__ __device__ __forceinline__ uint32_t bf16_bits(uint32_t u) {
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x0040u;
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

constexpr uint32_t COMPACT_BLOCKS = 8192;    // cap of k_compact_quant's grid; a fixed function of the table (compact_grid)

// L lanes (a power of two <= 64) share a feature and stride over its rs elements, 64 / L features per wavefront round (the map of
// k_param_sparsity): 64 consecutive floats per wave-wide load for every k.  The padding (f >= k) is written as +0 and is not counted.
//   dpart[2 * b + {0: max |v - q(v)|, 1: sum (v - q(v))^2}] over the finite q(v), cpart[b] = non-finite q(v)
// v - q(v) is exact in fp32 (q(v) is within half an ulp_bf16 of v: Sterbenz), so the maximum does not depend on the order.
static __global__ void __launch_bounds__(256)
k_compact_quant(const float* __restrict__ V, uint32_t rs, uint64_t n, int k, uint32_t L, uint16_t* __restrict__ out,
                double* __restrict__ dpart, unsigned long long* __restrict__ cpart) {
  __shared__ double dred[2][4];
  __shared__ unsigned long long cred[4];
  const uint32_t lane = threadIdx.x & 63u, grp = lane / L, sub = lane % L, rpw = 64u / L;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  float mx = 0.f; double ss = 0.0; unsigned long long nf = 0ull;
  for (uint64_t r0 = wave * rpw; r0 < n; r0 += nwaves * rpw) {
    const uint64_t j = r0 + grp;
    if (j < n) {
      for (uint32_t f = sub; f < rs; f += L) {
        uint32_t q = 0u;
        if (f < (uint32_t)k) {
          const float v = V[j * rs + f];
          q = bf16_bits(__float_as_uint(v));
          if ((q & 0x7F80u) == 0x7F80u) nf++;
          else {
            const float err = fabsf(v - __uint_as_float(q << 16));
            mx = fmaxf(mx, err);
            ss += (double)err * (double)err;
          }
        }
        out[j * rs + f] = (uint16_t)q;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o)); nf += __shfl_xor(nf, o); }
  ss = wave_sum_d(ss);
  const uint32_t w = threadIdx.x >> 6;
  if (lane == 0) { dred[0][w] = (double)mx; dred[1][w] = ss; cred[w] = nf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    dpart[2 * blockIdx.x + 0] = fmax(fmax(dred[0][0], dred[0][1]), fmax(dred[0][2], dred[0][3]));
    dpart[2 * blockIdx.x + 1] = (dred[1][0] + dred[1][1]) + (dred[1][2] + dred[1][3]);
    cpart[blockIdx.x] = (cred[0] + cred[1]) + (cred[2] + cred[3]);
  }
}

// one wavefront: lane l folds the blocks l, l + 64, ... in order, then the butterfly.  dout[2] = {max, sum}, cout[1]
static __global__ void __launch_bounds__(64)
k_compact_final(const double* __restrict__ dpart, const unsigned long long* __restrict__ cpart, uint32_t nblk,
                double* __restrict__ dout, unsigned long long* __restrict__ cout) {
  double mx = 0.0, ss = 0.0; unsigned long long nf = 0ull;
  for (uint32_t b = threadIdx.x; b < nblk; b += 64) { mx = fmax(mx, dpart[2 * b]); ss += dpart[2 * b + 1]; nf += cpart[b]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mx = fmax(mx, __shfl_xor(mx, o)); nf += __shfl_xor(nf, o); }
  ss = wave_sum_d(ss);
  if (threadIdx.x == 0) { dout[0] = mx; dout[1] = ss; cout[0] = nf; }
}

// ----------------------------------------------------------------------------------------------
// The lane map of a bf16 row.  A lane loads at least 4 bytes (two bf16) wherever the row has them:
//   KP = 1       2-byte loads, 64 rows per wave-wide load
//   KP = 2 .. 64 4-byte loads, KP / 2 lanes per row (k = 64: a 128-byte row on 32 lanes, two rows per wave-wide load)
//   KP >= 128    one row per wavefront, 2 * VEC bytes per lane (VEC = KP / 64)
// U: load rounds in flight, chosen so that a round asks for as many ROWS as row_sums does of RowsF32 (EPI * U = 8 * Map<KP>::EPI).
// Lane l of a row's LPR lanes holds elements [l * VEC, l * VEC + VEC); lanes beyond the row's rs elements read zeros.
// ----------------------------------------------------------------------------------------------
#ifndef FMX_COMPACT_ROUND
#define FMX_COMPACT_ROUND 1      // rows a round asks for, in units of RowsF32's (experiments: -DFMX_COMPACT_ROUND=2)
#endif
template <int KP> struct MapC {
  static constexpr int VEC = (KP >= 128) ? KP / 64 : (KP >= 2 ? 2 : 1);
  static constexpr int LPR = KP / VEC;
  static constexpr int EPI = 64 / LPR;
  static constexpr int U = FMX_COMPACT_ROUND * 8 * Map<KP>::EPI / EPI;
};

// VEC bf16 of a snapshot row -> fp32: the low half of a dword is shifted up, the high half masked (non-temporal like the fp32 gather:
// FMX_V_NT bit 4)
template <int VEC> __device__ __forceinline__ void row_ld_c(const CTab& ct, size_t id, uint32_t off, float (&out)[VEC]) {
  if (off < ct.rs) {
    const uint16_t* p = ct.V + id * ct.rs + off;
    if constexpr (VEC == 1) {
      const uint16_t t = (FMX_V_NT & 4) ? __builtin_nontemporal_load(p) : *p;
      out[0] = __uint_as_float((uint32_t)t << 16);
    } else {
      constexpr int NW = VEC / 2;                                        // dwords of the lane
      uint32_t u[NW];
      if constexpr (NW == 1) {
        u[0] = (FMX_V_NT & 4) ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p)) : *reinterpret_cast<const uint32_t*>(p);
      } else if constexpr (NW == 2) {
        typedef uint32_t v2u __attribute__((ext_vector_type(2)));
        const v2u t = (FMX_V_NT & 4) ? __builtin_nontemporal_load(reinterpret_cast<const v2u*>(p)) : *reinterpret_cast<const v2u*>(p);
        u[0] = t.x; u[1] = t.y;
      } else {
        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int c = 0; c < NW / 4; c++) {
          const v4u t = (FMX_V_NT & 4) ? __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p) + c) : reinterpret_cast<const v4u*>(p)[c];
          u[4 * c] = t.x; u[4 * c + 1] = t.y; u[4 * c + 2] = t.z; u[4 * c + 3] = t.w;
        }
      }
#pragma unroll
      for (int c = 0; c < NW; c++) { out[2 * c] = __uint_as_float(u[c] << 16); out[2 * c + 1] = __uint_as_float(u[c] & 0xFFFF0000u); }
    }
  } else {
#pragma unroll
    for (int v = 0; v < VEC; v++) out[v] = 0.f;
  }
}

// The snapshot as a row source of row_sums / k_rowsums / k_fetch_rows (fmx_kernels.h "ROW SOURCE"): MapC's lanes and rounds, row_ld_c,
// and w out of its own array (no side stream; the snapshot is unsharded, so feature id = row).
struct RowsBf16 {
  template <int KP> using Lanes = MapC<KP>;
  CTab ct;
  template <int VEC> __device__ __forceinline__ void ld(size_t id, uint32_t off, float (&out)[VEC]) const { row_ld_c<VEC>(ct, id, off, out); }
  __device__ __forceinline__ float w1(size_t row) const { return load_w(ct.w + row); }
  __device__ __forceinline__ float v1(size_t row, int f) const { return __uint_as_float((uint32_t)ct.V[row * ct.rs + f] << 16); }
  __device__ __forceinline__ float lin(uint32_t id, uint64_t, uint32_t) const { return w1((size_t)id); }
};

}  // namespace fmx
