// fmx_compact_kernels.h -- kernels of the serving snapshots (fmx_compact.hip; include/fmx.h "fmx_compact_*"; DESIGN.md sections 19, 21).
// bf16 first; the int8 row-wise format (k_compact_quant8, RowsI8) is the second half of the file; the pruned snapshot (the rank
// directory, its build kernels and the two sources that read through it) is the last part.
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

// The rank directory of a pruned snapshot: one 8-byte pair per 32 consecutive ids, x = bits (bit b: id 32 j + b is
// kept), y = base (kept ids below 32 j).  ONE 8-byte load answers "is it kept" and "where": slot = base + popc(bits below b).  The pair
// is read as one 64-bit value and both halves are used before anything is decided, so the load stays one global_load_dwordx2 and the
// result is a select, not a branch: DIR_NONE for a dropped id.
constexpr uint32_t DIR_NONE = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t dir_slot(const uint2* __restrict__ dir, size_t id) {
  const unsigned long long p = reinterpret_cast<const unsigned long long*>(dir)[id >> 5];
  const uint32_t bits = (uint32_t)p, base = (uint32_t)(p >> 32), b = (uint32_t)id & 31u;
  const uint32_t slot = base + (uint32_t)__popc(bits & ((1u << b) - 1u));
  return ((bits >> b) & 1u) ? slot : DIR_NONE;
}
__device__ __forceinline__ bool dir_lookup(const uint2* __restrict__ dir, size_t id, size_t& slot) {
  const uint32_t s = dir_slot(dir, id);
  slot = (size_t)s;
  return s != DIR_NONE;
}

constexpr uint32_t COMPACT_BLOCKS = 8192;    // cap of k_compact_quant's grid; a fixed function of the table (compact_grid)

// L lanes (a power of two <= 64) share a feature and stride over its rs elements, 64 / L features per wavefront round (the map of
// k_param_sparsity): 64 consecutive floats per wave-wide load for every k.  The padding (f >= k) is written as +0 and is not counted.
//   dpart[2 * b + {0: max |v - q(v)|, 1: sum (v - q(v))^2}] over the finite q(v), cpart[b] = non-finite q(v)
// v - q(v) is exact in fp32 (q(v) is within half an ulp_bf16 of v: Sterbenz), so the maximum does not depend on the order.
// MAPPED (the pruned snapshot): row j goes to its slot of `dir` and takes w[j] along to wout[slot]; a dropped row is neither read nor
// counted.  The blocks own the same ids either way, so the partials keep their order.
template <bool MAPPED>
static __global__ void __launch_bounds__(256)
k_compact_quant(const float* __restrict__ V, uint32_t rs, uint64_t n, int k, uint32_t L, uint16_t* __restrict__ out,
                double* __restrict__ dpart, unsigned long long* __restrict__ cpart, const uint2* __restrict__ dir,
                const float* __restrict__ w, float* __restrict__ wout) {
  __shared__ double dred[2][4];
  __shared__ unsigned long long cred[4];
  const uint32_t lane = threadIdx.x & 63u, grp = lane / L, sub = lane % L, rpw = 64u / L;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  float mx = 0.f; double ss = 0.0; unsigned long long nf = 0ull;
  for (uint64_t r0 = wave * rpw; r0 < n; r0 += nwaves * rpw) {
    const uint64_t j = r0 + grp;
    if (j < n) {
      size_t dst = (size_t)j;
      if constexpr (MAPPED) {
        if (!dir_lookup(dir, (size_t)j, dst)) continue;
        if (sub == 0u) wout[dst] = w[j];
      }
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
        out[dst * rs + f] = (uint16_t)q;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o)); nf += __shfl_xor(nf, o); }
  ss = wave_sum_d(ss);
  const uint32_t wv = threadIdx.x >> 6;
  if (lane == 0) { dred[0][wv] = (double)mx; dred[1][wv] = ss; cred[wv] = nf; }
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
  static constexpr bool W_IN_ROW = false;
  template <int KP> using Lanes = MapC<KP>;
  CTab ct;
  template <int VEC> __device__ __forceinline__ void ld(size_t id, uint32_t off, float (&out)[VEC]) const { row_ld_c<VEC>(ct, id, off, out); }
  __device__ __forceinline__ float w1(size_t row) const { return load_w(ct.w + row); }
  __device__ __forceinline__ float v1(size_t row, int f) const { return __uint_as_float((uint32_t)ct.V[row * ct.rs + f] << 16); }
  __device__ __forceinline__ float lin(uint32_t id, uint64_t, uint32_t) const { return w1((size_t)id); }
};

// ==============================================================================================
// The int8 row-wise snapshot (FMX_COMPACT_INT8).  ONE aligned block of P bytes per feature holds everything a
// scoring pass wants of it:
//   bytes 0..3  scale (fp32)      bytes 4..7  w_j (fp32)      bytes 8..8+k  the codes q_f (int8), zeros up to P
// P = compact8_row_bytes(k): the power of two >= k + 8 up to 128 (k = 64: 72 bytes in one 128-byte line; k = 32: 40 in one 64-byte
// sector), k + 8 rounded up to 64 above.  There is no w array.
// Codes: a = max_f |v_f|, q_f = clamp(rint(v_f * (127.0 / a)), -127, 127) in fp64 (ties to even), scale = (float)(a / 127.0); a row
// with a non-finite factor has scale NaN and codes 0.  A factor dequantises to fl32(scale * (float)q_f), one fp32 multiply.
// ==============================================================================================
__host__ __device__ constexpr uint32_t compact8_row_bytes(uint32_t k) {
  uint32_t need = k + 8u, p = 8u;
  if (need > 128u) return (need + 63u) / 64u * 64u;
  while (p < need) p <<= 1;
  return p;
}

constexpr int QUANT8_T = 5;      // dwords of a block per lane of k_compact_quant8, at most: P / 4 <= 272 dwords on 64 lanes (k <= 1024)

// L lanes (a power of two <= 64, L * QUANT8_T >= P / 4) share a feature, 64 / L features per wavefront round.  Lane `sub` holds the dwords
// sub, sub + L, ... of the block: dword 0 is the scale, dword 1 is w_j, dword d >= 2 the codes of factors 4 (d - 2) .. 4 (d - 2) + 3, whose
// fp32 values the lane keeps in registers between the absmax butterfly and the rounding -- V is read once.
//   dpart[2 * b + {0: max |v - deq|, 1: sum (v - deq)^2}] over the finite rows in fp64, cpart[b] = k per row with a non-finite factor
// MAPPED: as k_compact_quant -- the block of row j is written at its slot of `dir`, a dropped row is neither read nor counted.
template <bool MAPPED>
static __global__ void __launch_bounds__(256)
k_compact_quant8(const float* __restrict__ V, const float* __restrict__ w, uint32_t rs, uint64_t n, int k, uint32_t L, uint32_t P,
                 uint8_t* __restrict__ out, double* __restrict__ dpart, unsigned long long* __restrict__ cpart,
                 const uint2* __restrict__ dir) {
  __shared__ double dred[2][4];
  __shared__ unsigned long long cred[4];
  const uint32_t lane = threadIdx.x & 63u, grp = lane / L, sub = lane % L, rpw = 64u / L;
  const uint32_t nd = P / 4u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  double mx = 0.0, ss = 0.0; unsigned long long nf = 0ull;
  for (uint64_t r0 = wave * rpw; r0 < n; r0 += nwaves * rpw) {     // (r0 is wave-uniform: every lane takes part in the butterflies)
    const uint64_t j = r0 + grp;
    bool live = j < n;
    size_t dst = (size_t)j;
    if constexpr (MAPPED) { if (live) live = dir_lookup(dir, (size_t)j, dst); }
    float vals[QUANT8_T][4];
    float amax = 0.f; int bad = 0;
#pragma unroll
    for (int t = 0; t < QUANT8_T; t++) {
      const uint32_t d = sub + (uint32_t)t * L;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int f = 4 * ((int)d - 2) + i;
        float v = 0.f;
        if (live && d >= 2u && d < nd && f < k) v = V[j * rs + (uint32_t)f];
        vals[t][i] = v;
        const float av = fabsf(v);
        if (!(av <= 3.402823466e+38f)) bad = 1;                    // inf or NaN
        amax = fmaxf(amax, av);
      }
    }
    for (uint32_t o = L >> 1; o > 0; o >>= 1) { amax = fmaxf(amax, __shfl_xor(amax, (int)o)); bad |= __shfl_xor(bad, (int)o); }
    const double a = (double)amax;
    const double inv = a > 0.0 ? 127.0 / a : 0.0;
    const float scale = bad ? __uint_as_float(0x7FC00000u) : (float)(a / 127.0);
    if (live) {
      uint32_t* blk = reinterpret_cast<uint32_t*>(out + dst * P);
#pragma unroll
      for (int t = 0; t < QUANT8_T; t++) {
        const uint32_t d = sub + (uint32_t)t * L;
        if (d >= nd) continue;
        uint32_t word = 0u;
        if (d == 0u) word = __float_as_uint(scale);
        else if (d == 1u) word = __float_as_uint(w[j]);
        else if (!bad) {
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int f = 4 * ((int)d - 2) + i;
            if (f < k) {
              const float v = vals[t][i];
              const double q = fmin(fmax(rint((double)v * inv), -127.0), 127.0);
              const int qi = (int)q;
              word |= ((uint32_t)qi & 0xFFu) << (8 * i);
              const float deq = scale * (float)qi;
              const double err = fabs((double)v - (double)deq);
              mx = fmax(mx, err);
              ss += err * err;
            }
          }
        }
        blk[d] = word;
      }
      if (bad && sub == 0u) nf += (unsigned long long)k;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mx = fmax(mx, __shfl_xor(mx, o)); nf += __shfl_xor(nf, o); }
  ss = wave_sum_d(ss);
  const uint32_t wv = threadIdx.x >> 6;
  if (lane == 0) { dred[0][wv] = mx; dred[1][wv] = ss; cred[wv] = nf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    dpart[2 * blockIdx.x + 0] = fmax(fmax(dred[0][0], dred[0][1]), fmax(dred[0][2], dred[0][3]));
    dpart[2 * blockIdx.x + 1] = (dred[1][0] + dred[1][1]) + (dred[1][2] + dred[1][3]);
    cpart[blockIdx.x] = (cred[0] + cred[1]) + (cred[2] + cred[3]);
  }
}

// ----------------------------------------------------------------------------------------------
// The lane map of an int8 block.  A lane loads VEC bytes (8, one dwordx2, up to KP = 256; 16 / 32 above) and owns VEC factor SLOTS; slot v
// of lane f of a row's LPR lanes is byte f * VEC + v of the block, i.e. factor f * VEC + v - 8.  Lane 0 of the row therefore holds the
// header (scale, w_j) in its first 8 bytes -- with VEC = 8 nothing else -- and FL = LPR - 1 .. LPR lanes hold factors:
//   KP      <= 8   16   32   64   128   256   512   1024
//   VEC        8    8    8    8     8     8    16     32
//   LPR        2    4    8   16    32    64    64     64      (the power of two >= (KP + 8) / VEC lanes)
//   EPI       32   16    8    4     2     1     1      1      rows per wave-wide load (k = 64: four 128-byte lines, header and codes at once)
//   U          2    2    2    2     4     8     8      8      rounds in flight: EPI * U = min(8 * Map<KP>::EPI, 64) rows, as RowsF32 asks for
// The map is a function of KP; the block's size P is one of k.  Lanes whose bytes lie at or beyond P (k = 40: P = 64 under KP = 64's
// sixteen lanes) load nothing and hold zeros, like the lanes beyond rs of the other sources.
// ----------------------------------------------------------------------------------------------
constexpr int pow2_ge(int x) { int p = 1; while (p < x) p <<= 1; return p; }
template <int KP> struct MapI8 {
  static constexpr int VEC = (KP <= 256) ? 8 : KP / 32;
  static constexpr int LPR = pow2_ge((KP + 8 + VEC - 1) / VEC);
  static constexpr int EPI = 64 / LPR;
  static constexpr int ROWS = 8 * Map<KP>::EPI < 64 ? 8 * Map<KP>::EPI : 64;   // rows a round asks for (a 64-entry block holds no more)
  static constexpr int U = ROWS / EPI;
  static_assert(LPR <= 64 && LPR * VEC >= KP + 8 && U >= 1, "a row's lanes cover header and codes");
};

template <int VEC> struct RawI8 { uint32_t u[VEC / 4] = {}; };

struct RowsI8 {
  static constexpr bool W_IN_ROW = true;
  static constexpr int FOFF = 8;                                   // bytes of the header in front of the codes
  template <int KP> using Lanes = MapI8<KP>;
  template <int VEC> using Raw = RawI8<VEC>;
  const uint8_t* B; uint32_t P;                                    // the blocks, P bytes each (the snapshot is unsharded: feature id = row)

  // the lane's VEC bytes of block id: ONE non-temporal load (two dwordx4 at VEC = 32), zeros at or beyond P
  template <int VEC> __device__ __forceinline__ void ld_raw(size_t id, uint32_t f, RawI8<VEC>& r) const {
    constexpr int NW = VEC / 4;
    const uint32_t off = f * VEC;
    if (off < P) {
      const uint8_t* p = B + id * P + off;
      if constexpr (NW == 2) {
        typedef uint32_t v2u __attribute__((ext_vector_type(2)));
        const v2u t = (FMX_V_NT & 4) ? __builtin_nontemporal_load(reinterpret_cast<const v2u*>(p)) : *reinterpret_cast<const v2u*>(p);
        r.u[0] = t.x; r.u[1] = t.y;
      } else {
        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int c = 0; c < NW / 4; c++) {
          const v4u t = (FMX_V_NT & 4) ? __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p) + c) : reinterpret_cast<const v4u*>(p)[c];
          r.u[4 * c] = t.x; r.u[4 * c + 1] = t.y; r.u[4 * c + 2] = t.z; r.u[4 * c + 3] = t.w;
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < NW; c++) r.u[c] = 0u;
    }
  }
  // the scale comes from the row's lane 0 by a cross-lane read (no LDS allocation); the header's own 8 slots are not factors: zeros.
  // wj: w_j on the header lane, 0 elsewhere.  Called by all 64 lanes.
  template <int KP, int VEC> __device__ __forceinline__ void unpack(const RawI8<VEC>& r, uint32_t f, float (&out)[VEC], float& wj) const {
    constexpr int LPR = MapI8<KP>::LPR;
    float scale;
    if constexpr (LPR == 64) scale = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)r.u[0], 0));
    else scale = __uint_as_float((uint32_t)__shfl((int)r.u[0], 0, LPR));
    const bool hdr = f == 0u;
    wj = hdr ? __uint_as_float(r.u[1]) : 0.f;
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      const int q = (int)(int8_t)(r.u[v / 4] >> (8 * (v % 4)));
      const float x = scale * (float)q;
      out[v] = (v < FOFF && hdr) ? 0.f : x;
    }
  }
  __device__ __forceinline__ float w1(size_t row) const { return *reinterpret_cast<const float*>(B + row * P + 4); }
  __device__ __forceinline__ float v1(size_t row, int f) const {
    const uint8_t* p = B + row * P;
    return *reinterpret_cast<const float*>(p) * (float)(int)(int8_t)p[FOFF + f];
  }
};

// ==============================================================================================
// The pruned snapshot (fmx_compact_begin_pruned): only the features that can contribute to a score keep a row.
// Rows stand in ascending id order ("slots"); the rank directory (dir_lookup above) maps a feature id to its slot.
// Build: k_prune_live (one pass over w and V) -> [k_prune_mark over a slot's entries] -> k_prune_keep (AND, popcounts) -> an exclusive
// scan of the popcounts (hipcub) -> k_prune_dir; then the quantisers above with MAPPED.
// ==============================================================================================

// bits[j] bit b = feature 32 j + b is NOT dead: one of its k factors is != 0.0f (NaN is, -0 is not), or k1 and w_j != 0.0f
// (fmx_param_sparsity's dead_features rule, negated).  One wavefront per word: the 32 rows are one contiguous run of V, read with
// wave-wide loads for every rs; each lane ORs the rows it met, a butterfly ORs the lanes.  Bits at or beyond n are 0.
// *dead += the dead features: integer sums, one block reduction through LDS and one 64-bit integer atomic per block.
static __global__ void __launch_bounds__(256)
k_prune_live(const float* __restrict__ V, const float* __restrict__ w, uint32_t rs, uint64_t n, int k, int k1,
             uint32_t* __restrict__ bits, unsigned long long* __restrict__ dead) {
  __shared__ unsigned long long cred[4];
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t nwords = (n + 31u) / 32u;
  unsigned long long nd = 0ull;
  for (uint64_t j = wave; j < nwords; j += nwaves) {                 // (j is wave-uniform: every lane takes part in the butterfly)
    const uint64_t id0 = j * 32u;
    const uint32_t cnt = (uint32_t)min((uint64_t)32u, n - id0);
    uint32_t nz = 0u;
    if (k > 0) {
      const float* p = V + id0 * rs;
      const uint32_t tot = cnt * rs;
      for (uint32_t e = lane; e < tot; e += 64u) {
        const uint32_t r = e / rs, f = e - r * rs;
        if (f < (uint32_t)k && !(p[e] == 0.0f)) nz |= 1u << r;
      }
    }
    if (k1 && lane < cnt && !(w[id0 + lane] == 0.0f)) nz |= 1u << lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nz |= (uint32_t)__shfl_xor((int)nz, o);
    const uint32_t valid = cnt == 32u ? 0xFFFFFFFFu : ((1u << cnt) - 1u);
    if (lane == 0u) { bits[j] = nz; nd += (unsigned long long)__popc(~nz & valid); }
  }
  const uint32_t wv = threadIdx.x >> 6;
  if (lane == 0u) cred[wv] = nd;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = (cred[0] + cred[1]) + (cred[2] + cred[3]);
    if (t) atomicAdd(dead, t);
  }
}

// seen[id / 32] |= 1 << id % 32 for every entry of a slot's stream: integer atomics, so the result does not depend on the order.  A word
// that already holds the bit is left alone (the bits only ever get set, so a stale read costs one atomic and nothing else).
static __global__ void __launch_bounds__(256)
k_prune_mark(const Entry* __restrict__ ent, uint64_t nnz, uint64_t n, uint32_t* __restrict__ seen) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += stride) {
    const uint32_t id = ent[i].id;
    if (id >= n) continue;
    const uint32_t m = 1u << (id & 31u);
    uint32_t* p = seen + (id >> 5);
    if (!(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m)) atomicOr(p, m);
  }
}

// bits[j] &= seen[j] (seen may be null: everything counts as seen), cnt[j] = popc(bits[j]), *unseen += the live features that went
static __global__ void __launch_bounds__(256)
k_prune_keep(uint32_t* __restrict__ bits, const uint32_t* __restrict__ seen, uint64_t nwords, uint32_t* __restrict__ cnt,
             unsigned long long* __restrict__ unseen) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long nu = 0ull;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nwords; j += stride) {
    const uint32_t live = bits[j];
    const uint32_t keep = seen ? (live & seen[j]) : live;
    nu += (unsigned long long)__popc(live & ~keep);
    bits[j] = keep;
    cnt[j] = (uint32_t)__popc(keep);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nu += __shfl_xor(nu, o);
  if ((threadIdx.x & 63u) == 0u && nu) atomicAdd(unseen, nu);
}

static __global__ void __launch_bounds__(256)
k_prune_dir(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ base, uint64_t nwords, uint2* __restrict__ dir) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nwords; j += stride) dir[j] = make_uint2(bits[j], base[j]);
}

// fmx_compact_slot_of: the slot of each id, 0xFFFFFFFF for a dropped one
static __global__ void __launch_bounds__(256)
k_prune_slot_of(const uint2* __restrict__ dir, const uint32_t* __restrict__ ids, uint32_t count, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  size_t slot;
  out[t] = dir_lookup(dir, (size_t)ids[t], slot) ? (uint32_t)slot : 0xFFFFFFFFu;
}

// The pruned snapshots as row sources.  Each wraps the dense source of its format and differs in ONE thing: a feature id goes through
// the directory first.  They set MAP_IDS (fmx_kernels.h "ROW SOURCE"): row_sums hands every entry's id to map() on the lane that
// loaded the entry -- up to 64 independent 8-byte lookups in flight per block of entries, one extra memory latency per 64 entries, to a
// table of a few MB that lives in the caches -- and broadcasts the SLOT where the other sources broadcast the id.  ld_raw / ld / lin
// therefore take a slot (or DIR_NONE) and issue no lookup: a kept row is loaded from its slot exactly as the dense source loads row id;
// a dropped id issues no row load and yields what a stored row of +0 with w_j = +0 yields -- int8: an all-zero block, which unpack
// multiplies as it does a stored one (scale +0, codes 0); bf16: +0 factors and +0.f from lin -- so everything downstream runs on the
// same bits.  w1 / v1 (k_fetch_rows) take a feature id and look it up themselves.
struct RowsI8P {
  static constexpr bool W_IN_ROW = true;
  static constexpr bool MAP_IDS = true;
  static constexpr int FOFF = RowsI8::FOFF;
  template <int KP> using Lanes = MapI8<KP>;
  template <int VEC> using Raw = RawI8<VEC>;
  RowsI8 rows; const uint2* dir;
  __device__ __forceinline__ uint32_t map(uint32_t id) const { return dir_slot(dir, (size_t)id); }
  template <int VEC> __device__ __forceinline__ void ld_raw(size_t slot, uint32_t f, RawI8<VEC>& r) const {
    if ((uint32_t)slot != DIR_NONE) rows.template ld_raw<VEC>(slot, f, r);
    else r = RawI8<VEC>();
  }
  template <int KP, int VEC> __device__ __forceinline__ void unpack(const RawI8<VEC>& r, uint32_t f, float (&out)[VEC], float& wj) const {
    rows.template unpack<KP, VEC>(r, f, out, wj);
  }
  __device__ __forceinline__ float w1(size_t row) const { size_t slot; return dir_lookup(dir, row, slot) ? rows.w1(slot) : 0.f; }
  __device__ __forceinline__ float v1(size_t row, int f) const { size_t slot; return dir_lookup(dir, row, slot) ? rows.v1(slot, f) : 0.f; }
};

struct RowsBf16P {
  static constexpr bool W_IN_ROW = false;
  static constexpr bool MAP_IDS = true;
  template <int KP> using Lanes = MapC<KP>;
  RowsBf16 rows; const uint2* dir;
  __device__ __forceinline__ uint32_t map(uint32_t id) const { return dir_slot(dir, (size_t)id); }
  template <int VEC> __device__ __forceinline__ void ld(size_t slot, uint32_t off, float (&out)[VEC]) const {
    if ((uint32_t)slot != DIR_NONE) rows.template ld<VEC>(slot, off, out);
    else {
#pragma unroll
      for (int v = 0; v < VEC; v++) out[v] = 0.f;
    }
  }
  __device__ __forceinline__ float w1(size_t row) const { size_t slot; return dir_lookup(dir, row, slot) ? rows.w1(slot) : 0.f; }
  __device__ __forceinline__ float v1(size_t row, int f) const { size_t slot; return dir_lookup(dir, row, slot) ? rows.v1(slot, f) : 0.f; }
  __device__ __forceinline__ float lin(uint32_t slot, uint64_t, uint32_t) const { return slot != DIR_NONE ? rows.w1((size_t)slot) : 0.f; }
};

}  // namespace fmx
