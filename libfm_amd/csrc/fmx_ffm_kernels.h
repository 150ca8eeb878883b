// fmx_ffm_kernels.h -- the field-aware FM (FFM, Juan et al., RecSys 2016; include/fmx.h "fmx_ffm_*").
//
//   y(x) = w0 + sum_j w_j x_j + sum_{a<b} < v_ja[g(jb)], v_jb[g(ja)] > x_a x_b
//
// g() is the handle's feature -> field map (F fields); a feature's row of W = F kf floats holds one vector of kf factors per field,
// column c = h kf + f being factor f of the vector used against field h.  Per example the field tile
//     Q[h][:] = sum_{b: g(jb) = h} x_b V[jb][:]                      (F x W; Q[h][g] = block g of row h)
// and the own-term mass D = sum_b x_b^2 |v_jb[g(jb)]|^2 give everything:
//     pair term       = 1/2 sum_{g,h} <Q[h][g], Q[g][h]> - 1/2 D
//     d/dv_ja[h]      = x_a (Q[h][g(ja)] - [h = g(ja)] x_a v_ja[g(ja)])
// An occurrence of a feature of field g needs the block-transposed tile row Qt[g] = (Q[0][g], Q[1][g], ..., Q[F-1][g]): W floats.
//
// No matrix instructions: the model has no dense product.  The pair term contracts the tile with its own block transpose -- F W
// multiply-adds per example against nnz W floats gathered -- and the kernel is bound by the gather and the scratch stores.  The work
// that is new here is a data movement: rows arrive in the lane map of row_sums, are summed by field into an LDS tile, and leave through
// a block-transposed LDS read that feeds both the pair term and the coalesced store of Qt.
//
// LDS row stride LD (ffm_row_stride): the transposed read of column c = g kf + f in step h is word g LD + h kf + f.  With
// LD == kf (mod 64) that is c + const (mod 64): the 64 lanes of a wavefront, which hold 64 consecutive c, fall on 64 consecutive words --
// no two on one bank, whether the unit takes the wavefront as one pass over 64 banks or as two halves over 32.  LD is kept a multiple
// of 4 so that the row-wise float4 accumulation stays aligned; where kf is no multiple of 4 the residue is kf rounded up to 4, the
// lanes' words then advance by 1 .. 3 extra per block and at most a few lanes of a wavefront wrap onto an occupied bank (2-way).
// The direct operand Q[h][c] and the accumulation are row-contiguous and conflict-free at any stride.
// No float atomics: the tile is built by the one wavefront that owns the example, entries of one field in row order, and every lane
// walks its positions in a fixed order.  Two runs give the same bits.
#pragma once
#include "fmx_adapt_kernels.h"

namespace fmx {

constexpr uint32_t FFM_MAX_FIELDS = 64;
constexpr uint32_t FFM_MAX_LDS = 160u * 1024u;       // one workgroup's tile: gfx950's LDS per CU

// floats between two rows of the LDS tile: the smallest multiple of 4 that is >= W and == kf rounded up to 4 (mod 64)
inline uint32_t ffm_row_stride(uint32_t W, uint32_t kf) {
  const uint32_t want = ((kf + 3u) & ~3u) & 63u;
  uint32_t ld = (W + 3u) & ~3u;
  ld += (want + 64u - (ld & 63u)) & 63u;
  return ld;
}

template <int KP> struct FfmU { static constexpr int value = (KP <= 64) ? 8 : (KP <= 256) ? 4 : 2; };     // row loads in flight per lane group

// a lane's VEC consecutive floats of one entry's x v added into its field's tile row, in aligned pieces of min(VEC, 4) floats; pieces
// that begin at or beyond LD (columns past the row: they hold zeros) are left out.  LD is a multiple of 4 and so is every piece's start.
template <int VEC> __device__ __forceinline__ void tile_add(float* __restrict__ srow, uint32_t col0, uint32_t LD, const float (&d)[VEC]) {
  if constexpr (VEC == 1) {
    if (col0 < LD) srow[0] += d[0];
  } else if constexpr (VEC == 2) {
    if (col0 < LD) { float2 t = *reinterpret_cast<float2*>(srow); t.x += d[0]; t.y += d[1]; *reinterpret_cast<float2*>(srow) = t; }
  } else {
#pragma unroll
    for (int q = 0; q < VEC / 4; q++)
      if (col0 + 4u * q < LD) {
        float4 t = reinterpret_cast<float4*>(srow)[q];
        t.x += d[4 * q]; t.y += d[4 * q + 1]; t.z += d[4 * q + 2]; t.w += d[4 * q + 3];
        reinterpret_cast<float4*>(srow)[q] = t;
      }
  }
}

// ----------------------------------------------------------------------------------------------
// k_ffm_rows: one wavefront (one workgroup) per example, grid-strided.  Dynamic LDS: the tile, F * LD floats.
//   1. the row's V rows and w_j arrive through the Tab / row_ld lane map of row_sums (U rounds of EPI rows in flight); every entry's
//      x v is added into row g(id) of the tile, entries in row order.  The EPI entries of one round that fall into the SAME field are
//      serialised by k_fwfm_rows' rule: a lane group counts the earlier groups of its round with its field (c) and adds in pass c;
//      passes are separated by a barrier (the workgroup is the wavefront).  D comes from the entry's own block only: the columns
//      with c / kf == field, found without a division as c - field kf < kf.
//   2. positions: lane l owns columns c = t LPR + (l % LPR), t < VEC, of the rows h = h0 + l / LPR (KP >= 64: every row, 64
//      consecutive columns per t; KP < 64: EPI rows per step).  toff[t] = (c / kf) LD + c % kf is computed once per wavefront, and
//      b = tile[toff[t] + h kf] = Q[c / kf][h kf + c % kf] is both the second operand of the pair term (a = Q[h][c]) and
//      Qt[h][c], which TRAIN stores to scratch rows of RW floats (zeros from W to RW): coalesced.
//   3. rest_e = lin + 1/2 pair - 1/2 D: every lane's share in that fixed order, then the DPP reduction of k_rowsums.
// ----------------------------------------------------------------------------------------------
template <int KP, bool TRAIN>
__global__ void __launch_bounds__(64)
k_ffm_rows(const Entry* __restrict__ ent, const uint64_t* __restrict__ row_ptr, uint64_t row0, uint32_t n_rows, const Tab tb,
           const uint32_t* __restrict__ grp, uint32_t F, uint32_t kf, uint32_t LD, uint32_t RW, int k1, float* __restrict__ rest,
           float* __restrict__ Qt) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR, EPI = Map<KP>::EPI, U = FfmU<KP>::value;
  extern __shared__ __align__(16) float ffm_tile[];
  float* tile = ffm_tile;
  const uint32_t W = F * kf;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = lane / LPR, f = lane % LPR;
  const uint32_t col0 = f * VEC;

  uint32_t toff[VEC];
#pragma unroll
  for (int t = 0; t < VEC; t++) {
    const uint32_t c = (uint32_t)t * LPR + f;
    toff[t] = c < W ? (c / kf) * LD + c % kf : 0u;
  }

  for (uint32_t e = blockIdx.x; e < n_rows; e += gridDim.x) {
    for (uint32_t t = lane * 4u; t < F * LD; t += 256u) *reinterpret_cast<float4*>(tile + t) = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    const uint64_t a = row_ptr[row0 + e];
    const uint32_t size = (uint32_t)(row_ptr[row0 + e + 1] - a);
    const Entry* __restrict__ re = ent + a;
    float lin = 0.f, dl = 0.f;
    for (uint32_t base = 0; base < size; base += 64) {
      const uint32_t cnt = min(64u, size - base);
      Entry en; en.id = 0; en.value = 0.f;
      uint32_t fl = 0;
      if (lane < cnt) {
        en = load_stream8(re + base + lane);
        if (k1) lin += load_w(tb.w + (size_t)en.id * tb.ws) * en.value;
        if (grp) fl = grp[en.id];
      }
      for (uint32_t i = 0; i < cnt; i += EPI * U) {
        float vr[U][VEC];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const uint32_t idx = i + u * EPI + g;
          const uint32_t id = bcast_u32<EPI>(en.id, idx & 63u);
          if (idx < cnt) row_ld<VEC, 4>(tb, (size_t)id, col0, vr[u]);
          else {
#pragma unroll
            for (int v = 0; v < VEC; v++) vr[u][v] = 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          const uint32_t idx = i + u * EPI + g;
          const bool valid = idx < cnt;
          const float x = bcast_f32<EPI>(en.value, idx & 63u);
          const uint32_t fld = bcast_u32<EPI>(fl, idx & 63u);
          const uint32_t own0 = fld * kf;
          float d[VEC];
#pragma unroll
          for (int v = 0; v < VEC; v++) {
            d[v] = vr[u][v] * x;
            if (col0 + (uint32_t)v - own0 < kf) dl = fmaf(d[v], d[v], dl);      // (an entry beyond the row has d == 0)
          }
          float* srow = tile + fld * LD + col0;
          if constexpr (EPI == 1) {
            if (valid) tile_add<VEC>(srow, col0, LD, d);             // (wave-uniform: one entry per round)
          } else {
            uint32_t c = 0;                                          // earlier groups of this round in the same field
#pragma unroll
            for (int gp = 0; gp < EPI; gp++) {
              const uint32_t of = (uint32_t)__shfl((int)fld, gp * LPR);
              const bool ov = i + u * EPI + gp < cnt;
              c += ((uint32_t)gp < g && ov && of == fld) ? 1u : 0u;
            }
            for (uint32_t p = 0; __ballot(valid && c >= p) != 0ull; p++) {
              if (valid && c == p) tile_add<VEC>(srow, col0, LD, d);
              __syncthreads();                                       // (the loop condition is wave-uniform, and the wavefront IS the workgroup:
            }                                                        //  __launch_bounds__(64) here and dim3(64) in the launch go together)
          }
        }
      }
    }
    __syncthreads();

    float pair = 0.f;
    for (uint32_t h0 = 0; h0 < F; h0 += EPI) {
      const uint32_t hh = h0 + g;
      const bool hv = hh < F;
#pragma unroll
      for (int t = 0; t < VEC; t++) {
        const uint32_t c = (uint32_t)t * LPR + f;
        float b = 0.f;
        if (hv && c < W) {
          b = tile[toff[t] + hh * kf];
          pair = fmaf(tile[hh * LD + c], b, pair);
        }
        if (TRAIN && hv && c < RW) Qt[((size_t)e * F + hh) * RW + c] = b;
      }
    }
    float part = fmaf(0.5f, pair, lin);
    part = fmaf(-0.5f, dl, part);
    part = wave_sum_dpp(part);
    if (lane == 0) rest[e] = part;
    __syncthreads();
  }
}

// ----------------------------------------------------------------------------------------------
// The owner of a (batch, feature) segment: stateful_seg_block with AdagradRule, its sum rows taken from Qt.  Feature j of field g reads
// row (e F + g) RW of Qt for its occurrence in example e -- Qt + g RW with a stride of F RW floats -- through loads masked to the RW
// floats of a row, and its own term applies to the columns [g kf, (g + 1) kf) alone (the sum source's per-column self factor).
// ----------------------------------------------------------------------------------------------
struct FfmStride {
  uint32_t s, rw;
  template <int KP> __device__ __forceinline__ size_t of() const { return (size_t)s; }
  __device__ __forceinline__ bool live(uint32_t off) const { return off < rw; }
};
struct FfmSums {
  static constexpr bool PLAIN = false, COLUMN_SELF = true, SECOND = false;
  const float* Qt; const uint32_t* grp;
  uint32_t kf, rw, ex_stride;                                      // ex_stride = F * rw floats between two examples' rows
  __device__ __forceinline__ uint32_t field(uint32_t j) const { return grp ? grp[j] : 0u; }
  template <int KP> __device__ __forceinline__ const float* base(const float*, uint32_t j) const { return Qt + (size_t)field(j) * rw; }
  __device__ __forceinline__ FfmStride stride() const { return FfmStride{ex_stride, rw}; }
  __device__ __forceinline__ uint32_t own_begin(uint32_t j) const { return field(j) * kf; }
  __device__ __forceinline__ uint32_t own_width() const { return kf; }
};

template <int KP, int U>
__global__ void __launch_bounds__(256)
k_ffm_apply_seg(const SegWork sw, const Tab tb, const AdagradRule rule, Hyper h, const FfmSums sum) {
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t blk = wave0 * 64u; blk < sw.nseg; blk += nwaves * 64u) stateful_seg_block<AdagradRule, KP, U, FfmSums>(sw, blk, tb, rule, h, sum);
}

}  // namespace fmx
