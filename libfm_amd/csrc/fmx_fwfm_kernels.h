// fmx_fwfm_kernels.h -- the field-weighted FM (include/fmx.h "fmx_fwfm_*").
//
//   y(x) = w0 + sum_j w_j x_j + sum_{i<j} r[g(i)][g(j)] <v_i, v_j> x_i x_j
//
// g() is the handle's feature -> field map, r a symmetric F x F matrix.  Per example the field sums S_g = sum_{i in g} v_i x_i form an
// F x k tile, and everything follows from the one small dense product T = r S:
//     pair term = 1/2 sum_g <S_g, T_g> - 1/2 sum_g r_gg D_g             D_g = sum_{i in g} |v_i|^2 x_i^2
//     d/dv_i    = x_i (T_g(i) - r_g(i)g(i) v_i x_i)
//     d/dr_gh   = <S_g, S_h> (g != h)          d/dr_gg = 1/2 (|S_g|^2 - D_g)
// Both products (T = r S per example, sum_e mult_e S_e S_e^T per batch) run on the f32 matrix units (v_mfma_f32_16x16x4_f32: exact f32
// products, one rounding per fma, a fixed k order).  No float atomics: the tile is built by the one wavefront that owns the example,
// entries of one field in row order; the partials of the r gradient are summed in chunk order.  Two runs give the same bits.
//
// Shapes: FP = F rounded up to 16 (FT = FP / 16 MFMA row blocks, at most 4), KN = max(KP, 16) columns of the LDS tile (the MFMA's N).
// Padded rows and columns of r and S are zero and contribute nothing.  LDS: (FP * KN + FP) * 4 bytes per wavefront -- 33 024 at
// F = 64, k = 128: four one-wavefront workgroups per CU.  Scratch per batch: nb * FP * (2 KP + 1) * 4 bytes (T, S, D).
#pragma once
#include "fmx_adapt_kernels.h"

namespace fmx {

constexpr uint32_t FWFM_RCHUNK = 64;       // examples per partial of k_fwfm_rgrad: a constant, so the sum's association never depends on the grid
using fw_f32x4 = __attribute__((ext_vector_type(4))) float;

template <int KP> struct FwfmU { static constexpr int value = (KP <= 64) ? 8 : 4; };     // row loads in flight per lane group

// sum over the LPR lanes that hold one row (lane bits below log2(LPR)); every lane of the group gets the total
template <int LPR> __device__ __forceinline__ float rowgroup_sum(float x) {
#pragma unroll
  for (int o = 1; o < LPR; o <<= 1) x += __shfl_xor(x, o);
  return x;
}

// ----------------------------------------------------------------------------------------------
// k_fwfm_rows: one wavefront (one workgroup) per example, grid-strided.
//   1. the row's V rows and w_j arrive through the Tab / row_ld lane map of row_sums (U rounds of EPI rows in flight); every entry's
//      v x is added into row g(id) of the LDS tile S[FP][KN], its |v x|^2 into D[FP], entries in row order.  The EPI entries of one
//      round that fall into the SAME field are serialised: a lane group counts the earlier groups of its round with its field (c) and
//      adds in pass c; passes are separated by a barrier (the workgroup is the wavefront).  Different fields never share an address.
//   2. T = r S: M = FP, N = KN, K = FP.  A (r) fragments: lane l holds r[16 mt + (l & 15)][4 kk + (l >> 4)], loaded once per
//      wavefront; B (S) from LDS: S[4 kk + (l >> 4)][16 nt + (l & 15)]; C/D: lane l, register q = T[16 mt + 4 (l >> 4) + q][16 nt + (l & 15)].
//      One column block nt at a time, so FT accumulators are live.
//   3. rest_e = lin + 1/2 sum T o S - 1/2 sum_g r_gg D_g: every lane's share in a fixed order, then the DPP reduction of k_rowsums.
//   TRAIN: T, S ([nb][FP][KP]) and D ([nb][FP]) are stored for the owner and the r gradient.
// ----------------------------------------------------------------------------------------------
template <int KP, int FT, bool TRAIN>
__global__ void __launch_bounds__(64)
k_fwfm_rows(const Entry* __restrict__ ent, const uint64_t* __restrict__ row_ptr, uint64_t row0, uint32_t n_rows, const Tab tb,
            const uint32_t* __restrict__ grp, const float* __restrict__ R, int k1, float* __restrict__ rest,
            float* __restrict__ Tg, float* __restrict__ Sg, float* __restrict__ Dg) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR, EPI = Map<KP>::EPI, U = FwfmU<KP>::value;
  constexpr int FP = 16 * FT, KN = KP < 16 ? 16 : KP, NT = KN / 16, KS = FP / 4;
  __shared__ __align__(16) float tile[FP * KN + FP];
  float* Sl = tile;
  float* Dl = tile + FP * KN;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = lane / LPR, f = lane % LPR;
  const uint32_t lm = lane & 15u, lk = lane >> 4;

  float rf[FT][KS];
#pragma unroll
  for (int mt = 0; mt < FT; mt++)
#pragma unroll
    for (int kk = 0; kk < KS; kk++) rf[mt][kk] = R[(16 * mt + lm) * FP + 4 * kk + lk];
  const float rdiag = lane < (uint32_t)FP ? R[lane * FP + lane] : 0.f;

  for (uint32_t e = blockIdx.x; e < n_rows; e += gridDim.x) {
    for (int t = (int)lane * 4; t < FP * KN + FP; t += 256) *reinterpret_cast<float4*>(tile + t) = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    const uint64_t a = row_ptr[row0 + e];
    const uint32_t size = (uint32_t)(row_ptr[row0 + e + 1] - a);
    const Entry* __restrict__ re = ent + a;
    float lin = 0.f;
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
          if (idx < cnt) row_ld<VEC, 4>(tb, (size_t)id, f * VEC, vr[u]);
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
          float d[VEC], q = 0.f;
#pragma unroll
          for (int v = 0; v < VEC; v++) { d[v] = vr[u][v] * x; q = fmaf(d[v], d[v], q); }
          q = rowgroup_sum<LPR>(q);
          float* srow = Sl + fld * KN + f * VEC;
          if constexpr (EPI == 1) {
            if (valid) {                                          // (wave-uniform: one entry per round)
#pragma unroll
              for (int v = 0; v < VEC; v++) srow[v] += d[v];
              if (f == 0) Dl[fld] += q;
            }
          } else {
            uint32_t c = 0;                                       // earlier groups of this round in the same field
#pragma unroll
            for (int gp = 0; gp < EPI; gp++) {
              const uint32_t of = (uint32_t)__shfl((int)fld, gp * LPR);
              const bool ov = i + u * EPI + gp < cnt;
              c += ((uint32_t)gp < g && ov && of == fld) ? 1u : 0u;
            }
            for (uint32_t p = 0; __ballot(valid && c >= p) != 0ull; p++) {
              if (valid && c == p) {
#pragma unroll
                for (int v = 0; v < VEC; v++) srow[v] += d[v];
                if (f == 0) Dl[fld] += q;
              }
              __syncthreads();                                    // (the loop condition is wave-uniform, and the wavefront IS the workgroup:
            }                                                     //  __launch_bounds__(64) here and dim3(64) in FWFM_LAUNCH_1W go together)
          }
        }
      }
    }
    __syncthreads();

    float pair = 0.f;
#pragma unroll 1
    for (int nt = 0; nt < NT; nt++) {
      float b[KS];
#pragma unroll
      for (int kk = 0; kk < KS; kk++) b[kk] = Sl[(4 * kk + lk) * KN + 16 * nt + lm];
#pragma unroll
      for (int mt = 0; mt < FT; mt++) {
        fw_f32x4 acc = fw_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KS; kk++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(rf[mt][kk], b[kk], acc, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint32_t row = 16 * mt + 4 * lk + q, col = 16 * nt + lm;
          pair = fmaf(acc[q], Sl[row * KN + col], pair);
          if (TRAIN && col < (uint32_t)KP) Tg[((size_t)e * FP + row) * KP + col] = acc[q];
        }
      }
    }
    float part = fmaf(0.5f, pair, lin);
    if (lane < (uint32_t)FP) part = fmaf(-0.5f * rdiag, Dl[lane], part);
    part = wave_sum_dpp(part);
    if (lane == 0) rest[e] = part;
    if (TRAIN) {
      for (int t = (int)lane; t < FP * KP; t += 64) Sg[(size_t)e * FP * KP + t] = Sl[(t / KP) * KN + (t % KP)];
      if (lane < (uint32_t)FP) Dg[(size_t)e * FP + lane] = Dl[lane];
    }
    __syncthreads();
  }
}

// ----------------------------------------------------------------------------------------------
// The owner of a (batch, feature) segment: stateful_seg_block with AdagradRule, its sum rows taken from T.  Feature j of field g reads
// row (e FP + g) KP of T for its occurrence in example e -- T + g KP with a stride of FP KP floats -- and its own term carries r_gg.
// ----------------------------------------------------------------------------------------------
struct FwfmSums {
  static constexpr bool PLAIN = false, COLUMN_SELF = false, SECOND = false;
  const float* T; const uint32_t* grp; const float* R;             // R: the fp32 copy [FP][FP]
  uint32_t FP, ex_stride;                                          // ex_stride = FP * KP floats between two examples' T rows
  __device__ __forceinline__ uint32_t field(uint32_t j) const { return grp ? grp[j] : 0u; }
  template <int KP> __device__ __forceinline__ const float* base(const float*, uint32_t j) const { return T + (size_t)field(j) * KP; }
  __device__ __forceinline__ RowStrideRT stride() const { return RowStrideRT{ex_stride}; }
  __device__ __forceinline__ float self(uint32_t j) const { const uint32_t gg = field(j); return R[gg * FP + gg]; }
};

template <int KP, int U>
__global__ void __launch_bounds__(256)
k_fwfm_apply_seg(const SegWork sw, const Tab tb, const AdagradRule rule, Hyper h, const FwfmSums sum) {
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t blk = wave0 * 64u; blk < sw.nseg; blk += nwaves * 64u) stateful_seg_block<AdagradRule, KP, U, FwfmSums>(sw, blk, tb, rule, h, sum);
}

// ----------------------------------------------------------------------------------------------
// k_fwfm_rgrad: the gradient of r as the GEMM sum_e mult_e S_e S_e^T (M = N = FP, K = nb KP).  One wavefront per chunk of FWFM_RCHUNK
// consecutive examples; per example and 16 factors, lane l loads factors 16 ch + 4 (l >> 4) .. + 3 of field row 16 t + (l & 15) of every
// row block t (one float4): the A operand of block mt (scaled by mult_e) and the B operand of block nt see the same factor in every
// step.  Only the blocks mt <= nt are formed.  P[chunk][FP][FP] gets the accumulators, PD[chunk][FP] the chunk's sum_e mult_e D_e.
// ----------------------------------------------------------------------------------------------
template <int KP, int FT>
__global__ void __launch_bounds__(64)
k_fwfm_rgrad(const float* __restrict__ Sg, const float* __restrict__ Dg, const float* __restrict__ mult, uint32_t nb,
             float* __restrict__ P, float* __restrict__ PD) {
  constexpr int FP = 16 * FT;
  constexpr int NSTEP = KP >= 16 ? KP / 16 : 1;                      // loads per example and row block
  const uint32_t lane = threadIdx.x & 63u, lm = lane & 15u, lk = lane >> 4;
  const uint32_t nchunk = (nb + FWFM_RCHUNK - 1) / FWFM_RCHUNK;
  for (uint32_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
    fw_f32x4 acc[FT][FT];
#pragma unroll
    for (int mt = 0; mt < FT; mt++)
#pragma unroll
      for (int nt = 0; nt < FT; nt++) acc[mt][nt] = fw_f32x4{0.f, 0.f, 0.f, 0.f};
    float dacc = 0.f;
    const uint32_t e1 = min(nb, (c + 1) * FWFM_RCHUNK);
    for (uint32_t e = c * FWFM_RCHUNK; e < e1; e++) {
      const float m = mult[e];
      const float* __restrict__ Se = Sg + (size_t)e * FP * KP;
      if (lane < (uint32_t)FP) dacc = fmaf(m, Dg[(size_t)e * FP + lane], dacc);
#pragma unroll 2
      for (int ch = 0; ch < NSTEP; ch++) {
        float fr[FT][4];
#pragma unroll
        for (int t = 0; t < FT; t++) {
          if constexpr (KP >= 16) {
            const float4 v = *reinterpret_cast<const float4*>(Se + (16 * t + lm) * KP + 16 * ch + 4 * lk);
            fr[t][0] = v.x; fr[t][1] = v.y; fr[t][2] = v.z; fr[t][3] = v.w;
          } else {                                                    // k < 16: factor 4 s + (l >> 4) in step s, zeros beyond the row
#pragma unroll
            for (int s = 0; s < 4; s++) fr[t][s] = (4 * s + (int)lk < KP) ? Se[(16 * t + lm) * KP + 4 * s + lk] : 0.f;
          }
        }
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
          for (int mt = 0; mt < FT; mt++) {
            const float am = m * fr[mt][s];
#pragma unroll
            for (int nt = mt; nt < FT; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(am, fr[nt][s], acc[mt][nt], 0, 0, 0);
          }
      }
    }
#pragma unroll
    for (int mt = 0; mt < FT; mt++)
#pragma unroll
      for (int nt = mt; nt < FT; nt++)
#pragma unroll
        for (int q = 0; q < 4; q++) P[((size_t)c * FP + 16 * mt + 4 * lk + q) * FP + 16 * nt + lm] = acc[mt][nt][q];
    if (lane < (uint32_t)FP) PD[(size_t)c * FP + lane] = dacc;
  }
}

// k_fwfm_rstep: one thread per pair g <= h < F.  The partials in chunk order in fp64, the diagonal with D, L2 once per batch, then
//     n_r += g^2;  r -= eta_r g / sqrt(n_r)
// in fp64 on the session's r and n_r ([F][F]); both halves and the kernels' fp32 copy R32 ([FP][FP]) get the same value.
static __global__ void __launch_bounds__(256)
k_fwfm_rstep(const float* __restrict__ P, const float* __restrict__ PD, uint32_t nchunk, uint32_t F, uint32_t FP,
             double* __restrict__ r, double* __restrict__ nr, float* __restrict__ R32, double eta, double reg) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t g = t / FP, hh = t % FP;
  if (g > hh || hh >= F) return;
  double s = 0.0;
  for (uint32_t c = 0; c < nchunk; c++) s += (double)P[((size_t)c * FP + g) * FP + hh];
  if (g == hh) {
    double d = 0.0;
    for (uint32_t c = 0; c < nchunk; c++) d += (double)PD[(size_t)c * FP + g];
    s = 0.5 * (s - d);
  }
  const double rv = r[(size_t)g * F + hh];
  const double gr = s + reg * rv;
  const double n1 = nr[(size_t)g * F + hh] + gr * gr;
  const double rn = rv - eta * gr / sqrt(n1);
  r[(size_t)g * F + hh] = rn; r[(size_t)hh * F + g] = rn;
  nr[(size_t)g * F + hh] = n1; nr[(size_t)hh * F + g] = n1;
  R32[g * FP + hh] = (float)rn; R32[hh * FP + g] = (float)rn;
}

// R32 [FP][FP] from r [F][F]: the fp32 copy the kernels read, zero beyond F
static __global__ void __launch_bounds__(256)
k_fwfm_pad_r(const double* __restrict__ r, uint32_t F, uint32_t FP, float* __restrict__ R32) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= FP * FP) return;
  const uint32_t g = t / FP, hh = t % FP;
  R32[t] = (g < F && hh < F) ? (float)r[(size_t)g * F + hh] : 0.f;
}

}  // namespace fmx
