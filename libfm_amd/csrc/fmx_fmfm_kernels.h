// fmx_fmfm_kernels.h -- the field-matrixed FM (FmFM, Sun et al., WWW 2021; include/fmx.h "fmx_fmfm_*").
//
//   y(x) = w0 + sum_j w_j x_j + sum_{a<b} x_a x_b  v_ja^T M[g(ja)][g(jb)] v_jb
//
// g() is the handle's feature -> field map, M[g][h] a k x k matrix with M[h][g] = M[g][h]^T and M[g][g] = I (not learned).  Per example
// the field sums S_g = sum_{i in g} v_i x_i, side by side, are one vector s of W = F KP floats (field g at columns g KP), D = sum_i
// |v_i x_i|^2, and with the symmetric W x W matrix MM of all blocks
//     t = MM s          pair term = 1/2 <s, t> - 1/2 D          d/dv_i = x_i (t_g(i) - v_i x_i)          d/dM[g][h] = S_g S_h^T  (g < h)
// Over a batch these are two plain GEMMs: T = S MM (M = nb, N = K = WP) and G = S^T diag(mult) S (M = N = WP, K = nb), both on the f32
// matrix units (v_mfma_f32_16x16x4_f32: exact f32 products, a fixed k order), workgroup-tiled and staged through double-buffered LDS.
// WP = W rounded up to 16; S, T are [nb][WP], MM32 (the fp32 copy of MM) is [WP][WP]; all padding is zero and contributes nothing.
// No float atomics: a field row of an example is built by the one wavefront that owns the example, entries in row order; every output
// element of a GEMM belongs to one wavefront, which walks K in order; the K split of G is a function of nb alone (FMFM_MCHUNK,
// FMFM_MSPLIT) and its partials are summed in order.  Two runs give the same bits, and no result depends on a grid size.
#pragma once
#include "fmx_adapt_kernels.h"

namespace fmx {

constexpr uint32_t FMFM_MAX_FIELDS = 64, FMFM_MAX_FACTORS = 128, FMFM_MAX_WP = 2048;
constexpr uint32_t FMFM_BM = 64;           // examples per workgroup tile of k_fmfm_gemm_t (16 per wavefront)
constexpr uint32_t FMFM_BN = 64;           // columns per tile of both GEMMs
constexpr uint32_t FMFM_BK = 16;           // K per LDS stage of both GEMMs (four MFMA steps)
constexpr uint32_t FMFM_LDB = 80;          // floats between two k rows of a k-major LDS stage: 16 (mod 64), see the bank argument below
constexpr uint32_t FMFM_MCHUNK = 128;      // examples per chunk of k_fmfm_mgrad's K dimension: a constant, so the sum's association never depends on the grid
constexpr uint32_t FMFM_MSPLIT = 8;        // partials of k_fmfm_mgrad: partial p sums the chunks p, p + 8, p + 16, ... in order
using fm_f32x4 = __attribute__((ext_vector_type(4))) float;

template <int KP> struct FmfmU { static constexpr int value = (KP <= 64) ? 8 : 4; };     // row loads in flight per lane group

// ----------------------------------------------------------------------------------------------
// k_fmfm_sums: the gather.  One wavefront (one workgroup) per example, grid-strided.  Dynamic LDS: the example's field rows, F KP floats
// (rounded up to 4).  The row's V rows and w_j arrive through the Tab / row_ld lane map of row_sums (U rounds of EPI rows in flight);
// every entry's x v is added into row g(id) of the tile, its |x v|^2 into the lane's share of D, entries in row order.  The EPI entries
// of one round that fall into the SAME field are serialised by k_fwfm_rows' rule: a lane group counts the earlier groups of its round
// with its field (c) and adds in pass c; passes are separated by a barrier (the workgroup is the wavefront).  Different fields never
// share an address.  Stored: S_e (WP floats, zeros from F KP on), D_e and the linear part L_e -- scoring and training need the same
// three, so the kernel has one form.  FOLD is the DeepFM's gather (fmx_dfm.hip; a compile-time switch, false for the FmFM): the tile
// holds all field rows when the row ends, and the wavefront also sums them into Stot_e (KP floats, lane c column c, fields ascending),
// which goes to Dg ([rows][KP]) in place of D_e, and stores base_e = L_e + 1/2 |Stot_e|^2 - 1/2 D_e in Lg in place of L_e (a lane's
// columns squared in ascending order, then wave_sum_dpp).
// ----------------------------------------------------------------------------------------------
template <int KP, bool FOLD = false>
__global__ void __launch_bounds__(64)
k_fmfm_sums(const Entry* __restrict__ ent, const uint64_t* __restrict__ row_ptr, uint64_t row0, uint32_t n_rows, const Tab tb,
            const uint32_t* __restrict__ grp, uint32_t F, uint32_t WP, int k1, float* __restrict__ Sg, float* __restrict__ Dg,
            float* __restrict__ Lg) {
  constexpr int VEC = Map<KP>::VEC, LPR = Map<KP>::LPR, EPI = Map<KP>::EPI, U = FmfmU<KP>::value;
  extern __shared__ __align__(16) float fmfm_tile[];
  float* tile = fmfm_tile;
  const uint32_t W = F * KP, W4 = (W + 3u) & ~3u;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = lane / LPR, f = lane % LPR;

  for (uint32_t e = blockIdx.x; e < n_rows; e += gridDim.x) {
    for (uint32_t t = lane * 4u; t < W4; t += 256u) *reinterpret_cast<float4*>(tile + t) = make_float4(0.f, 0.f, 0.f, 0.f);
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
          float d[VEC];
#pragma unroll
          for (int v = 0; v < VEC; v++) { d[v] = vr[u][v] * x; dl = fmaf(d[v], d[v], dl); }     // (an entry beyond the row has d == 0)
          float* srow = tile + fld * KP + f * VEC;
          if constexpr (EPI == 1) {
            if (valid) {                                          // (wave-uniform: one entry per round)
#pragma unroll
              for (int v = 0; v < VEC; v++) srow[v] += d[v];
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
              }
              __syncthreads();                                    // (the loop condition is wave-uniform, and the wavefront IS the workgroup:
            }                                                     //  __launch_bounds__(64) here and dim3(64) in the launch go together)
          }
        }
      }
    }
    __syncthreads();
    for (uint32_t t = lane; t < WP; t += 64u) Sg[(size_t)e * WP + t] = t < W ? tile[t] : 0.f;
    lin = wave_sum_dpp(lin);
    dl = wave_sum_dpp(dl);
    if constexpr (FOLD) {
      float sq = 0.f;
      for (uint32_t c = lane; c < (uint32_t)KP; c += 64u) {
        float stot = 0.f;
        for (uint32_t fg = 0; fg < F; fg++) stot += tile[fg * KP + c];
        Dg[(size_t)e * KP + c] = stot;
        sq = fmaf(stot, stot, sq);
      }
      sq = wave_sum_dpp(sq);
      if (lane == 0) Lg[e] = fmaf(0.5f, sq, fmaf(-0.5f, dl, lin));
    } else {
      if (lane == 0) { Lg[e] = lin; Dg[e] = dl; }
    }
    __syncthreads();
  }
}

// ----------------------------------------------------------------------------------------------
// The MFMA shapes of both GEMMs.  v_mfma_f32_16x16x4_f32: lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15], and register q of the
// accumulator is C[4 (l >> 4) + q][l & 15].  A wavefront owns 16 rows and the FMFM_BN = 64 columns of the workgroup's tile: four
// accumulators, and per MFMA step one A fragment against four B fragments.
//
// LDS stages and their banks (64 banks of 4 bytes; a wavefront's ds_read_b32 is conflict-free when its 64 words fall on 64 different
// banks, and then also when the unit takes it as two halves of 32 lanes over 32 banks, provided each half's words differ mod 32):
//   k-major stage  X[k][c], k < 16, row stride FMFM_LDB = 80 floats.  A fragment of step kk reads word (4 kk + (l >> 4)) 80 + c0 + (l & 15):
//                  mod 64 that is 16 (l >> 4) + (l & 15) + const = l + const -- 64 consecutive banks; lanes 0..31 alone: 32 consecutive
//                  banks mod 32.  This is every B fragment (MM32 rows, S rows of k_fmfm_mgrad) and k_fmfm_mgrad's A fragment (S^T).
//   row-major stage of k_fmfm_gemm_t's A (S rows): Y[kk][row][4], kk < 4, row < 64.  The fragment of step kk reads word
//                  256 kk + 4 (16 w + (l & 15)) + (l >> 4): with r = l & 15, j = l >> 4 the 64 values 4 r + j are 0 .. 63 once each.
//   Stage writes are one aligned float4 per thread.  The k-major stages are written row by row, consecutive threads on consecutive
//   float4s: conflict-free.  The row-major A stage of k_fmfm_gemm_t is NOT: four consecutive threads hold the four float4s of one S row's
//   64 bytes (so the global load is 64 contiguous bytes per row) and write them 256 words apart, onto the same banks -- a 4-way
//   conflict on one ds_write_b128 per thread and stage, against 20 conflict-free fragment reads; a wavefront's global load touches 16 rows.
// Double buffering: two stages of each operand; while the MFMAs of step s read stage s & 1, the global loads of step s + 1 are in
// flight in registers and are written to the other stage after the MFMAs -- one barrier per K step of 16.
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ void gemm_stage_mma(const float* __restrict__ Af, uint32_t a_kk_stride, const float* __restrict__ Bf, fm_f32x4 (&acc)[4]) {
  // Af: the lane's A word of step 0, a_kk_stride floats between steps; Bf: the lane's B word of step 0 and column block 0 (k-major)
#pragma unroll
  for (int kk = 0; kk < 4; kk++) {
    const float a = Af[kk * a_kk_stride];
#pragma unroll
    for (int nt = 0; nt < 4; nt++) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bf[kk * 4 * FMFM_LDB + 16 * nt], acc[nt], 0, 0, 0);
  }
}
__device__ __forceinline__ float4 ld4_or_zero(const float* __restrict__ p, bool ok) {
  return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ----------------------------------------------------------------------------------------------
// k_fmfm_gemm_t: T = S MM32 and rest_e.  A workgroup of four wavefronts owns FMFM_BM = 64 examples (grid-strided over the example tiles)
// and walks ALL column tiles of them, so that rest_e is finished where its T row is formed:
//     rest_e = L_e + 1/2 <S_e, T_e> - 1/2 D_e
// <S_e, T_e>: the lane that holds T[e][c] multiplies it by S[e][c] (column tiles, then column blocks, ascending), the 16 lanes of a row
// are folded by a fixed butterfly.  Per column tile the K loop runs over WP in stages of 16: A = S[e0 .. e0 + 63][k .. k + 15] (row-major
// stage), B = MM32[k .. k + 15][n0 .. n0 + 63] (k-major stage).  Rows beyond nb and columns beyond WP are staged as zeros and never
// stored.  TRAIN: T is stored for the owner; scoring does not need it.
// ----------------------------------------------------------------------------------------------
template <bool TRAIN>
__global__ void __launch_bounds__(256)
k_fmfm_gemm_t(const float* __restrict__ S, const float* __restrict__ MM, const float* __restrict__ Dg, const float* __restrict__ Lg,
              uint32_t nb, uint32_t WP, float* __restrict__ T, float* __restrict__ rest) {
  __shared__ __align__(16) float As[2][FMFM_BK * FMFM_BM];
  __shared__ __align__(16) float Bs[2][FMFM_BK * FMFM_LDB];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, lm = lane & 15u, lk = lane >> 4;
  const uint32_t a_row = tid >> 2, a_kk = tid & 3u;               // staging: S row a_row, floats 4 a_kk .. + 3 of the stage
  const uint32_t b_k = tid >> 4, b_c = 4u * (tid & 15u);          //          MM32 row b_k, columns b_c .. + 3 of the tile
  const uint32_t ntile = (nb + FMFM_BM - 1) / FMFM_BM, nct = (WP + FMFM_BN - 1) / FMFM_BN, nks = WP / FMFM_BK;
  const uint32_t a_dst = a_kk * (4u * FMFM_BM) + a_row * 4u, b_dst = b_k * FMFM_LDB + b_c;
  const uint32_t a_frag = (16u * w + lm) * 4u + lk, b_frag = lk * FMFM_LDB + lm;

  for (uint32_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint32_t e0 = tile * FMFM_BM;
    const bool a_ok = e0 + a_row < nb;
    const float* __restrict__ a_src = S + (size_t)(a_ok ? e0 + a_row : 0u) * WP + 4u * a_kk;
    float dot[4] = {0.f, 0.f, 0.f, 0.f};
    for (uint32_t ct = 0; ct < nct; ct++) {
      const uint32_t n0 = ct * FMFM_BN;
      const bool b_ok = n0 + b_c < WP;
      const float* __restrict__ b_src = MM + (size_t)b_k * WP + (b_ok ? n0 + b_c : 0u);
      fm_f32x4 acc[4];
#pragma unroll
      for (int nt = 0; nt < 4; nt++) acc[nt] = fm_f32x4{0.f, 0.f, 0.f, 0.f};
      float4 ra = ld4_or_zero(a_src, a_ok), rb = ld4_or_zero(b_src, b_ok);
      *reinterpret_cast<float4*>(&As[0][a_dst]) = ra;
      *reinterpret_cast<float4*>(&Bs[0][b_dst]) = rb;
      __syncthreads();
      for (uint32_t ks = 0; ks < nks; ks++) {
        const uint32_t cur = ks & 1u;
        const bool more = ks + 1 < nks;
        if (more) {
          ra = ld4_or_zero(a_src + (size_t)(ks + 1) * FMFM_BK, a_ok);
          rb = ld4_or_zero(b_src + (size_t)(ks + 1) * FMFM_BK * WP, b_ok);
        }
        gemm_stage_mma(&As[cur][a_frag], 4u * FMFM_BM, &Bs[cur][b_frag], acc);
        if (more) {
          *reinterpret_cast<float4*>(&As[cur ^ 1u][a_dst]) = ra;
          *reinterpret_cast<float4*>(&Bs[cur ^ 1u][b_dst]) = rb;
        }
        __syncthreads();
      }
#pragma unroll
      for (int nt = 0; nt < 4; nt++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint32_t row = e0 + 16u * w + 4u * lk + q, col = n0 + 16u * nt + lm;
          if (row < nb && col < WP) {
            dot[q] = fmaf(acc[nt][q], S[(size_t)row * WP + col], dot[q]);
            if (TRAIN) T[(size_t)row * WP + col] = acc[nt][q];
          }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      float d = dot[q];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) d += __shfl_xor(d, o);
      const uint32_t row = e0 + 16u * w + 4u * lk + q;
      if (lm == 0 && row < nb) rest[row] = fmaf(-0.5f, Dg[row], fmaf(0.5f, d, Lg[row]));
    }
  }
}

// ----------------------------------------------------------------------------------------------
// The owner of a (batch, feature) segment: stateful_seg_block with AdagradRule, its sum rows taken from T.  Feature j of field g reads
// T[e][g KP ..] for its occurrence in example e -- T + g KP with a stride of WP floats -- and its own term has the factor 1 (M[g][g] = I).
// ----------------------------------------------------------------------------------------------
struct FmfmSums {
  static constexpr bool PLAIN = false, COLUMN_SELF = false, SECOND = false;
  const float* T; const uint32_t* grp; uint32_t WP;
  __device__ __forceinline__ uint32_t field(uint32_t j) const { return grp ? grp[j] : 0u; }
  template <int KP> __device__ __forceinline__ const float* base(const float*, uint32_t j) const { return T + (size_t)field(j) * KP; }
  __device__ __forceinline__ RowStrideRT stride() const { return RowStrideRT{WP}; }
  __device__ __forceinline__ constexpr float self(uint32_t) const { return 1.f; }
};

template <int KP, int U>
__global__ void __launch_bounds__(256)
k_fmfm_apply_seg(const SegWork sw, const Tab tb, const AdagradRule rule, Hyper h, const FmfmSums sum) {
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t blk = wave0 * 64u; blk < sw.nseg; blk += nwaves * 64u) stateful_seg_block<AdagradRule, KP, U, FmfmSums>(sw, blk, tb, rule, h, sum);
}

// ----------------------------------------------------------------------------------------------
// k_fmfm_mgrad: G = S^T diag(mult) S (M = N = WP, K = nb).  Workgroup (tj, ti, p) of the grid (column tiles, row tiles, partials) forms
// the 64 x 64 tile (ti, tj) of partial p, and only where the tile holds an element of a block g < h: ti <= tj, and the field of the
// tile's first row is below the field of its last column.  K is cut into chunks of FMFM_MCHUNK examples; partial p walks the chunks
// p, p + FMFM_MSPLIT, ... in order, in stages of 16 examples: A = mult_e S[e][r0 .. r0 + 63], B = S[e][c0 .. c0 + 63], both k-major.
// P[p][WP][WP] gets the accumulators; the launch has min(chunks, FMFM_MSPLIT) partials, so each has work.  A few long partials rather
// than none: a tile's owner walking all of nb alone would leave (WP / 64)^2 / 2 workgroups for the whole device (55 at WP = 624) and an
// fp32 sum of nb terms; one partial per chunk would need chunks x WP^2 floats.  Eight bound the buffer at 8 WP^2 floats whatever nb is.
// ----------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_fmfm_mgrad(const float* __restrict__ S, const float* __restrict__ mult, uint32_t nb, uint32_t WP, uint32_t KP, uint32_t F,
             float* __restrict__ P) {
  __shared__ __align__(16) float As[2][FMFM_BK * FMFM_LDB];
  __shared__ __align__(16) float Bs[2][FMFM_BK * FMFM_LDB];
  const uint32_t tj = blockIdx.x, ti = blockIdx.y, p = blockIdx.z;
  const uint32_t r0 = ti * FMFM_BN, c0 = tj * FMFM_BN, W = F * KP;
  if (ti > tj || c0 >= W) return;                                  // (uniform: before any barrier)
  if (r0 / KP >= min(c0 + FMFM_BN - 1, W - 1) / KP) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, lm = lane & 15u, lk = lane >> 4;
  const uint32_t s_ex = tid >> 4, s_c = 4u * (tid & 15u);           // staging: example s_ex of the stage, columns s_c .. + 3 of a tile
  const bool a_ok = r0 + s_c < WP, b_ok = c0 + s_c < WP;
  const uint32_t dst = s_ex * FMFM_LDB + s_c;
  const uint32_t a_frag = lk * FMFM_LDB + 16u * w + lm, b_frag = lk * FMFM_LDB + lm;
  fm_f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; nt++) acc[nt] = fm_f32x4{0.f, 0.f, 0.f, 0.f};
  float4 ra, rb;
  auto load = [&](uint32_t e0) {
    const uint32_t e = e0 + s_ex;
    const bool ok = e < nb;
    const float m = ok ? mult[e] : 0.f;
    const float* __restrict__ row = S + (size_t)(ok ? e : 0u) * WP;
    ra = ld4_or_zero(row + r0 + s_c, ok && a_ok);
    rb = ld4_or_zero(row + c0 + s_c, ok && b_ok);
    ra.x *= m; ra.y *= m; ra.z *= m; ra.w *= m;
  };
  auto next = [](uint32_t e0) {
    e0 += FMFM_BK;
    return (e0 & (FMFM_MCHUNK - 1u)) ? e0 : e0 + (FMFM_MSPLIT - 1u) * FMFM_MCHUNK;
  };
  uint32_t e0 = p * FMFM_MCHUNK, cur = 0;
  load(e0);
  *reinterpret_cast<float4*>(&As[0][dst]) = ra;
  *reinterpret_cast<float4*>(&Bs[0][dst]) = rb;
  __syncthreads();
  for (;;) {
    const uint32_t en = next(e0);
    const bool more = en < nb;
    if (more) load(en);
    gemm_stage_mma(&As[cur][a_frag], 4u * FMFM_LDB, &Bs[cur][b_frag], acc);
    if (more) {
      *reinterpret_cast<float4*>(&As[cur ^ 1u][dst]) = ra;
      *reinterpret_cast<float4*>(&Bs[cur ^ 1u][dst]) = rb;
    }
    __syncthreads();
    if (!more) break;
    e0 = en; cur ^= 1u;
  }
#pragma unroll
  for (int nt = 0; nt < 4; nt++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint32_t row = r0 + 16u * w + 4u * lk + q, col = c0 + 16u * nt + lm;
      if (row < WP && col < WP) P[((size_t)p * WP + row) * WP + col] = acc[nt][q];
    }
}

// k_fmfm_mstep: one thread per element of MM32's upper part; those of a block g < h < F inside the k x k factors step.  The partials in
// order in fp64, L2 once per batch, then
//     n_M += g^2;  M -= eta_m g / sqrt(n_M)
// in fp64 on the session's M and n_M ([F][F][k][k]); the transposed element of M[h][g] and both places of MM32 get the same value.
static __global__ void __launch_bounds__(256)
k_fmfm_mstep(const float* __restrict__ P, uint32_t nsplit, uint32_t F, uint32_t k, uint32_t KP, uint32_t WP,
             double* __restrict__ M, double* __restrict__ nM, float* __restrict__ MM, double eta, double reg) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= WP * WP) return;
  const uint32_t row = t / WP, col = t % WP;
  const uint32_t g = row / KP, a = row % KP, hh = col / KP, b = col % KP;
  if (g >= hh || hh >= F || a >= k || b >= k) return;
  double s = 0.0;
  for (uint32_t p = 0; p < nsplit; p++) s += (double)P[((size_t)p * WP + row) * WP + col];
  const size_t up = (((size_t)g * F + hh) * k + a) * k + b, lo = (((size_t)hh * F + g) * k + b) * k + a;
  const double mv = M[up];
  const double gr = s + reg * mv;
  const double n1 = nM[up] + gr * gr;
  const double mn = mv - eta * gr / sqrt(n1);
  M[up] = mn; M[lo] = mn;
  nM[up] = n1; nM[lo] = n1;
  MM[(size_t)row * WP + col] = (float)mn; MM[(size_t)col * WP + row] = (float)mn;
}

// MM32 [WP][WP] from M [F][F][k][k]: the fp32 copy the kernels read, zero in all padding
static __global__ void __launch_bounds__(256)
k_fmfm_pad_m(const double* __restrict__ M, uint32_t F, uint32_t k, uint32_t KP, uint32_t WP, float* __restrict__ MM) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= WP * WP) return;
  const uint32_t row = t / WP, col = t % WP;
  const uint32_t g = row / KP, a = row % KP, hh = col / KP, b = col % KP;
  MM[t] = (g < F && hh < F && a < k && b < k) ? (float)M[(((size_t)g * F + hh) * k + a) * k + b] : 0.f;
}

}  // namespace fmx
