// fmx_dfm_kernels.h -- DeepFM with one hidden layer (Guo et al., IJCAI 2017; include/fmx.h "fmx_dfm_*").
//
//   y(x) = w0 + sum_j w_j x_j + 1/2 (|sum_g S_g|^2 - D) + <w2, relu(W1^T s + b1)>
//
// g() is the handle's feature -> field map, S_g = sum_{i in g} v_i x_i the field sums, s all of them side by side (W = F KP floats, field
// g at columns g KP, as in fmx_fmfm_kernels.h), D = sum_i |v_i x_i|^2, W1 [F k][H], b1 and w2 [H].  Per example, with the ReLU mask
// `pre-activation > 0`:
//     a = relu(W1^T s + b1)     dh = [a > 0] w2     z = W1 dh     d/dv_i = x_i (Stot + z_g(i) - v_i x_i),  Stot = sum_g S_g
//     d/dW1 = s dh^T            d/db1 = dh          d/dw2 = a
// Over a batch these are three rectangular GEMMs on the f32 matrix units (v_mfma_f32_16x16x4_f32), HP = H rounded up to 16:
//     A = relu(S W1p + b1)        M = nb, N = HP, K = WP       k_dfm_gemm_h, rest_e in its epilogue
//     Z = Dh W1p^T                M = nb, N = WP, K = HP       k_dfm_gemm_z, R = Z + Stot in its epilogue; Dh is formed while staging
//     G = S^T diag(mult) Dh       M = WP, N = HP, K = nb       k_dfm_wgrad, with the rows of g_b1 and g_w2 as two more row tiles
// dy/dS does not depend on the loss multiplier, so the first two run before the bias recurrence and the owner (k_fmfm_apply_seg with
// FmfmSums{R}) multiplies by mult_e per occurrence.  W1p [WP][HP] and W1t [HP][WP] (its transpose), b1p and w2p [HP] are the zero-padded
// fp32 copies the kernels read; the net and its AdaGrad accumulators live in fp64 and step in k_dfm_netstep.
// MFMA shapes, LDS stages and their bank argument are fmx_fmfm_kernels.h's: every B operand here is a k-major stage of FMFM_LDB = 80
// floats per k row (word (4 kk + (l >> 4)) 80 + 16 nt + (l & 15) = l + const mod 64: 64 different banks), the A operand of the two
// example-major GEMMs is the row-major stage Y[kk][row][4] (word 256 kk + 4 (16 w + (l & 15)) + (l >> 4): 4 r + j takes 0 .. 63 once), and
// k_dfm_wgrad's A operand (S^T) is k-major as k_fmfm_mgrad's.  W1p^T is NOT read through a transposing stage: B[kh][n] = W1p[n][kh] taken
// from W1p gives a thread a float4 along k for one column n -- written into the k-major stage that is four words 80 apart, a 4-way
// conflict on every write.  An n-major stage X[n][20] would be conflict-free too (fragment word 20 (l & 15) + (l >> 4): 20 r mod 64 is
// 16 different multiples of 4), but it is a second stage layout, fragment address and K loop.  The transposed copy W1t costs WP HP
// floats, is written by the one thread that steps the element, and makes stage, fragment and K loop k_dfm_gemm_h's: the simpler one.
// No float atomics; every output element belongs to one wavefront, which walks K in order; the K split of G is a function of nb alone
// (FMFM_MCHUNK, FMFM_MSPLIT) and its partials are summed in order; two runs give the same bits.
#pragma once
#include "fmx_fmfm_kernels.h"

namespace fmx {

constexpr uint32_t DFM_MAX_HIDDEN = 512;

// The gather is k_fmfm_sums<KP, true> (fmx_fmfm_kernels.h), its FOLD form: S_e, Stot_e = sum_g S_e[g] ([nb][KP]) and
// base_e = L_e + 1/2 |Stot_e|^2 - 1/2 D_e.

// ----------------------------------------------------------------------------------------------
// One column tile of an example-major GEMM: acc = A'[e0 .. e0 + 63][0 .. 16 nks) B[0 .. 16 nks)[n0 .. n0 + 63], k_fmfm_gemm_t's K loop.
// a_ld(ks) is the thread's float4 of A' for stage ks (row tid >> 2, floats 4 (tid & 3) .. + 3 of the stage's 16): the caller forms A'
// while staging.  b_src is the thread's float4 of B at stage 0 (row tid >> 4 of the stage, columns 4 (tid & 15) .. + 3 of the tile),
// b_step floats between stages.  Double-buffered, one barrier per stage; the last barrier also frees stage 0 for the next tile.
// ----------------------------------------------------------------------------------------------
struct DfmStage { float (*As)[FMFM_BK * FMFM_BM]; float (*Bs)[FMFM_BK * FMFM_LDB]; uint32_t a_dst, b_dst, a_frag, b_frag; };
template <class ALd>
__device__ __forceinline__ void dfm_tile_gemm(const DfmStage& sg, ALd a_ld, const float* __restrict__ b_src, bool b_ok, size_t b_step,
                                              uint32_t nks, fm_f32x4 (&acc)[4]) {
#pragma unroll
  for (int nt = 0; nt < 4; nt++) acc[nt] = fm_f32x4{0.f, 0.f, 0.f, 0.f};
  float4 ra = a_ld(0u), rb = ld4_or_zero(b_src, b_ok);
  *reinterpret_cast<float4*>(&sg.As[0][sg.a_dst]) = ra;
  *reinterpret_cast<float4*>(&sg.Bs[0][sg.b_dst]) = rb;
  __syncthreads();
  for (uint32_t ks = 0; ks < nks; ks++) {
    const uint32_t cur = ks & 1u;
    const bool more = ks + 1 < nks;
    if (more) {
      ra = a_ld(ks + 1);
      rb = ld4_or_zero(b_src + (size_t)(ks + 1) * b_step, b_ok);
    }
    gemm_stage_mma(&sg.As[cur][sg.a_frag], 4u * FMFM_BM, &sg.Bs[cur][sg.b_frag], acc);
    if (more) {
      *reinterpret_cast<float4*>(&sg.As[cur ^ 1u][sg.a_dst]) = ra;
      *reinterpret_cast<float4*>(&sg.Bs[cur ^ 1u][sg.b_dst]) = rb;
    }
    __syncthreads();
  }
}
#define DFM_STAGE_SETUP                                                                                         \
  __shared__ __align__(16) float As[2][FMFM_BK * FMFM_BM];                                                      \
  __shared__ __align__(16) float Bs[2][FMFM_BK * FMFM_LDB];                                                     \
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, lm = lane & 15u, lk = lane >> 4;            \
  const uint32_t a_row = tid >> 2, a_kk = tid & 3u, b_k = tid >> 4, b_c = 4u * (tid & 15u);                     \
  const DfmStage sg{As, Bs, a_kk * (4u * FMFM_BM) + a_row * 4u, b_k * FMFM_LDB + b_c, (16u * w + lm) * 4u + lk, lk * FMFM_LDB + lm}

// ----------------------------------------------------------------------------------------------
// k_dfm_gemm_h: A = relu(S W1p + b1) and rest_e.  A workgroup of four wavefronts owns FMFM_BM = 64 examples (grid-strided over the
// example tiles) and walks ALL column tiles of the hidden layer, so that the score is finished where the row is formed:
//     rest_e = base_e + <a_e, w2>
// the lane that holds a[e][c] multiplies it by w2[c] (column tiles, then column blocks, ascending), the 16 lanes of a row are folded by
// a fixed butterfly.  Hidden units from H on have a zero column of W1p and b1p == 0: pre-activation 0, masked.  TRAIN: A is stored for
// k_dfm_gemm_z and k_dfm_wgrad ([nb][HP]); scoring stores nothing but rest.
// ----------------------------------------------------------------------------------------------
template <bool TRAIN>
__global__ void __launch_bounds__(256)
k_dfm_gemm_h(const float* __restrict__ S, const float* __restrict__ W1p, const float* __restrict__ b1p, const float* __restrict__ w2p,
             const float* __restrict__ baseg, uint32_t nb, uint32_t WP, uint32_t HP, float* __restrict__ A, float* __restrict__ rest) {
  DFM_STAGE_SETUP;
  const uint32_t ntile = (nb + FMFM_BM - 1) / FMFM_BM, nct = (HP + FMFM_BN - 1) / FMFM_BN, nks = WP / FMFM_BK;
  for (uint32_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint32_t e0 = tile * FMFM_BM;
    const bool a_ok = e0 + a_row < nb;
    const float* __restrict__ a_src = S + (size_t)(a_ok ? e0 + a_row : 0u) * WP + 4u * a_kk;
    float dot[4] = {0.f, 0.f, 0.f, 0.f};
    for (uint32_t ct = 0; ct < nct; ct++) {
      const uint32_t n0 = ct * FMFM_BN;
      const bool b_ok = n0 + b_c < HP;
      fm_f32x4 acc[4];
      dfm_tile_gemm(sg, [&](uint32_t ks) { return ld4_or_zero(a_src + (size_t)ks * FMFM_BK, a_ok); },
                    W1p + (size_t)b_k * HP + (b_ok ? n0 + b_c : 0u), b_ok, (size_t)FMFM_BK * HP, nks, acc);
#pragma unroll
      for (int nt = 0; nt < 4; nt++) {
        const uint32_t col = n0 + 16u * nt + lm;
        if (col < HP) {
          const float bias = b1p[col], wo = w2p[col];
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const uint32_t row = e0 + 16u * w + 4u * lk + q;
            if (row < nb) {
              const float pre = acc[nt][q] + bias;
              const float a = pre > 0.f ? pre : 0.f;
              dot[q] = fmaf(a, wo, dot[q]);
              if (TRAIN) A[(size_t)row * HP + col] = a;
            }
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      float d = dot[q];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) d += __shfl_xor(d, o);
      const uint32_t row = e0 + 16u * w + 4u * lk + q;
      if (lm == 0 && row < nb) rest[row] = baseg[row] + d;
    }
  }
}

// ----------------------------------------------------------------------------------------------
// k_dfm_gemm_z: R = Dh W1p^T + Stot.  The tiling is k_dfm_gemm_h's with K = HP and N = WP.  The A operand is formed while staging:
// dh[e][h] = a[e][h] > 0 ? w2[h] : 0, so Dh is never written to memory (w2's float4 of a stage is the same for all rows).  B is W1t.
// Epilogue: R[e][g KP + c] = Z[e][g KP + c] + Stot[e][c] below W = F KP, zero from there on -- the sum rows FmfmSums hands to the owner.
// ----------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_dfm_gemm_z(const float* __restrict__ A, const float* __restrict__ w2p, const float* __restrict__ W1t, const float* __restrict__ Stg,
             uint32_t nb, uint32_t WP, uint32_t HP, uint32_t KP, uint32_t W, float* __restrict__ R) {
  DFM_STAGE_SETUP;
  const uint32_t ntile = (nb + FMFM_BM - 1) / FMFM_BM, nct = (WP + FMFM_BN - 1) / FMFM_BN, nks = HP / FMFM_BK;
  for (uint32_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint32_t e0 = tile * FMFM_BM;
    const bool a_ok = e0 + a_row < nb;
    const float* __restrict__ a_src = A + (size_t)(a_ok ? e0 + a_row : 0u) * HP + 4u * a_kk;
    const float* __restrict__ w_src = w2p + 4u * a_kk;
    for (uint32_t ct = 0; ct < nct; ct++) {
      const uint32_t n0 = ct * FMFM_BN;
      const bool b_ok = n0 + b_c < WP;
      fm_f32x4 acc[4];
      dfm_tile_gemm(sg, [&](uint32_t ks) {
                      const float4 a = ld4_or_zero(a_src + (size_t)ks * FMFM_BK, a_ok);
                      const float4 wo = *reinterpret_cast<const float4*>(w_src + (size_t)ks * FMFM_BK);
                      return make_float4(a.x > 0.f ? wo.x : 0.f, a.y > 0.f ? wo.y : 0.f, a.z > 0.f ? wo.z : 0.f, a.w > 0.f ? wo.w : 0.f);
                    },
                    W1t + (size_t)b_k * WP + (b_ok ? n0 + b_c : 0u), b_ok, (size_t)FMFM_BK * WP, nks, acc);
#pragma unroll
      for (int nt = 0; nt < 4; nt++) {
        const uint32_t col = n0 + 16u * nt + lm;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint32_t row = e0 + 16u * w + 4u * lk + q;
          if (row < nb && col < WP) R[(size_t)row * WP + col] = col < W ? acc[nt][q] + Stg[(size_t)row * KP + (col & (KP - 1u))] : 0.f;
        }
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------
// k_dfm_wgrad: G = S^T diag(mult) Dh (M = WP, N = HP, K = nb) by k_fmfm_mgrad's scheme: workgroup (tj, ti, p) of the grid (column tiles
// of HP, row tiles, partials) forms one 64 x 64 tile of partial p; K is cut into chunks of FMFM_MCHUNK examples and partial p walks the
// chunks p, p + FMFM_MSPLIT, ... in order, in stages of 16 examples, both operands k-major: A = mult_e S[e][r0 .. r0 + 63],
// B = dh[e][c0 .. c0 + 63], mult_e and the mask applied while staging.  Every row tile works.  Two more row tiles behind the WP / 64 of
// S carry the vectors' gradients through the same split and order: in both the A operand is mult_e in row 0 and zero below; tile
// nrt has B = dh (g_b1 = sum_e mult_e dh_e), tile nrt + 1 has B = a (g_w2 = sum_e mult_e a_e).  P[p][WP + 2][HP] gets the accumulators:
// rows WP and WP + 1 are g_b1 and g_w2.  The launch has min(chunks, FMFM_MSPLIT) partials, so each has work.
// ----------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_dfm_wgrad(const float* __restrict__ S, const float* __restrict__ A, const float* __restrict__ w2p, const float* __restrict__ mult,
            uint32_t nb, uint32_t WP, uint32_t HP, float* __restrict__ P) {
  __shared__ __align__(16) float As[2][FMFM_BK * FMFM_LDB];
  __shared__ __align__(16) float Bs[2][FMFM_BK * FMFM_LDB];
  const uint32_t tj = blockIdx.x, ti = blockIdx.y, p = blockIdx.z;
  const uint32_t nrt = (WP + FMFM_BN - 1) / FMFM_BN;
  const uint32_t vec = ti < nrt ? 0u : ti - nrt + 1u;               // 0: a tile of g_W1; 1: the row g_b1; 2: the row g_w2 (uniform)
  const uint32_t r0 = ti * FMFM_BN, c0 = tj * FMFM_BN;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, lm = lane & 15u, lk = lane >> 4;
  const uint32_t s_ex = tid >> 4, s_c = 4u * (tid & 15u);           // staging: example s_ex of the stage, columns s_c .. + 3 of a tile
  const bool a_ok = !vec && r0 + s_c < WP, b_ok = c0 + s_c < HP;
  const uint32_t dst = s_ex * FMFM_LDB + s_c;
  const uint32_t a_frag = lk * FMFM_LDB + 16u * w + lm, b_frag = lk * FMFM_LDB + lm;
  const float4 wo = ld4_or_zero(w2p + c0 + s_c, b_ok);
  fm_f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; nt++) acc[nt] = fm_f32x4{0.f, 0.f, 0.f, 0.f};
  float4 ra, rb;
  auto load = [&](uint32_t e0) {
    const uint32_t e = e0 + s_ex;
    const bool ok = e < nb;
    const float m = ok ? mult[e] : 0.f;
    ra = ld4_or_zero(S + (size_t)(ok ? e : 0u) * WP + (a_ok ? r0 + s_c : 0u), ok && a_ok);
    ra.x *= m; ra.y *= m; ra.z *= m; ra.w *= m;
    if (vec && s_c == 0u) ra.x = m;
    rb = ld4_or_zero(A + (size_t)(ok ? e : 0u) * HP + (b_ok ? c0 + s_c : 0u), ok && b_ok);
    if (vec != 2u) rb = make_float4(rb.x > 0.f ? wo.x : 0.f, rb.y > 0.f ? wo.y : 0.f, rb.z > 0.f ? wo.z : 0.f, rb.w > 0.f ? wo.w : 0.f);
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
  float* __restrict__ Pp = P + (size_t)p * (WP + 2u) * HP;
#pragma unroll
  for (int nt = 0; nt < 4; nt++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint32_t lr = 16u * w + 4u * lk + q, col = c0 + 16u * nt + lm;
      if (col >= HP) continue;
      if (!vec) { if (r0 + lr < WP) Pp[(size_t)(r0 + lr) * HP + col] = acc[nt][q]; }
      else if (lr == 0u) Pp[(size_t)(WP + vec - 1u) * HP + col] = acc[nt][q];
    }
}

// where element (row, col) of the padded net [WP + 2][HP] lives in the session's fp64 arrays -- rows below WP are W1 (row g KP + a is
// W1[g k + a]), row WP is b1, row WP + 1 is w2 -- or -1 for padding.  net64: W1 [F k][H], b1 [H], w2 [H], one behind the other.
__device__ __forceinline__ int64_t dfm_net_index(uint32_t row, uint32_t col, uint32_t F, uint32_t k, uint32_t KP, uint32_t WP, uint32_t H) {
  if (col >= H) return -1;
  if (row >= WP) return (int64_t)F * k * H + (int64_t)(row - WP) * H + col;
  const uint32_t g = row / KP, a = row % KP;
  return (g < F && a < k) ? ((int64_t)g * k + a) * H + col : -1;
}
// the fp32 copies of one element: W1p [WP][HP], W1t [HP][WP], b1p [HP], w2p [HP], one behind the other in net32
__device__ __forceinline__ void dfm_net_put32(float* __restrict__ net32, uint32_t row, uint32_t col, uint32_t WP, uint32_t HP, float v) {
  const size_t wh = (size_t)WP * HP;
  if (row < WP) { net32[(size_t)row * HP + col] = v; net32[wh + (size_t)col * WP + row] = v; }
  else net32[2 * wh + (size_t)(row - WP) * HP + col] = v;
}

// k_dfm_netstep: one thread per element of the padded net; those inside W1, b1 and w2 step.  The partials in order in fp64, L2 once per
// batch, then  n += g^2;  theta -= eta g / sqrt(n)  in fp64 on the session's net and accumulators (acc64, laid out as net64); the fp32
// copies get the new value.  A net that is all zero has g == 0 everywhere and stays exactly zero.
static __global__ void __launch_bounds__(256)
k_dfm_netstep(const float* __restrict__ P, uint32_t nsplit, uint32_t F, uint32_t k, uint32_t KP, uint32_t WP, uint32_t H, uint32_t HP,
              double* __restrict__ net64, double* __restrict__ acc64, float* __restrict__ net32, double eta, double reg) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (WP + 2u) * HP) return;
  const uint32_t row = t / HP, col = t % HP;
  const int64_t at = dfm_net_index(row, col, F, k, KP, WP, H);
  if (at < 0) return;
  double s = 0.0;
  for (uint32_t p = 0; p < nsplit; p++) s += (double)P[((size_t)p * (WP + 2u) + row) * HP + col];
  const double th = net64[at];
  const double gr = s + reg * th;
  const double n1 = acc64[at] + gr * gr;
  const double tn = th - eta * gr / sqrt(n1);
  net64[at] = tn; acc64[at] = n1;
  dfm_net_put32(net32, row, col, WP, HP, (float)tn);
}

// the fp32 copies from net64, zero in all padding
static __global__ void __launch_bounds__(256)
k_dfm_pad_net(const double* __restrict__ net64, uint32_t F, uint32_t k, uint32_t KP, uint32_t WP, uint32_t H, uint32_t HP, float* __restrict__ net32) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (WP + 2u) * HP) return;
  const uint32_t row = t / HP, col = t % HP;
  const int64_t at = dfm_net_index(row, col, F, k, KP, WP, H);
  dfm_net_put32(net32, row, col, WP, HP, at < 0 ? 0.f : (float)net64[at]);
}

}  // namespace fmx
