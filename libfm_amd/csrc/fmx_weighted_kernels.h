// fmx_weighted_kernels.h -- kernels of the per-row weights (include/fmx.h "fmx_set_row_weights").
//
// k_scan_weighted  step 2 of a batch of fmx_adapt_epoch / fmx_ftrl_epoch on a slot with weights: the bias recurrence in micro-chunks
//                  with every example's multiplier scaled by its weight.  Modelled on k_scan (fmx_kernels.h), which it leaves alone.
// (The kernels of fmx_evaluate_weighted are in fmx_evalw_kernels.h.)
#pragma once
#include "fmx_kernels.h"

namespace fmx {

// ----------------------------------------------------------------------------------------------
// k_scan_weighted: per micro-chunk with its start bias w0s
//   m_e = c_e * multiplier(w0s + rest_e, y_e)             fp32 product of the fp32 multiplier and the fp32 weight
//   w0 -= lr * (sum_chunk m_e + chunk_rows * reg0 * w0s)    fp64, the form of k_scan's chunk end: reg0 counts rows, not weight
//   mult[e] = m_e
// ONE workgroup of ONE wavefront.  rest / target / weight tiles arrive by LDS-DMA (scan_fetch_array: its dword path takes a start
// that is not 16-byte aligned, and each array decides for itself), tile t+1 in flight while tile t is scanned.  Three arrays, two
// buffers each: a tile of 2048 examples keeps the kernel in 48 KiB of static LDS (k_scan's 4096 would need 96 KiB).
// CH = 0: any micro-chunk length.  Summation order: a lane's elements of a micro-chunk in order (blocks of 256: four per lane,
// pairwise), the lanes by DPP.
// CH = 16 / 32 / 64 (chunk == CH; the library's default micro-chunks): the sub-piece form, after k_scan1's.  A vector of 64
// examples, one per lane, is 64 / CH micro-chunks that never straddle a vector or a tile (SCANW_TILE is a multiple of 64): the
// operands of vector v+1 are read from LDS before the chain of vector v starts, so no LDS latency sits between two micro-chunks;
// every lane evaluates the multiplier with the micro-chunk's bias, the micro-chunk's lanes keep it, group_sum_dpp closes one DPP
// row (16), half a wavefront (32) or the wavefront (64).  Lanes past the batch's end hold weight 0 (m = 0 * a finite number = 0).
// Either order is fixed for a given (n_rows, chunk): two runs are bit-identical.  Without k0 the bias is not read or written and
// w0s = 0; the host passes chunk = n_rows and CH = 0 then (nothing depends on the micro-chunk).
// It runs on the handle's stream between k_rowsums and the owner kernel: no hand-off, no side stream, no VGPR budget to share a SIMD
// with a gather.
// ----------------------------------------------------------------------------------------------
constexpr int SCANW_TILE = 2048;

__device__ __forceinline__ void scanw_fetch_tile(const float* __restrict__ g_rest, const float* __restrict__ g_y, const float* __restrict__ g_c,
                                                 uint32_t cnt, float* s_r, float* s_t, float* s_c, uint32_t lane) {
  scan_fetch_array(g_rest, cnt, s_r, lane);
  scan_fetch_array(g_y, cnt, s_t, lane);
  scan_fetch_array(g_c, cnt, s_c, lane);
}

template <int TASK, int CH>
__global__ void __launch_bounds__(64)
k_scan_weighted(const float* __restrict__ rest, const float* __restrict__ target, const float* __restrict__ weight, uint32_t n_rows,
                uint32_t chunk, Hyper h, double* __restrict__ w0_io, float* __restrict__ mult) {
  __shared__ float s_rest[2][SCANW_TILE];
  __shared__ float s_y[2][SCANW_TILE];
  __shared__ float s_c[2][SCANW_TILE];
  const uint32_t lane = threadIdx.x;
  const uint32_t n_tiles = (n_rows + SCANW_TILE - 1) / SCANW_TILE;
  double w0 = h.k0 ? *w0_io : 0.0;
  uint32_t chunk_pos = 0;
  float acc = 0.f;
  scanw_fetch_tile(rest, target, weight, min((uint32_t)SCANW_TILE, n_rows), s_rest[0], s_y[0], s_c[0], lane);
  for (uint32_t t = 0; t < n_tiles; t++) {
    const uint32_t t0 = t * SCANW_TILE;
    const uint32_t tn = min((uint32_t)SCANW_TILE, n_rows - t0);
    const uint32_t cur = t & 1u;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // tile t has landed in LDS (issued one tile ago)
    __builtin_amdgcn_s_barrier();                              // single wavefront: orders the DMA writes before the reads
    if (t + 1 < n_tiles) {
      const uint32_t u0 = t0 + SCANW_TILE;
      scanw_fetch_tile(rest + u0, target + u0, weight + u0, min((uint32_t)SCANW_TILE, n_rows - u0), s_rest[cur ^ 1u], s_y[cur ^ 1u],
                       s_c[cur ^ 1u], lane);
    }
    const float* sr = s_rest[cur];
    const float* sy = s_y[cur];
    const float* sc = s_c[cur];
    if constexpr (CH > 0) {
      float r = lane < tn ? sr[lane] : 0.f, y = lane < tn ? sy[lane] : 0.f, c = lane < tn ? sc[lane] : 0.f;
      for (uint32_t base = 0; base < tn; base += 64) {
        const uint32_t qn = base + 64 + lane;                  // (qn < tn <= SCANW_TILE: inside the tile)
        const bool hn = qn < tn;
        const float rn = hn ? sr[qn] : 0.f, yn = hn ? sy[qn] : 0.f, cn = hn ? sc[qn] : 0.f;
        const uint32_t left = tn - base;                       // examples from this vector's first to the tile's end (>= 1)
        float mk = 0.f;
#pragma unroll
        for (uint32_t g = 0; g < 64u / (uint32_t)CH; g++) {
          if (g * (uint32_t)CH < left) {                       // (wave-uniform: all 64 lanes take part in the DPP sum)
            const float w0s = h.k0 ? (float)w0 : 0.f;
            const float m = __fmul_rn(c, multiplier_task<TASK>(h, w0s + r, y));
            if (lane / (uint32_t)CH == g) mk = m;
            const float tot = group_sum_dpp<CH>(m, g);
            const uint32_t rows_here = min((uint32_t)CH, left - g * (uint32_t)CH);
            if (h.k0) w0 -= (double)h.lr * ((double)tot + (double)rows_here * (double)h.reg0 * (double)w0s);
          }
        }
        if (base + lane < tn) mult[t0 + base + lane] = mk;     // (t0 + base + lane < t0 + tn <= n_rows)
        r = rn; y = yn; c = cn;
      }
      continue;
    }
    uint32_t i = 0;
    while (i < tn) {
      const uint32_t take = min(chunk - chunk_pos, tn - i);   // (i + take <= tn <= SCANW_TILE: every LDS index below stays in the tile)
      const float w0s = h.k0 ? (float)w0 : 0.f;
      uint32_t tt = 0;
      for (; tt + 256 <= take; tt += 256) {                   // 4 independent elements per lane: reads first, then math
        const uint32_t q = i + tt + lane;
        float m0 = sr[q], m1 = sr[q + 64], m2 = sr[q + 128], m3 = sr[q + 192];
        const float y0 = sy[q], y1 = sy[q + 64], y2 = sy[q + 128], y3 = sy[q + 192];
        const float c0 = sc[q], c1 = sc[q + 64], c2 = sc[q + 128], c3 = sc[q + 192];
        m0 = __fmul_rn(c0, multiplier_task<TASK>(h, w0s + m0, y0));   // (the rounded product is what is stored AND summed: no fma contraction)
        m1 = __fmul_rn(c1, multiplier_task<TASK>(h, w0s + m1, y1));
        m2 = __fmul_rn(c2, multiplier_task<TASK>(h, w0s + m2, y2));
        m3 = __fmul_rn(c3, multiplier_task<TASK>(h, w0s + m3, y3));
        mult[t0 + q] = m0; mult[t0 + q + 64] = m1; mult[t0 + q + 128] = m2; mult[t0 + q + 192] = m3;   // (t0 + q + 192 < t0 + i + take <= n_rows)
        acc += (m0 + m1) + (m2 + m3);
      }
      for (tt += lane; tt < take; tt += 64) {
        const float m = __fmul_rn(sc[i + tt], multiplier_task<TASK>(h, w0s + sr[i + tt], sy[i + tt]));
        mult[t0 + i + tt] = m;
        acc += m;
      }
      i += take; chunk_pos += take;
      if (chunk_pos == chunk || t0 + i == n_rows) {
        const float tot = wave_sum_dpp(acc);
        if (h.k0) w0 -= (double)h.lr * ((double)tot + (double)chunk_pos * (double)h.reg0 * (double)w0s);
        acc = 0.f; chunk_pos = 0;
      }
    }
  }
  if (h.k0 && lane == 0) *w0_io = w0;
}

}  // namespace fmx
