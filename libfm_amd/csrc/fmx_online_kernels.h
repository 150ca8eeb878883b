// fmx_online_kernels.h -- the parity instruments: the reference's online loops walked entry by entry on ONE wavefront.
//   k_sequential      fm_learn_sgd_element (fm_learn_sgd_element.h:56-67 around fm_SGD, fm_sgd.h:33-51): FMX_SGD_SEQUENTIAL where no faster
//                     form applies; its row step seq_row_entries is also what the row-at-a-time kernels (fmx_seq_kernels.h) fall back to
//   k_sgda            fm_learn_sgd_element_adapt_reg (`-method sgda`): fmx_sgda_epoch
// Every other SGD form of the library is judged against these, so each piece of the loop is written once: pass 1 (online_row_predict), the
// fm_SGD entry update (seq_row_entries), the SGDA entry update (sgda_row_theta); the fp64 multipliers are sgd_mult_d / sgda_mult_d
// (fmx_kernels.h).  Loads bypass the per-CU L1 (ld_l2) and every entry ends with a drain of the store queue, so a later entry of the row
// (a repeated id, fm_sgd.h:44-50) and the next row see the update like the reference's loop.  Sums in fp64, parameters stored fp32.
// Included by fmx_sgd.hip only, before fmx_seq_kernels.h.
#pragma once

namespace fmx {

// pass 1 of a row (fm_model.h:105-127): returns p = w0 + sum w x + 0.5 sum_f (sum[f]^2 - sum (v x)^2), leaves this lane's factors of
// fm.m_sum in `sum`
template <int KP>
__device__ __forceinline__ double online_row_predict(const Entry* __restrict__ ent, uint64_t a, uint32_t size, const Tab& tb, const Hyper& h, double w0,
                                                     double (&sum)[Map<KP>::VEC]) {
  constexpr int VEC = Map<KP>::VEC;
  const uint32_t lane = threadIdx.x & 63u;
  const bool act = row_lane<KP>(lane, tb);
  double sq = 0.0, lin = 0.0;
#pragma unroll
  for (int v = 0; v < VEC; v++) sum[v] = 0.0;
  for (uint32_t i = 0; i < size; i++) {
    const Entry e = ent[a + i];
    if (h.k1 && lane == 0) lin += (double)ld_l2(tb.w + (size_t)e.id * tb.ws) * (double)e.value;
    if (act) {
#pragma unroll
      for (int v = 0; v < VEC; v++) {
        const double d = (double)ld_l2(tb.V + (size_t)e.id * tb.rs + lane * VEC + v) * (double)e.value;
        sum[v] += d;
        sq += d * d;
      }
    }
  }
  double part = lin - 0.5 * sq;
  if (act) {
#pragma unroll
    for (int v = 0; v < VEC; v++) part += 0.5 * sum[v] * sum[v];
  }
  return (h.k0 ? w0 : 0.0) + wave_sum_d(part);
}

// the fm_SGD step of one row (fm_sgd.h:33-51), entry by entry, every store drained before the next entry
template <int KP>
__device__ __forceinline__ void seq_row_entries(const Entry* __restrict__ ent, uint64_t a, uint32_t size, float yf, const Tab& tb, const Hyper& h, double& w0) {
  constexpr int VEC = Map<KP>::VEC;
  const uint32_t lane = threadIdx.x & 63u;
  const bool act = row_lane<KP>(lane, tb);
  double sum[VEC];
  const double p = online_row_predict<KP>(ent, a, size, tb, h, w0, sum);
  const double mult = sgd_mult_d(h, p, (double)yf);
  if (h.k0) w0 -= h.lr_d * (mult + h.reg0_d * w0);
  for (uint32_t i = 0; i < size; i++) {
    const Entry e = ent[a + i];
    const double x = (double)e.value;
    if (h.k1 && lane == 0) {
      float* pw = tb.w + (size_t)e.id * tb.ws;
      const double wv = (double)ld_l2(pw);
      st_l2(pw, (float)(wv - h.lr_d * (mult * x + h.regw_d * wv)));
    }
    if (act) {
#pragma unroll
      for (int v = 0; v < VEC; v++) {
        float* pv = tb.V + (size_t)e.id * tb.rs + lane * VEC + v;
        const double vv = (double)ld_l2(pv);
        const double grad = sum[v] * x - vv * x * x;
        st_l2(pv, (float)(vv - h.lr_d * (mult * grad + h.regv_d * vv)));
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // a later entry of this row (repeated id) and the next row must observe these stores
  }
}

// the reference trajectory (batch = 1, storage order) of n_rows rows
template <int KP>
__global__ void __launch_bounds__(64)
k_sequential(const Entry* __restrict__ ent, const uint64_t* __restrict__ row_ptr, const float* __restrict__ target,
             uint32_t n_rows, const Tab tb, Hyper h, double* w0_ptr) {
  double w0 = *w0_ptr;
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint64_t a = row_ptr[r];
    seq_row_entries<KP>(ent, a, (uint32_t)(row_ptr[r + 1] - a), target[r], tb, h, w0);
  }
  if ((threadIdx.x & 63u) == 0) *w0_ptr = w0;
}

// ----------------------------------------------------------------------------------------------
// SGDA (src/libfm/src/fm_learn_sgd_element_adapt_reg.h), the reference's strictly online interleaving: for every train row a theta step
// (:136-169), then (from the 2nd epoch on) a lambda step on the next validation row (:201-248 through predict_scaled :171-199).
// ----------------------------------------------------------------------------------------------
// What a lane holds of the attribute group of one feature: the learned regularisation reg_w (lane 0) / the lane's factors of reg_v, and the
// group's sums of the running lambda step lambda_w_grad (lane 0), sum_f, sum_f_dash_f (:96-98).  One group: the kernel's registers; with
// attribute groups: its LDS tables at grp[id], and the stamp that says whether the group's sums belong to the current validation row.
struct SgdaCells { double* reg_w; double* reg_v; double* lw; double* sf; double* sdf; uint32_t* stamp; };

// the theta step of one train row (:136-169): like fm_SGD, but mult = 2 (p - y), reg_0 = 0, regularisation 2 * reg * theta with the LEARNED
// reg_w / reg_v[f] of the feature's group (cells_of(id)), and the gradient of every touched parameter remembered in gw / gv (as fp32:
// the update uses what a later predict_scaled will read)
template <int KP, class CellsOf>
__device__ __forceinline__ void sgda_row_theta(const Entry* __restrict__ ent, uint64_t a, uint32_t size, float yf, const Tab& tb, const Hyper& h, double& w0,
                                               float* gw, float* gv, const CellsOf& cells_of) {
  constexpr int VEC = Map<KP>::VEC;
  const uint32_t lane = threadIdx.x & 63u;
  const bool act = row_lane<KP>(lane, tb);
  double sum[VEC];
  const double p = online_row_predict<KP>(ent, a, size, tb, h, w0, sum);
  const double mult = sgda_mult_d(h, p, (double)yf);
  if (h.k0) w0 -= h.lr_d * (mult + 2 * 0.0 * w0);                            // reg_0 = 0 (:100)
  for (uint32_t i = 0; i < size; i++) {
    const Entry e = ent[a + i];
    const double x = (double)e.value;
    const SgdaCells c = cells_of(e.id);
    if (h.k1 && lane == 0) {
      float* pw = tb.w + (size_t)e.id * tb.ws;
      const double wv = (double)ld_l2(pw);
      const double g = mult * x;
      st_l2(gw + e.id, (float)g);
      st_l2(pw, (float)(wv - h.lr_d * ((double)(float)g + 2 * c.reg_w[0] * wv)));
    }
    if (act) {
#pragma unroll
      for (int v = 0; v < VEC; v++) {
        float* pv = tb.V + (size_t)e.id * tb.rs + lane * VEC + v;
        const double vv = (double)ld_l2(pv);
        const double g = mult * (x * (sum[v] - vv * x));
        st_l2(gv + (size_t)e.id * tb.rs + lane * VEC + v, (float)g);
        st_l2(pv, (float)(vv - h.lr_d * ((double)(float)g + 2 * c.reg_v[v] * vv)));
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

// k_sgda: one wavefront.  reg (global): [G][1 + KP], reg[g*(1+KP)] = reg_w(g), reg[g*(1+KP)+1+f] = reg_v(g,f).
// !GROUPED (one attribute group; grp unused, G = 1): the regularisation and the sums of the lambda step stay in registers, no barrier.
// GROUPED (`-meta`): they live in LDS:  regw[G] | regv[G][KP] | lwg[G] | sfg[G][KP] | sdfg[G][KP] | stamp[G]
// Only the groups present in a validation row are zeroed / updated: for an absent group the reference's update is
// reg -= lr * grad_loss * (-0.0), i.e. the identity for every finite grad_loss.  Each (g, factor) cell is owned by
// one lane; lane 0 owns the linear cells and the stamps, hence the barriers around the stamp reads.
template <int KP, bool GROUPED>
__global__ void __launch_bounds__(64)
k_sgda(const Entry* __restrict__ ent, const uint64_t* __restrict__ row_ptr, const float* __restrict__ target, uint32_t n_rows,
       const Entry* __restrict__ vent, const uint64_t* __restrict__ vrow_ptr, const float* __restrict__ vtarget, uint32_t v_rows,
       const Tab tb, float* gw, float* gv, Hyper h, double* w0_ptr, double* reg, int do_lambda,
       const uint32_t* __restrict__ grp, uint32_t G) {
  constexpr int VEC = Map<KP>::VEC;
  extern __shared__ double sgda_lds[];
  double* regw = sgda_lds;
  double* regv = regw + G;
  double* lwg = regv + (size_t)G * KP;
  double* sfg = lwg + G;
  double* sdfg = sfg + (size_t)G * KP;
  uint32_t* stamp = (uint32_t*)(sdfg + (size_t)G * KP);
  const uint32_t lane = threadIdx.x & 63u;
  const bool act = row_lane<KP>(lane, tb);
  double reg_w = 0.0, lw = 0.0, reg_v[VEC], s_f[VEC], s_df[VEC];
  if constexpr (GROUPED) {
    for (uint32_t g = lane; g < G; g += 64) { regw[g] = reg[(size_t)g * (1 + KP)]; stamp[g] = 0; }
    for (uint32_t i = lane; i < G * KP; i += 64) regv[i] = reg[(size_t)(i / KP) * (1 + KP) + 1 + (i % KP)];
    __syncthreads();
  } else {
    reg_w = reg[0];
#pragma unroll
    for (int v = 0; v < VEC; v++) reg_v[v] = act ? reg[1 + lane * VEC + v] : 0.0;
  }
  const auto cells_of = [&](uint32_t id) -> SgdaCells {
    if constexpr (GROUPED) {
      const uint32_t g = grp[id];
      const size_t c = (size_t)g * KP + lane * VEC;
      return SgdaCells{regw + g, regv + c, lwg + g, sfg + c, sdfg + c, stamp + g};
    } else {
      return SgdaCells{&reg_w, reg_v, &lw, s_f, s_df, nullptr};
    }
  };
  double w0 = *w0_ptr;
  uint32_t vpos = 0, cur = 0;                                                 // validation->data->begin() (:266)
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint64_t a = row_ptr[r];
    sgda_row_theta<KP>(ent, a, (uint32_t)(row_ptr[r + 1] - a), target[r], tb, h, w0, gw, gv, cells_of);
    if (!do_lambda || v_rows == 0) continue;
    // ---------------- lambda step on the next validation row (:271-276, :201-248)
    if (vpos >= v_rows) vpos = 0;
    const uint64_t va = vrow_ptr[vpos];
    const uint32_t vsize = (uint32_t)(vrow_ptr[vpos + 1] - va);
    const double vy = (double)vtarget[vpos];
    vpos++;
    if constexpr (GROUPED) {
      cur += 2;                                                                  // stamp == cur: sums valid; cur+1: updated
    } else {
      lw = 0.0;
#pragma unroll
      for (int v = 0; v < VEC; v++) { s_f[v] = 0.0; s_df[v] = 0.0; }
    }
    double plin = 0.0, q_dash = 0.0;
    double s_dash[VEC];
#pragma unroll
    for (int v = 0; v < VEC; v++) s_dash[v] = 0.0;
    for (uint32_t i = 0; i < vsize; i++) {
      const Entry e = vent[va + i];
      const double x = (double)e.value;
      const SgdaCells c = cells_of(e.id);
      if constexpr (GROUPED) {                                                   // the row meets the group for the first time: its sums start at 0
        const bool fresh = *c.stamp != cur;
        __syncthreads();
        if (fresh) {
          if (lane == 0) { *c.lw = 0.0; *c.stamp = cur; }
          if (act) {
#pragma unroll
            for (int v = 0; v < VEC; v++) { c.sf[v] = 0.0; c.sdf[v] = 0.0; }
          }
        }
        __syncthreads();
      }
      if (h.k1 && lane == 0) {
        const double wv = (double)ld_l2(tb.w + (size_t)e.id * tb.ws);
        const double w_dash = wv - h.lr_d * ((double)ld_l2(gw + e.id) + 2 * c.reg_w[0] * wv);   // predict_scaled :178-184
        plin += w_dash * x;
        *c.lw += x * wv;                                                         // :215-218
      }
      if (act) {
#pragma unroll
        for (int v = 0; v < VEC; v++) {
          const double vv = (double)ld_l2(tb.V + (size_t)e.id * tb.rs + lane * VEC + v);
          const double v_dash = vv - h.lr_d * ((double)ld_l2(gv + (size_t)e.id * tb.rs + lane * VEC + v) + 2 * c.reg_v[v] * vv);
          const double d = v_dash * x;
          s_dash[v] += d; q_dash += d * d;                                       // :186-196
          c.sf[v] += vv * x;                                                     // :233-238
          c.sdf[v] += d * vv * x;
        }
      }
    }
    double vpart = plin - 0.5 * q_dash;
    if (act) {
#pragma unroll
      for (int v = 0; v < VEC; v++) vpart += 0.5 * s_dash[v] * s_dash[v];
    }
    const double grad_loss = sgda_mult_d(h, (h.k0 ? w0 : 0.0) + wave_sum_d(vpart), vy);
    const auto reg_step = [&](const SgdaCells& c) {
      if (h.k1 && lane == 0) {                                                   // :213-224
        const double lwt = -2 * h.lr_d * c.lw[0];
        c.reg_w[0] = fmax(0.0, c.reg_w[0] - h.lr_d * grad_loss * lwt);
      }
      if (act) {                                                                 // :240-246
#pragma unroll
        for (int v = 0; v < VEC; v++) {
          const double lambda_v_grad = -2 * h.lr_d * (s_dash[v] * c.sf[v] - c.sdf[v]);
          c.reg_v[v] = fmax(0.0, c.reg_v[v] - h.lr_d * grad_loss * lambda_v_grad);
        }
      }
    };
    if constexpr (GROUPED) {
      for (uint32_t i = 0; i < vsize; i++) {                                     // every group of the row, once
        const SgdaCells c = cells_of(vent[va + i].id);
        const bool todo = *c.stamp == cur;
        __syncthreads();
        if (todo) {
          if (lane == 0) *c.stamp = cur + 1;
          reg_step(c);
        }
        __syncthreads();
      }
    } else {
      reg_step(cells_of(0));
    }
  }
  if (lane == 0) *w0_ptr = w0;
  if constexpr (GROUPED) {
    __syncthreads();
    for (uint32_t g = lane; g < G; g += 64) reg[(size_t)g * (1 + KP)] = regw[g];
    for (uint32_t i = lane; i < G * KP; i += 64) reg[(size_t)(i / KP) * (1 + KP) + 1 + (i % KP)] = regv[i];
  } else {
    if (lane == 0) reg[0] = reg_w;
    if (act) {
#pragma unroll
      for (int v = 0; v < VEC; v++) reg[1 + lane * VEC + v] = reg_v[v];
    }
  }
}

}  // namespace fmx
