/*
 * fm_oracle_noise.c -- the device's keyed noise of a sampled sweep (libfm_amd/csrc/fmx_als_kernels.h), restated on the host.
 * TEST INFRASTRUCTURE ONLY (see fm_oracle.h).
 *
 * This is not the reference's generator (libc rand(), util/random.h): it restates the PRODUCT's noise contract, so that a
 * sampled chain of the device can be followed draw for draw.  The hashes and the integer-to-float steps are exact; the
 * transcendental functions are the host's (logf / cosf where the device uses __logf / __cosf: a few fp32 ulps apart;
 * log / cos / exp / sqrt in fp64 where the device uses the same fp64 functions: at most an ulp apart).
 */
#include "fm_oracle.h"

#include <math.h>

/* the stream of one (sweep, family): fmx_als_kernels.h mcmc_stream */
uint64_t fmo_mcmc_stream(uint64_t iter, uint32_t family, int f) { return iter * 4096u + (uint64_t)family + (uint64_t)f; }

/* unif_hash: (0, 1) from 53 bits of one hash of (seed, stream, idx, attempt) */
double fmo_unif_hash(uint64_t seed, uint64_t stream, uint64_t idx, uint32_t attempt) {
  const uint64_t hh = fmo_mix64(seed ^ (stream * 0x9E3779B97F4A7C15ULL) ^
                                (idx * 0xD6E8FEB86659FD93ULL + (uint64_t)attempt * 0xA24BAED4963EE407ULL + 0x9FB21C651E98DF25ULL));
  return ((double)(hh >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

/* gauss_hash2: fp64 Box-Muller on uniforms 2 * attempt and 2 * attempt + 1 */
double fmo_gauss_hash2(uint64_t seed, uint64_t stream, uint64_t idx, uint32_t attempt) {
  const double u1 = fmo_unif_hash(seed, stream, idx, 2 * attempt), u2 = fmo_unif_hash(seed, stream, idx, 2 * attempt + 1);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

/* gauss_hash: the N(0,1) of a coordinate draw -- two chained hashes, 24-bit uniforms, fp32 Box-Muller */
double fmo_gauss_hash(uint64_t seed, uint64_t stream, uint64_t idx) {
  const uint64_t h1 = fmo_mix64(seed ^ (stream * 0x9E3779B97F4A7C15ULL) ^ (idx * 0xD6E8FEB86659FD93ULL + 0x632BE59BD9B4E019ULL));
  const uint64_t h2 = fmo_mix64(h1 + 0x9E3779B97F4A7C15ULL);
  const float u1 = ((float)(uint32_t)(h1 >> 40) + 1.0f) * (1.0f / 16777216.0f);    /* (0,1] */
  const float u2 = (float)(uint32_t)(h2 >> 40) * (1.0f / 16777216.0f);             /* [0,1) */
  return (double)(sqrtf(-2.0f * logf(u1)) * cosf(6.2831853f * u2));
}

/* left_tgauss: N(0,1) conditioned on z >= left, in the device's order of attempts (random.h:70-101 restated with keyed
 * uniforms): naive rejection through gauss_hash2(attempt) for left <= 0, Robert's translated exponential otherwise
 * (uniforms 2a for the exponential, 2a + 1 for the acceptance); 64 attempts at most */
double fmo_left_tgauss(double left, uint64_t seed, uint64_t stream, uint64_t idx) {
  if (left <= 0.0) {
    double r = 0.0;
    for (uint32_t a = 0; a < 64; a++) { r = fmo_gauss_hash2(seed, stream, idx, a); if (r >= left) return r; }
    return fmax(r, left);
  }
  const double alpha_star = 0.5 * (left + sqrt(left * left + 4.0));
  double zz = left;
  for (uint32_t a = 0; a < 64; a++) {
    zz = -log(1.0 - fmo_unif_hash(seed, stream, idx, 2 * a)) / alpha_star + left;
    double d = zz - alpha_star;
    d = exp(-(d * d) / 2);
    if (fmo_unif_hash(seed, stream, idx, 2 * a + 1) < d) return zz;
  }
  return zz;
}

void fmo_gauss_hash_n(uint64_t seed, uint64_t stream, const uint64_t *idx, uint64_t n, double *out) {
  for (uint64_t i = 0; i < n; i++) out[i] = fmo_gauss_hash(seed, stream, idx[i]);
}
