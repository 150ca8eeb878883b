// fm_oracle_w0.cpp -- the N(0,1) of a sampled sweep's bias draw, restated (TEST INFRASTRUCTURE ONLY, see fm_oracle.h).
// The device draws it on the host (libfm_amd/csrc/fmx_als.hip, als_sweep_shards): a fresh std::mt19937_64 per sweep seeded with
// seed * 0x9E3779B97F4A7C15 + iter + 1, and the first variate of std::normal_distribution<double>(0, 1).  Built against the same
// C++ standard library, this is the same number.
#include <cstdint>
#include <random>

extern "C" double fmo_w0_noise(uint64_t seed, uint64_t iter) {
  std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + iter + 1);
  std::normal_distribution<double> nd(0.0, 1.0);
  return nd(rng);
}
