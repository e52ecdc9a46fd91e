// phm_qupdate.h -- rate-matrix updates of the Q-updating drivers (host side); see phm_qupdate.cpp
#pragma once

#include <stdint.h>

#include <cmath>

namespace phm {

// Philox4x32-7 on the host, as every stream of the engine (phm_device.h): counter (c0, c1, c2, c3), key (k0, k1)
inline void philox_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
  for (int r = 0; r < 7; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// Sequential host draws of the stream (seed, entity, iteration word, replica word): the uniform of draw d is word d & 3 of block
// d >> 2, (x + 0.5) 2^-32; the gamma variate is Marsaglia & Tsang's (2000) squeeze with a Box-Muller normal.  The Q-updating
// drivers address it by UpdateStream (phm_qupdate.cpp), phm_gibbs_rates by (ENT_RATE | parameter, chain, iteration + offset).
struct HostStream {
  uint64_t seed;
  uint32_t ent, iter, rep, next = 0;
  double uniform() {
    uint32_t o[4];
    const uint32_t d = next++;
    philox_host(d >> 2, ent, iter, rep, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), o);
    return ((double)o[d & 3u] + 0.5) * 2.3283064365386962890625e-10;
  }
  double gamma(double shape, double scale) {
    double boost = 1.0;
    if (shape < 1.0) { const double u = uniform(); boost = std::pow(u, 1.0 / shape); shape += 1.0; }
    const double d = shape - 1.0 / 3.0, c = 1.0 / std::sqrt(9.0 * d);
    for (;;) {
      const double u1 = uniform(), u2 = uniform();
      const double z = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
      double v = 1.0 + c * z;
      if (v <= 0.0) continue;
      v = v * v * v;
      const double u = uniform();
      if (std::log(u) < 0.5 * z * z + d - d * v + d * std::log(v)) return d * v * boost * scale;
    }
  }
};

// entity tag of phm_gibbs_rates' rate draws, or-ed with the 0-based parameter: section 19's histories, which share the address
// space (seed, entity, evaluation or chain, iteration), use ENT_NODE and ENT_BUNIF of phm_device.h only; 2 << 30 is free there
constexpr uint32_t ENT_RATE = 2u << 30;

// Q: n x n column-major, edited in place.  row: one iteration's statistics, n dwell sums then n*n counts (row-major from,to).
// bf: prior[4] = (alpha01, beta01, alpha10, beta10)         src/phylomap.cpp:1189-1253
void bf_updates(double* Q, double Omega, const double* prior, const double* row, uint64_t seed, uint32_t iter);
// ks: prior[6] = (alpha_lambda, beta_lambda, alpha_kappa, beta_kappa, alpha_gamma, beta_gamma), n = 2k+2 >= 4   :1435-1785
// mt = true: the multi-tree twins (prior[8]: l01, l10, kappa, gamma shape/rate pairs)                         :2371-2705
void ks_updates(double* Q, int n, double Omega, const double* prior, const double* row, uint64_t seed, uint32_t iter, bool mt = false);
// two-state multi-tree updates (acceptance tested), prior[4]                                                  :2192-2262
void mt_updates(double* Q, double Omega, const double* prior, const double* row, uint64_t seed, uint32_t iter);
// index of the tree whose row drives this iteration's update (sampleOnce over unit weights, :2347-2348); n_trees = ran off the end
uint32_t pick_tree(int n_trees, uint64_t seed, uint32_t iter);

}  // namespace phm
