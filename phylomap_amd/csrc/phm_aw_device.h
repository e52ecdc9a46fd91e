// phm_aw_device.h -- the device pieces of the one-state-per-lane kernels at 9..64 states, shared by
// phm_ancestral_wide.hip, phm_scores_wide.hip and phm_sample_wide.hip: the shape of a 256-lane workgroup of NP-lane groups, the
// group maximum, the rescale, the transposed staging of a matrix, and mu_k and B_k of a model.
#pragma once

#include <hip/hip_runtime.h>

namespace phm {

constexpr int AW_BLOCK = 256;

template <int NP> struct AwShape {
  static constexpr int G = AW_BLOCK / NP;      // groups (items) of a workgroup
  static constexpr int LD = NP + 1;            // row of a staged matrix
  static constexpr int VS = NP + 2;            // row of a staged vector
};

template <int NP> __device__ __forceinline__ double aw_group_max(double v) {
  double m = fmax(0.0, v);
#pragma unroll
  for (int off = NP / 2; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off, NP));
  return m;
}

// the value scaled by 2^-e with the maximum in [1/2, 1); e = 0 for an all-zero vector (ex_rescale)
__device__ __forceinline__ double aw_rescale(double v, double mx, int& e) {
  e = 0;
  if (!(mx > 0.0)) return v;
  (void)frexp(mx, &e);
  return ldexp(v, -e);
}

// sP[j * LD + i] = P[i][j]
template <int NP> __device__ __forceinline__ void aw_stage_t(double* sP, const double* __restrict__ P, int n) {
  for (int e = threadIdx.x; e < n * n; e += AW_BLOCK) {
    const int i = e / n, j = e - i * n;
    sP[j * AwShape<NP>::LD + i] = P[e];
  }
}

// mu_k = max_i(-q_ii)
__device__ __forceinline__ double aw_model_mu(const double* __restrict__ Qk, int n) {
  double mu = 0.0;
  for (int i = 0; i < n; ++i) mu = fmax(mu, -Qk[(size_t)i * n + i]);
  return mu;
}

// one cell of B_k = I + Q_k / mu_k (I when mu_k = 0): q the cell of Q_k, d the cell of I
__device__ __forceinline__ double aw_model_b(double q, double mu, double d) { return mu > 0.0 ? d + q / mu : d; }

}  // namespace phm
