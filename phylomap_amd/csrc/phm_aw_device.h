// phm_aw_device.h -- the device pieces of the one-state-per-lane kernels at 9..64 states, shared by
// phm_ancestral_wide.hip, phm_scores_wide.hip and phm_sample_wide.hip: the shape of a 256-lane workgroup of NP-lane groups, the
// group maximum, the rescale and the transposed staging of a matrix.  mu_k and the cell of B_k are phm_ll_device.h's model_mu and
// model_b, one definition for 2..64 states.
#pragma once

#include <hip/hip_runtime.h>

#include "phm_ll_device.h"

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

// ll_rescale's rule (phm_ll_device.h) with the vector across the lanes: this lane's value and the group's maximum
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

}  // namespace phm
