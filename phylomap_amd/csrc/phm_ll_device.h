// phm_ll_device.h -- the device pieces of the one-model-per-lane kernels at 2..8 states, shared by
// phm_loglik.hip, phm_scores.hip, phm_ancestral.hip and phm_sample.hip: the dispatch on the state count, what a lane works on, the
// rescale, the grid of a launch and the range check of its launcher.  mu_k and the cell of B_k are here for both families
// (phm_aw_device.h includes this header), and phm_expect.hip takes the dispatch and LL_GRID_Y for its one-site-per-lane branch
// kernels; LN2 and count_col are phm_expect.h's.
#pragma once

#include <type_traits>

#include "phm_expect.h"
#include "phm_loglik.h"

namespace phm {

constexpr int LL_GRID_Y = 65535;               // most rows (edges, steps, columns) and most sites of one launch

// f(std::integral_constant<int, N>) of the state count, its value returned: constexpr int N = decltype(ns)::value
template <class F>
inline auto ll_with_states(int n, F&& f) {
  switch (n) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

// what a lane of a BLOCK-wide workgroup works on: model k and evaluation ev = (site blockIdx.z) * Kp + k of Ev; idle: no model
struct LlLane {
  int k;
  size_t Kp, Ev, ev;
  bool idle;
};
template <int BLOCK> __device__ __forceinline__ LlLane ll_lane(const LlParams& q) {
  const int k = blockIdx.x * BLOCK + threadIdx.x;
  const size_t Kp = q.Kp;
  return {k, Kp, (size_t)q.n_sites * Kp, (size_t)blockIdx.z * Kp + k, k >= q.Kc};
}

// THE rescale rule of every pass: v[0 .. N) scaled by 2^-e with max in [1/2, 1); returns e (0 for an all-zero vector)
template <int N>
__device__ __forceinline__ int ll_rescale(double (&v)[N], double mx) {
  if (!(mx > 0.0)) return 0;
  int e = 0;
  (void)frexp(mx, &e);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = ldexp(v[i], -e);
  return e;
}

// mu_k = max_i(-q_ii); st: the stride between the entries of Q_k (Kp in the model-fastest buffers, 1 in a matrix of its own)
__device__ __forceinline__ double model_mu(const double* __restrict__ Qk, size_t st, int n) {
  double mu = 0.0;
  for (int i = 0; i < n; ++i) mu = fmax(mu, -Qk[(size_t)(i * n + i) * st]);
  return mu;
}

// one cell of B_k = I + Q_k / mu_k (I when mu_k = 0): q the cell of Q_k, d the cell of I
__device__ __forceinline__ double model_b(double q, double mu, double d) { return mu > 0.0 ? d + q / mu : d; }

inline dim3 model_grid(const LlParams& q, int block, int y, int z) { return dim3((q.Kp + block - 1) / block, y, z); }

inline bool ll_sites_ok(const LlParams& q) { return q.n_sites >= 1 && q.n_sites <= LL_GRID_Y; }
inline bool ll_states_ok(const LlParams& q) { return q.n >= 2 && q.n <= LL_LANE_MAX; }
// what every launcher of the scores and the ancestral kernels asks of its LlParams
inline bool ll_ok(const LlParams& q) { return ll_states_ok(q) && q.Kp % 64 == 0 && ll_sites_ok(q); }

}  // namespace phm
