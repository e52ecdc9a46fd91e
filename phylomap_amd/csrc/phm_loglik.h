// phm_loglik.h -- kernel parameter block and launchers of the batched log-likelihood over many rate matrices (phm_loglik.hip),
// behind phm_loglik_models (phm_loglik_api.cpp).  DESIGN.md section 17.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "phm_sched.h"

namespace phm {

constexpr int LL_LANE_MAX = 8;                 // n <= 8: models across the lanes; 9..64 states are not batched (phm_loglik_api.cpp)
constexpr int LL_REG_MAX = 4;                  // n <= 4: the Pade matrices of a lane live in registers; 5..8: in `work`

// An evaluation is (model k, site s).  Every per-model buffer is [row][Kp] and every per-evaluation buffer [row][Ev] with the
// model index fastest: Ev = n_sites * Kp, evaluation s * Kp + k.  Kp is a multiple of 64; lanes k >= Kc do nothing.
struct LlParams {
  int32_t n, n_tips, Kp, Kc;
  int32_t n_sites;                             // sites of this launch (grid z); 1 in paired mode
  int32_t paired;                              // 0: tips[site][tip], uniform over a wave; 1: tips[tip][Kp], one byte per lane
  const double* Q;                             // [n * n][Kp] row-major entries
  const double* pid;                           // [n][Kp] normalised root priors
  const double* t;                             // [n_edge] branch lengths
  double* P;                                   // [n_edge][n * n][Kp] row-major entries of expm(Q_k t_b)
  double* work;                                // 5..8 states: [edge of the launch][4][n * n][Kp]
  uint32_t* bad;                               // [Kp] non-zero: a zero pivot in some P of the model (its evaluations are -inf)
  const uint8_t* tips;
  const int32_t* obs;                          // [n]
  double* L;                                   // [node row][n][Ev] rescaled partial likelihoods
  double* sL;                                  // [node row][Ev] base-2 exponents
  double* ll;                                  // [Ev] log p(tips_s | Q_k, pid_k), -inf for probability 0
};

// P of edge rows [e0, e0 + count); with 5..8 states count is at most the number of edges `work` holds
hipError_t launch_ll_expm(const LlParams& p, int e0, int count, hipStream_t stream);
hipError_t launch_ll_tips(const LlParams& p, hipStream_t stream);
// one height level of the up pass: `steps` (device) holds `count` UpStep entries
hipError_t launch_ll_up(const LlParams& p, const UpStep* steps, int count, hipStream_t stream);
hipError_t launch_ll_root(const LlParams& p, int root_row, hipStream_t stream);

}  // namespace phm
