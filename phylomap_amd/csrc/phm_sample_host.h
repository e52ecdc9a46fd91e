// phm_sample_host.h -- what the two exact samplers of histories share on the host: phm_sample_histories_models
// (phm_sample_api.cpp, 2..8 states) and phm_sample_histories_models_wide (phm_sample_wide_api.cpp, 9..64
// states, section 24).  The checked input and the checks that follow ll_validate; no device call.
#pragma once

#include "phm_loglik_host.h"
#include "phm_sample.h"

namespace phm_ll {

struct SmInput {
  LlInput ll;
  int cols = 0, D = 0, fx_exp = 0;
  int64_t n_eval = 0, H = 0;                            // evaluations, histories
  std::vector<int32_t> depth;                           // [K] M(mu_k max_b t_b)
  std::vector<int32_t> order, level_off;                // s.down positions by the depth of the parent
  phm_options opt;
  int32_t* nodes = nullptr;
};

// draws, the state count (outside n_lo .. n_hi: PHM_ERR_UNSUPPORTED with fn + range_msg), the 31-bit evaluation ids, the count
// of histories, max(-q_ii) t_b of every model and branch, and from them every model's table depth and the depth levels
inline int32_t sm_prepare(const std::string& fn, int n_lo, int n_hi, const char* range_msg, SmInput& sm, int32_t draws) {
  LlInput& in = sm.ll;
  const int n = in.n;
  if (draws < 1) return fail(PHM_ERR_BAD_INPUT, fn + "draws must be >= 1");
  if (n < n_lo || n > n_hi) return fail(PHM_ERR_UNSUPPORTED, fn + range_msg);
  if ((int64_t)in.S * in.K > (int64_t)INT32_MAX) return fail(PHM_ERR_BAD_INPUT, fn + "sites * models must fit in 31 bits (evaluation ids)");
  sm.cols = n + n * (n - 1);
  sm.D = draws;
  sm.n_eval = in.paired ? in.K : (int64_t)in.S * in.K;
  if (sm.n_eval > INT64_MAX / 4096 / draws) return fail(PHM_ERR_BAD_INPUT, fn + "evaluations * draws overflows");
  sm.H = sm.n_eval * draws;
  const size_t nn = (size_t)n * n;
  double t_max = 0.0, tree_len = 0.0;
  for (int b = 0; b < in.E; ++b) { t_max = std::max(t_max, in.edge_length[b]); tree_len += in.edge_length[b]; }
  (void)std::frexp(std::max(tree_len, 1.0), &sm.fx_exp);
  sm.depth.resize(in.K);
  for (int k = 0; k < in.K; ++k) {
    double mu = 0.0;
    for (int i = 0; i < n; ++i) mu = std::max(mu, -in.Qr[(size_t)k * nn + (size_t)i * n + i]);
    for (int b = 0; b < in.E; ++b)
      if (mu * in.edge_length[b] > phm::SM_MAX_JUMP_MEAN)
        return fail(PHM_ERR_UNSUPPORTED, "model " + std::to_string(k) + ", edge row " + std::to_string(b + 1) + ": max(-q_ii) * t_b above 32768");
    sm.depth[k] = phm::sm_stop_index(mu * t_max);
  }
  phm::depth_levels(in.sched, sm.order, sm.level_off);
  return PHM_OK;
}

}  // namespace phm_ll
