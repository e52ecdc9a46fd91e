// phm_loglik_host.h -- host side shared by the entry points that take many rate matrices in one call: phm_loglik_models
// (phm_loglik_api.cpp) and phm_expected_stats_models (phm_scores_api.cpp, section 18).  The checked input
// and the one validation both run before any device call.
#pragma once

#include "phm_expect_host.h"
#include "phm_loglik.h"

namespace phm_ll {

constexpr size_t LL_WORK = size_t(256) << 20;          // 5..8 states: Pade matrices of one P launch

// What every device of a call shares.
struct LlInput {
  int n = 0, T = 0, Nn = 0, E = 0, NT = 0, S = 0, K = 0;
  bool per_site = false, paired = false;
  const int32_t* states = nullptr;
  const int32_t* site_of_model = nullptr;
  phm::Schedule sched;
  std::vector<double> Qr;                               // [K][n * n] row-major
  std::vector<double> pid;                              // [K][n] normalised
  std::vector<double> edge_length;
  std::vector<int32_t> obs;
  std::vector<phm::UpStep> up;                          // grouped by height
  std::vector<int32_t> up_off;
  const int32_t* tips_of(int64_t site) const { return states + (per_site ? site * T : 0); }
};

// tree, models, root priors, tips, observe, site_of_model and option checks (no device call); fn prefixes the messages
int32_t ll_validate(const std::string& fn, const phm_tree* x, int32_t n, int32_t K, const double* Q, const double* pid, int32_t n_pid,
                    const int32_t* observe, const int32_t* site_of_model, const phm_options& o, LlInput& in);

// out[(site, model)]: cross S x K with the site fastest, paired K
inline double& ll_out(const LlInput& in, double* out, int64_t site, int64_t model) {
  return in.paired ? out[model] : out[site + (int64_t)in.S * model];
}

}  // namespace phm_ll
