// phm_gibbs_host.h -- what the two posterior samplers of the rates of an index model share on the host: phm_gibbs_rates
// (phm_gibbs_api.cpp, 2..8 states) and phm_gibbs_rates_wide (phm_gibbs_wide_api.cpp, 9..64 states, section
// 25).  The checked input, Q(theta), the one body of both entry points' argument checks (gb_validate), and of a chain's update
// after an iteration the row it records (gb_record), the draw of one rate (gb_draw) and the clock of the phases (GbLap): pure
// host code, no device call.  The chains of a chunk are dealt to host threads by deal_ranges (phm_internal.h).
#pragma once

#include <chrono>
#include <limits>

#include "phm_ancestral_wide.h"
#include "phm_sample_host.h"

namespace phm_ll {

struct GbInput {
  LlInput ll;                                           // K = chains, site_of_model = site_of_chain, Qr = Q(theta0)
  int p = 0, cols = 0, fx_exp = 0, depth = 0, rows = 0, iters = 0, thin = 1, n_prior = 1;
  double theta_max = 0.0, t_max = 0.0;
  std::vector<int32_t> index;                           // [n * n] row-major, 0 = structural zero (and the diagonal)
  std::vector<int32_t> order, level_off;                // s.down positions by the depth of the parent
  const double* theta0 = nullptr;
  const double* prior = nullptr;
  phm_options opt;
  double* theta = nullptr;
  double* loglik = nullptr;
  double* stats = nullptr;
  int32_t* rejected = nullptr;
  int32_t* status = nullptr;
};

// row-major Q(theta) with stride `stride` between entries: q_ij = theta[index - 1], the diagonal minus the row's off-diagonal
// entries summed left to right
inline void fill_q(const GbInput& g, const double* th, double* Q, size_t stride) {
  const int n = g.ll.n;
  for (int i = 0; i < n; ++i) {
    double row = 0.0;
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const int c = g.index[(size_t)i * n + j];
      const double q = c > 0 ? th[c - 1] : 0.0;
      Q[(size_t)(i * n + j) * stride] = q;
      row += q;
    }
    Q[(size_t)(i * n + i) * stride] = -row;
  }
}

// What iteration `iter` records of chain ch, if it is one of the thinned rows: the chain's theta thk, its log-likelihood ll and the
// statistics stat(0 .. cols) -- or NaN throughout for an impossible chain (status set).  False for such a chain: it draws nothing.
template <class Stat>
inline bool gb_record(const GbInput& g, int iter, int64_t ch, const double* thk, double ll, Stat&& stat) {
  const bool live = !g.status[ch];
  if (iter % g.thin == 0) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t at = (size_t)(iter / g.thin) * g.ll.K + ch;
    for (int c = 0; c < g.p; ++c) g.theta[at * g.p + c] = live ? thk[c] : nan;
    g.loglik[at] = live ? ll : nan;
    if (g.stats)
      for (int c = 0; c < g.cols; ++c) g.stats[at * g.cols + c] = live ? stat(c) : nan;
  }
  return live;
}

// The draw of parameter c of chain ch in iteration `iter` from its full conditional Gamma(a + N_c, rate b + W_c), on the stream
// (ENT_RATE | c, chain, iteration + replica_offset); a draw above theta_max (or not positive) is counted and the old value stays.
inline void gb_draw(const GbInput& g, int iter, int64_t ch, int c, double Nc, double Wc, double* thk) {
  const double* pr = g.prior + (g.n_prior > 1 ? (size_t)ch * g.p * 2 : 0);
  phm::HostStream rs{g.opt.seed, phm::ENT_RATE | (uint32_t)c, (uint32_t)ch, (uint32_t)iter + (uint32_t)g.opt.replica_offset};
  const double fresh = rs.gamma(pr[2 * c] + Nc, 1 / (pr[2 * c + 1] + Wc));
  if (fresh > g.theta_max || !(fresh > 0.0)) ++g.rejected[(size_t)ch * g.p + c];
  else thk[c] = fresh;
}

// host clock of the phases of an iteration (q_timing): lap(ms) adds the time since the last lap
struct GbLap {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void operator()(double& ms) {
    const auto t1 = std::chrono::steady_clock::now();
    ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
  }
};

// Every argument check of the two entry points, in one order, and the fill of g; fn prefixes the messages.  wide = false: 2..8
// states (more is PHM_ERR_UNSUPPORTED); wide = true: 9..64 states (2..8 is PHM_ERR_UNSUPPORTED naming phm_gibbs_rates, anything
// outside 2..64 is ll_validate's PHM_ERR_BAD_INPUT).  rejected and chain_status are zeroed on success.
inline int32_t gb_validate(const std::string& fn, bool wide, const phm_tree* x, int32_t n_states, const int32_t* index, int32_t n_params,
                           int32_t n_chains, const double* theta0, const double* prior, int32_t n_prior, double theta_max,
                           const double* pid, int32_t n_pid, const int32_t* observe, const int32_t* site_of_chain, int32_t iters,
                           int32_t thin, const phm_options& o, double* theta, double* loglik, double* stats, int32_t* rejected,
                           int32_t* chain_status, GbInput& g) {
  if (!x || !index || !theta0 || !prior || !pid || !theta || !loglik || !rejected || !chain_status)
    return fail(PHM_ERR_BAD_INPUT, fn + "NULL argument (only observe, site_of_chain, opt and stats may be NULL)");
  const int n = n_states;
  if (wide) {
    if (n < 2 || n > phm::EX_MAX_STATES) return fail(PHM_ERR_BAD_INPUT, fn + "n_states must be in 2..64");   // ll_validate's, before n sizes anything
    if (n < phm::AW_MIN_STATES) return fail(PHM_ERR_UNSUPPORTED, fn + "9..64 states only: 2..8 states go to phm_gibbs_rates");
  } else {
    if (n < 2) return fail(PHM_ERR_BAD_INPUT, fn + "n_states must be in 2..8");
    if (n > phm::LL_LANE_MAX) return fail(PHM_ERR_UNSUPPORTED, fn + "more than 8 states are not supported");
  }
  if (n_chains < 1) return fail(PHM_ERR_BAD_INPUT, fn + "n_chains must be >= 1");
  if (n_params < 1 || n_params > n * (n - 1)) return fail(PHM_ERR_BAD_INPUT, fn + "n_params must be in 1..n(n-1)");
  if (iters < 1) return fail(PHM_ERR_BAD_INPUT, fn + "iters must be >= 1");
  if (thin < 1) return fail(PHM_ERR_BAD_INPUT, fn + "thin must be >= 1");
  if (n_prior != 1 && n_prior != n_chains) return fail(PHM_ERR_BAD_INPUT, fn + "n_prior must be 1 (shared) or n_chains");
  if (!(theta_max > 0.0) || !std::isfinite(theta_max)) return fail(PHM_ERR_BAD_INPUT, fn + "theta_max must be positive and finite");
  g.p = n_params; g.iters = iters; g.thin = thin; g.n_prior = n_prior; g.theta_max = theta_max;
  g.rows = (iters + thin - 1) / thin;
  g.index.assign((size_t)n * n, 0);
  std::vector<int> owned(n_params, 0);
  int row_max = 0;
  for (int i = 0; i < n; ++i) {
    int in_row = 0;
    for (int j = 0; j < n; ++j) {
      const int32_t c = i == j ? 0 : index[i + (size_t)j * n];                // column-major in, the diagonal is ignored
      if (c > n_params) return fail(PHM_ERR_BAD_INPUT, fn + "index: entry (" + std::to_string(i + 1) + ", " + std::to_string(j + 1) + ") names parameter " + std::to_string(c) + " of " + std::to_string(n_params));
      if (c > 0) { g.index[(size_t)i * n + j] = c; ++owned[c - 1]; ++in_row; }
    }
    row_max = std::max(row_max, in_row);
  }
  for (int c = 0; c < n_params; ++c)
    if (!owned[c]) return fail(PHM_ERR_BAD_INPUT, fn + "index: parameter " + std::to_string(c + 1) + " owns no entry (parameters are numbered 1..p without gaps)");
  for (int64_t k = 0; k < (int64_t)n_prior; ++k)
    for (int c = 0; c < n_params; ++c) {
      const double a = prior[((size_t)k * n_params + c) * 2], b = prior[((size_t)k * n_params + c) * 2 + 1];
      if (!(a > 0.0) || !(b > 0.0) || !std::isfinite(a) || !std::isfinite(b))
        return fail(PHM_ERR_BAD_INPUT, fn + "prior: shape and rate of parameter " + std::to_string(c + 1) + " (prior row " + std::to_string(k) + ") must be positive and finite");
    }
  for (int64_t k = 0; k < n_chains; ++k)
    for (int c = 0; c < n_params; ++c) {
      const double v = theta0[(size_t)k * n_params + c];
      if (!(v > 0.0) || !(v <= theta_max))
        return fail(PHM_ERR_BAD_INPUT, fn + "theta0 of chain " + std::to_string(k) + ", parameter " + std::to_string(c + 1) + " must be in (0, theta_max]");
    }
  const int S = std::max(1, (int)o.n_replicas);
  if (site_of_chain)
    for (int64_t k = 0; k < n_chains; ++k)
      if (site_of_chain[k] < 0 || site_of_chain[k] >= S)
        return fail(PHM_ERR_BAD_INPUT, fn + "site_of_chain[" + std::to_string(k) + "]: the site of chain " + std::to_string(k) + " must be in 0..S-1");
  if ((int64_t)S * n_chains > (int64_t)INT32_MAX) return fail(PHM_ERR_BAD_INPUT, fn + "sites * chains must fit in 31 bits (evaluation ids)");
  if (!site_of_chain && S > 65535) return fail(PHM_ERR_UNSUPPORTED, fn + "more than 65535 sites per chain (joint mode)");

  // ll_validate on Q(theta0): the tree, the root priors, the tips, observe and the options
  const size_t nn = (size_t)n * n;
  std::vector<double> Q0((size_t)n_chains * nn), qr(nn);
  g.ll.n = n;
  for (int64_t k = 0; k < n_chains; ++k) {
    fill_q(g, theta0 + (size_t)k * n_params, qr.data(), 1);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) Q0[(size_t)k * nn + i + (size_t)j * n] = qr[(size_t)i * n + j];
  }
  int32_t st = ll_validate(fn, x, n, n_chains, Q0.data(), pid, n_pid, observe, site_of_chain, o, g.ll);
  if (st) return st;
  const LlInput& in = g.ll;
  double tree_len = 0.0;
  for (int b = 0; b < in.E; ++b) { g.t_max = std::max(g.t_max, in.edge_length[b]); tree_len += in.edge_length[b]; }
  // theta_max bounds every chain's uniformization rate for the whole run: the table is allocated once, to the depth it allows
  const double x_max = ((double)row_max * theta_max) * g.t_max;
  if (x_max > phm::SM_MAX_JUMP_MEAN)
    return fail(PHM_ERR_UNSUPPORTED, fn + "theta_max: (largest number of rates in a row = " + std::to_string(row_max) +
                                         ") * theta_max * (longest branch) is above 32768; lower theta_max");
  g.depth = phm::sm_stop_index(x_max);
  (void)std::frexp(std::max(tree_len, 1.0), &g.fx_exp);
  g.cols = n + n * (n - 1);
  phm::depth_levels(in.sched, g.order, g.level_off);
  g.theta0 = theta0; g.prior = prior; g.opt = o;
  g.theta = theta; g.loglik = loglik; g.stats = stats; g.rejected = rejected; g.status = chain_status;
  std::fill_n(rejected, (size_t)n_chains * n_params, 0);
  std::fill_n(chain_status, (size_t)n_chains, 0);
  return PHM_OK;
}

}  // namespace phm_ll
