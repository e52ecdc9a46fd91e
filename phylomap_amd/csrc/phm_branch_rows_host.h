// phm_branch_rows_host.h -- the pure host pieces of phm_expected_branch_stats_models (phm_branch_rows_api.cpp, DESIGN.md section
// 27): the checked edge selection and label weights, the limit on mu t_b over the selected edges, and how many models, sites and
// selected edges one branch-stage launch may take so that its rows stay within the scratch bound.  No HIP call and no library
// state: a refusal comes back as a status and a message (tests/native/branch_rows_host_check.cpp runs all of it without a device).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/phylomap_hip.h"

namespace phm_br {

constexpr size_t BR_SCRATCH = size_t(256) << 20;       // finished rows of one branch-stage launch (and, apart, its labelled sums)
constexpr int BR_LABELS_MAX = 65535;                    // phm::BR_MAX_LABELS

struct BrSelection {
  std::vector<int32_t> edges;                           // [n_sel] 0-based edge rows, the caller's order
  int n_sel = 0;
  int n_labels = 0;                                     // 0: full rows
  int out_cols = 0;                                     // C of the output: n * n, or n_labels
  std::vector<double> w;                                // [n_labels][n * n] label weights in phm_expected_stats' column order
};

// the column of E[N_ij], i != j, behind the n dwell columns (phm::count_col on the host)
inline int br_count_col(int n, int i, int j) { return n + i * (n - 1) + (j < i ? j : j - 1); }

// edges == NULL: every edge row in row order (n_edges ignored).  labels: [n_labels][n][n], each matrix column-major as Q is;
// (i, i) weighs E[dwell_i], (i, j) weighs E[N_ij].
inline int32_t br_select(int n, int E, int32_t n_edges, const int32_t* edges, int32_t n_labels, const double* labels, BrSelection& sel,
                         std::string& err) {
  if (edges) {
    if (n_edges < 1) { err = "n_edges must be >= 1 when edges is given"; return PHM_ERR_BAD_INPUT; }
    for (int32_t j = 0; j < n_edges; ++j)
      if (edges[j] < 0 || edges[j] >= E) {
        err = "edges[" + std::to_string(j) + "] = " + std::to_string(edges[j]) + " is outside 0.." + std::to_string(E - 1);
        return PHM_ERR_BAD_INPUT;
      }
    sel.edges.assign(edges, edges + n_edges);
  } else {
    sel.edges.resize((size_t)E);
    for (int b = 0; b < E; ++b) sel.edges[b] = b;
  }
  sel.n_sel = (int)sel.edges.size();
  const int cols = n * n;
  sel.n_labels = 0;
  sel.out_cols = cols;
  sel.w.clear();
  if (!labels) return PHM_OK;
  if (n_labels < 1) { err = "n_labels must be >= 1 when labels is given"; return PHM_ERR_BAD_INPUT; }
  if (n_labels > BR_LABELS_MAX) { err = "n_labels must be at most " + std::to_string(BR_LABELS_MAX); return PHM_ERR_BAD_INPUT; }
  const size_t nn = (size_t)cols;
  for (size_t e = 0; e < nn * (size_t)n_labels; ++e)
    if (!std::isfinite(labels[e])) {
      err = "label " + std::to_string(e / nn) + " has a non-finite weight";
      return PHM_ERR_BAD_INPUT;
    }
  sel.n_labels = n_labels;
  sel.out_cols = n_labels;
  sel.w.assign(nn * (size_t)n_labels, 0.0);
  for (int l = 0; l < n_labels; ++l)
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) sel.w[(size_t)l * nn + (i == j ? i : br_count_col(n, i, j))] = labels[(size_t)l * nn + (size_t)j * n + i];
  return PHM_OK;
}

// max(-q_ii) of K row-major matrices
inline void br_model_mu(const double* Qr, int n, int K, std::vector<double>& mu) {
  const size_t nn = (size_t)n * n;
  mu.assign((size_t)K, 0.0);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < n; ++i) mu[k] = std::max(mu[k], -Qr[(size_t)k * nn + (size_t)i * n + i]);
}

// The branch stage runs ~mu t_b steps: mu_k t_b above `limit` on a SELECTED edge is refused, naming the model and the edge row
// (1-based, as phm_expected_stats_models names it).  An edge that is not selected is not held to it.
inline int32_t br_check_jump_mean(const std::vector<double>& mu, const double* t, const BrSelection& sel, double limit, std::string& err) {
  for (size_t k = 0; k < mu.size(); ++k)
    for (int32_t b : sel.edges)
      if (mu[k] * t[b] > limit) {
        err = "model " + std::to_string(k) + ", edge row " + std::to_string(b + 1) + ": max(-q_ii) * t_b above 1e6";
        return PHM_ERR_UNSUPPORTED;
      }
  return PHM_OK;
}

// doubles one (selected edge, evaluation) pair takes in the larger of the two scratch buffers: its row, or its labelled sums
inline size_t br_cell_doubles(int n, const BrSelection& sel) { return std::max<size_t>((size_t)n * n, (size_t)sel.n_labels); }

// Shrinks a chunk of Kc_max models x Sc_max sites until ONE selected edge's rows fit in BR_SCRATCH: first the models, in units of
// k_unit (64 with the models across the lanes, 1 with a state per lane) and never below one unit, then the sites, never below 1.
inline void br_fit_chunk(size_t cell_doubles, int64_t k_unit, int64_t& Kc_max, int64_t& Sc_max) {
  const size_t cell_b = sizeof(double) * cell_doubles;
  if (cell_b * (size_t)Kc_max * (size_t)Sc_max <= BR_SCRATCH) return;
  Kc_max = std::max<int64_t>(k_unit, (int64_t)(BR_SCRATCH / (cell_b * (size_t)Sc_max)) / k_unit * k_unit);
  if (cell_b * (size_t)Kc_max * (size_t)Sc_max > BR_SCRATCH) Sc_max = std::max<int64_t>(1, (int64_t)(BR_SCRATCH / (cell_b * (size_t)Kc_max)));
}

// selected edges of one branch-stage launch for chunks of Evm evaluations; chunk: phm_debug_options.expect_chunk
inline int br_edges_per_launch(int n_sel, size_t cell_doubles, size_t Evm, int chunk, int grid_max) {
  const size_t fit = BR_SCRATCH / (sizeof(double) * cell_doubles * std::max<size_t>(Evm, 1));
  int ne = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n_sel, (size_t)grid_max, fit}));
  if (chunk > 0) ne = std::min(ne, chunk);
  return ne;
}

}  // namespace phm_br
