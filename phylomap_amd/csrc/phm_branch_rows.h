// phm_branch_rows.h -- launchers of the per-branch expected statistics for many rate matrices at 2..8 states
// (phm_branch_rows.hip) and of the label reduction that serves 2..64 states, behind phm_expected_branch_stats_models
// (phm_branch_rows_api.cpp).  DESIGN.md section 27.
#pragma once

#include "phm_scores.h"

namespace phm {

constexpr int BR_MAX_LABELS = 65535;           // labels of one call: a grid dimension of the reduction
constexpr int BR_GRID_MAX = 65535;             // selected edges of one launch (LL_GRID_Y, AW_GRID_MAX)

// Branch stage of `count` selected edge rows sel[0 .. count) (device; any order, repeats allowed), after section 18's passes on
// p (launch_sc_model, launch_sc_root, launch_sc_down; p.runs and p.tot are not read).  rows[(j * n * n + col) * Eo + eo] gets
// the finished row of edge sel[j]: column col of evaluation eo = site * Kc + model of Eo = n_sites * Kc (the chunk's models without
// the lanes that pad them to 64), exactly the value sc_branch_kernel adds into its run total.
hipError_t launch_br_branch(const ScParams& p, const int32_t* sel, int count, double* rows, hipStream_t stream);

// Labelled sums of finished rows.  Row j, evaluation ev, column col is rows[j * row_j + ev * row_ev + col * row_col] (the two
// families lay their rows out differently); w is [n_labels][cols].  out[(j * n_labels + l) * n_ev + ev] =
// (((0 + w[l][0] row[0]) + w[l][1] row[1]) + ..): every product and every sum rounded on its own, no fma.
struct BrLabelParams {
  const double* rows;
  const double* w;
  double* out;
  int32_t cols, n_labels, count;               // count: rows j of the launch
  int64_t n_ev;
  int64_t row_j, row_ev, row_col;
};
hipError_t launch_br_labels(const BrLabelParams& p, hipStream_t stream);

}  // namespace phm
