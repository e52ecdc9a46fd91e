// phm_time_models_wide_host.h -- the pure host pieces that phm_expected_through_time_models_wide (phm_time_models_wide_api.cpp,
// DESIGN.md section 29) adds to section 28's (phm_time_models_host.h: the checks of the bounds and the points, the plan, the items
// of a launch) and section 27's (phm_branch_rows_host.h: the labels, the fit of a chunk): the state counts it serves, what an
// evaluation takes on the device on top of aw_plan's own footprint, what an item of a launch writes, and how many models, sites
// and items a launch takes.  No HIP call and no library state (tests/native/time_models_wide_host_check.cpp runs all of it
// without a device).
#pragma once

#include "phm_ancestral_wide.h"
#include "phm_branch_rows_host.h"
#include "phm_time_models_host.h"

namespace phm_tmw {

inline bool tmw_serves(int n) { return n >= phm::AW_MIN_STATES && n <= phm::EX_MAX_STATES; }

// doubles one (item, evaluation) pair writes in a launch of points: the posterior
inline size_t tmw_point_cell(int n) { return (size_t)n; }
// .. and in a launch of sub-branches: a and beta (NP each), their exponents and the row
inline size_t tmw_sub_cell(int n) { return 2 * (size_t)phm::aw_lanes(n) + 2 + (size_t)n * n; }

// bytes an evaluation of a chunk takes on top of aw_plan's own: O and F with their exponents, lam, and the sums per boundary,
// per bin and per labelled bin that are asked for
inline size_t tmw_per_eval_bytes(int n, int NT, int E, int n_bounds, bool occ, bool bins, int n_labels) {
  const size_t vec_b = sizeof(double) * (size_t)phm::aw_lanes(n) + sizeof(int32_t);
  const size_t NB = (size_t)std::max(0, n_bounds - 1);
  return vec_b * (size_t)NT + vec_b * (size_t)E + sizeof(double) *
         (1 + (occ ? (size_t)n * (size_t)n_bounds : 0) + (bins ? (size_t)n * n * NB : 0) + (bins ? (size_t)n_labels * NB : 0));
}

struct TmwLaunch {
  int np_max = 0, ns_max = 0;                           // points and sub-branches of one launch (0: the call has none)
};

// Shrinks the chunk of Kc_max models x Sc_max sites until one item of the larger kind fits in the scratch (br_fit_chunk: models
// first, then sites), then sizes the launches: at most 65 535 items, at most `chunk` (phm_debug_options.expect_chunk) and at most
// what keeps a launch's writes within TM_SCRATCH.
inline TmwLaunch tmw_launches(int n, int64_t n_points, int64_t n_sub, int chunk, int64_t& Kc_max, int64_t& Sc_max) {
  phm_br::br_fit_chunk(n_sub ? tmw_sub_cell(n) : tmw_point_cell(n), 1, Kc_max, Sc_max);
  const size_t Evm = (size_t)Kc_max * (size_t)Sc_max;
  TmwLaunch l;
  if (n_points) l.np_max = phm_tm::tm_items_per_launch(n_points, tmw_point_cell(n), Evm, chunk);
  if (n_sub) l.ns_max = phm_tm::tm_items_per_launch(n_sub, tmw_sub_cell(n), Evm, chunk);
  return l;
}

}  // namespace phm_tmw
