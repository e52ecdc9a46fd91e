// phm_time_models_wide.h -- kernel parameter block and launchers of the exact expectations through time for many rate matrices at
// 9..64 states (phm_time_models_wide.hip), behind phm_expected_through_time_models_wide (phm_time_models_wide_api.cpp).
// DESIGN.md section 29.
#pragma once

#include "phm_scores_wide.h"
#include "phm_time_models.h"
#include "phm_time_models_wide_form.h"

namespace phm {

constexpr int TMW_WALK = 16;                   // consecutive items of a launch a workgroup walks through its model's staged B
constexpr int TMW_SITES = 4;                   // sites a group walks (SCW_WALK)
// groups of NP lanes in a workgroup of the along and branch stages (scw_branch_kernel's shape): a workgroup's site tile is
// tmw_groups(NP) * TMW_SITES sites
inline int tmw_groups(int NP) { return NP == 16 ? 4 : 2; }

// Section 23's buffers with lam, F and sF stored and section 26's Q, t, child, mu and B (sc; sc.form, sc.runs and sc.tot are not
// read), and what the stages of section 29 add.  One state per lane: an evaluation of the chunk is ev = model * Sc + site of
// Ev = Kc * Sc; an item of the launch (TmItem: a point pair on a branch) has slot j = 0 .. count - 1 in every buffer below.
struct TmwParams {
  ScwParams sc;
  const TmItem* items;                         // [count] of this launch (device)
  double* post;                                // posterior mode: [item][Ev][n]; NULL: a, sa, beta, sbeta are written
  double* a;                                   // [item][Ev][NP] rescaled forward vectors, the states past n zero
  int32_t* sa;                                 // [item][Ev] their base-2 exponents (sF_b included)
  double* beta;                                // [item][Ev][NP] rescaled backward vectors
  int32_t* sbeta;                              // [item][Ev] their base-2 exponents (sL_c included)
  double* rows;                                // [item][Ev][n * n] sub-branch rows in phm_expected_stats' column order
};

// a and / or beta of `count` items (at most TM_GRID_MAX); posterior mode when p.post is set
hipError_t launch_tmw_along(const TmwParams& p, int count, hipStream_t stream);
// the branch stage over `count` sub-branches whose a, beta were written by launch_tmw_along into the same item slots
hipError_t launch_tmw_branch(const TmwParams& p, int count, hipStream_t stream);
// tot[range][cell] += x[item][cell] over the items of ranges [r_begin, r_end) that lie in [q0, q0 + count): range r is items
// off[r] .. off[r + 1] - 1 (global item numbers); x holds items q0 .. q0 + count - 1, `cells` values each ([Ev][col]).  In item
// order, continued from tot: tm_range_sum_kernel's sum for the layout of this family.
hipError_t launch_tmw_range_sum(const double* x, int64_t cells, int count, int64_t q0, const int64_t* off, int r_begin, int r_end,
                                int n_ranges, double* tot, hipStream_t stream);

}  // namespace phm
