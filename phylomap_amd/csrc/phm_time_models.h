// phm_time_models.h -- kernel parameter block and launchers of the exact expectations through time for many rate matrices at
// 2..8 states (phm_time_models.hip), behind phm_expected_through_time_models (phm_time_models_api.cpp).  DESIGN.md section 28.
#pragma once

#include "phm_scores.h"

namespace phm {

constexpr int TM_GRID_MAX = 65535;             // most items of one along / branch launch (grid y)

// A point pair on a branch: a = P(t1)^T F_b from the parent end and beta = P(t2) L_c towards the child.  A point at position s
// has t1 = s, t2 = t_b - s and h unused; a sub-branch [s1, s2] has t1 = s1, t2 = t_b - s2 and h = s2 - s1.
struct TmItem {
  int32_t edge, pad;
  double t1, t2, h;
};

// The passes' buffers (sc: section 18's, section 17's inside) and what the stages of section 28 add.  Everything the new stages
// write holds the chunk's Kc models alone, not the padded lanes: Eo = n_sites * Kc values per row, evaluation site * Kc + k.
struct TmParams {
  ScParams sc;
  const TmItem* items;                         // [count] of this launch (device)
  double* post;                                // posterior mode: [item][n][Eo]; NULL: a, sa, beta, sbeta are written
  double* a;                                   // [item][n][Eo] rescaled forward vectors
  double* sa;                                  // [item][Eo] their base-2 exponents (sF_b included)
  double* beta;                                // [item][n][Eo] rescaled backward vectors
  double* sbeta;                               // [item][Eo] their base-2 exponents (sL_c included)
  double* rows;                                // [item][n * n][Eo] sub-branch rows in phm_expected_stats' column order
};

// a and / or beta of `count` items (at most TM_GRID_MAX); posterior mode when p.post is set
hipError_t launch_tm_along(const TmParams& p, int count, hipStream_t stream);
// the branch stage over `count` sub-branches whose a, beta were written by launch_tm_along into the same item slots
hipError_t launch_tm_branch(const TmParams& p, int count, hipStream_t stream);
// tot[col][range][Eo] += x[item][col][Eo] over the items of ranges [r_begin, r_end) that lie in [q0, q0 + count): range r is
// items off[r] .. off[r + 1] - 1 (global item numbers); x holds items q0 .. q0 + count - 1.  In item order, continued from tot.
hipError_t launch_tm_range_sum(const double* x, int cols, int count, int64_t q0, const int64_t* off, int r_begin, int r_end,
                               int n_ranges, int64_t Eo, double* tot, hipStream_t stream);

}  // namespace phm
