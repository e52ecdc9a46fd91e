// phm_branch_rows_wide.h -- launcher of the per-branch expected statistics for many rate matrices at 9..64 states
// (phm_branch_rows_wide.hip), behind phm_expected_branch_stats_models (phm_branch_rows_api.cpp).  DESIGN.md section 27.
#pragma once

#include "phm_scores_wide.h"

namespace phm {

// Branch stage of `count` selected edge rows sel[0 .. count) (device; any order, repeats allowed), after section 23's passes with
// lam, F and sF stored and launch_scw_model on q (q.runs and q.tot are not read).  rows[(j * Ev + ev) * n * n + col] gets the
// finished row of edge sel[j], Ev = Kc * Sc: exactly the value scw_branch_kernel adds into its run total, in the form
// (short or long) q.form gives the (model, edge) item.
hipError_t launch_brw_branch(const ScwParams& q, const int32_t* sel, int count, double* rows, hipStream_t stream);

}  // namespace phm
