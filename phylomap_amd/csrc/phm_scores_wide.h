// phm_scores_wide.h -- kernel parameter block and launchers of the exact conditional expectations for many rate matrices at
// 9..64 states (phm_scores_wide.hip), behind phm_expected_stats_models_wide (phm_scores_wide_api.cpp).  DESIGN.md section 26.
#pragma once

#include "phm_ancestral_wide.h"
#include "phm_scores.h"
#include "phm_scores_wide_form.h"

namespace phm {

// Section 23's buffers (aw: P, pid, L, sL, O, sO, the root's lam and the down pass' F, sF, and the layout rules of AwParams: one
// state per lane, ev = model * Sc + site, rows of NP doubles with the states past n zero, int32 exponents) and what the branch
// stage adds.
struct ScwParams {
  AwParams aw;
  const double* Q;                             // [model][n][n] row-major
  const double* t;                             // [n_edge] branch lengths
  const int32_t* child;                        // [n_edge] node row of each edge's child
  double* mu;                                  // [model] max_i(-q_ii)
  double* B;                                   // [model][n][n] row-major I + Q_k / mu_k (I when mu_k = 0)
  const int32_t* form;                         // [model][n_edge] sw_form_terms(mu_k t_b, SW_M_CAP): M of the short form, or SW_M_CAP + 1
  double* runs;                                // [run of the launch][Ev][col] totals of SC_RUN edge rows each
  double* tot;                                 // [Ev][col], cols = n + n(n-1) (phm_expected_stats' column order)
};

// mu_k and B_k of the chunk's models
hipError_t launch_scw_model(const ScwParams& p, hipStream_t stream);
// branch stage (after launch_aw_root with lam and launch_aw_down with F, sF on p.aw) of runs [r0, r0 + count): run r is edge rows [r SC_RUN, min(n_edge, (r + 1) SC_RUN)); runs[r - r0] gets its total
hipError_t launch_scw_branch(const ScwParams& p, int r0, int count, hipStream_t stream);
// tot += runs[0] + .. + runs[count - 1], one after the other (tot is continued across launches: the order is the run order)
hipError_t launch_scw_total(const ScwParams& p, int count, hipStream_t stream);

}  // namespace phm
