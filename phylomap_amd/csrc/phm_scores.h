// phm_scores.h -- kernel parameter block and launchers of the exact conditional expectations for many rate matrices at once
// (phm_scores.hip), behind phm_expected_stats_models (phm_scores_api.cpp).  DESIGN.md section 18.
#pragma once

#include "phm_expect.h"
#include "phm_loglik.h"

namespace phm {

constexpr int SC_RUN = 16;                     // consecutive edge rows one lane of the branch stage adds up, in edge order
constexpr int SC_M_CAP = 1 << 21;              // hard end of a lane's uniformization loop (the host refuses mu t_b above 1e6)

// Section 17's buffers (ll: Q, pid, t, P, tips, obs, L, sL, ll and the layout rules of LlParams) and what the down pass and the
// branch stage add.  Per-evaluation buffers are [row][state][Ev] or [row][Ev], the model index fastest.
struct ScParams {
  LlParams ll;
  int32_t n_edge, root;                        // root: node row of the root
  double* mu;                                  // [Kp] max_i(-q_ii)
  double* B;                                   // 5..8 states: [n * n][Kp] row-major I + Q_k / mu_k (I when mu_k = 0); else NULL
  const int32_t* child;                        // [n_edge] node row of each edge's child
  double* O;                                   // [node row][n][Ev] rescaled outside vectors
  double* sO;                                  // [node row][Ev]
  double* F;                                   // [edge row][n][Ev] F_b = O_parent (.) P(t_sib) L_sib
  double* sF;                                  // [edge row][Ev]
  double* lam;                                 // [Ev] pid . L_root (rescaled)
  double* runs;                                // [run of the launch][col][Ev] totals of SC_RUN edge rows each
  double* tot;                                 // [col][Ev], cols = n + n(n-1) (phm_expected_stats' column order)
};

// mu_k and, with 5..8 states, B_k
hipError_t launch_sc_model(const ScParams& p, hipStream_t stream);
// O_root = pid_k, sO_root = 0, lam = pid_k . L_root (after the up pass)
hipError_t launch_sc_root(const ScParams& p, hipStream_t stream);
// one depth level of the down pass: `steps` (device) holds `count` ExDown entries
hipError_t launch_sc_down(const ScParams& p, const ExDown* steps, int count, hipStream_t stream);
// branch stage of runs [r0, r0 + count): run r is edge rows [r SC_RUN, min(n_edge, (r + 1) SC_RUN)); runs[r - r0] gets its total
hipError_t launch_sc_branch(const ScParams& p, int r0, int count, hipStream_t stream);
// tot += runs[0] + .. + runs[count - 1], one after the other (tot is continued across launches: the order is the run order)
hipError_t launch_sc_total(const ScParams& p, int count, hipStream_t stream);

}  // namespace phm
