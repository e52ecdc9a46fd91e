/*
 * phylomap_hip_ext5.h -- entry points of the C-ABI that were added after phylomap_hip_ext4.h and its symbol list were pinned in
 * their turn (tests/test_branch_rows_cpu.py holds that header and phylomap_amd/_lib.py's EXT4_EXPORTS to one name).  An entry
 * point added since then is declared here and bound through _lib.EXT5_EXPORTS; when the records are regenerated the six
 * headers become one.  The types, the status codes, phm_last_error and PHM_VERSION are phylomap_hip.h's.
 */
#ifndef PHYLOMAP_HIP_EXT5_H
#define PHYLOMAP_HIP_EXT5_H

#include "phylomap_hip_ext4.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- exact expectations THROUGH TIME for many rate matrices, 2..64 states ----
 * Section 16's phm_expected_through_time under K rate matrices in one call: the state posterior at points inside branches, the
 * expected lineages in each state at depth boundaries, and E[dwell_i], E[N_ij] per depth bin -- when the changes happened, under
 * the models of a fit and its uncertainty or of a posterior sample of Q.  The first nine arguments are
 * phm_expected_stats_models', one for one, with the same meaning, cross and paired evaluation order and NULL rules; n_bounds,
 * bounds, n_points, point_edge and point_pos are phm_expected_through_time's, with its rules and its checks.
 *   occupancy   [n][n_bounds][evaluations], or NULL (needs n_bounds >= 1)
 *   bin_stats   [n + n(n-1)][n_bounds - 1][evaluations] in phm_expected_stats' column order, or NULL (needs n_bounds >= 2)
 *   point_post  [n][n_points][evaluations], or NULL (needs n_points >= 1)
 *   loglik      [evaluations], or NULL; phm_loglik_models' value bit for bit
 * Column slowest, evaluation fastest, as phm_expected_branch_stats_models lays its rows out.  At least one output is not NULL.
 * Per evaluation (model k, site s) the values are section 16's: depths from the root, a branch counts at tau when
 * d_p < tau <= d_c (tau = 0 counts the root; a zero-length branch never counts), a bin takes the part of each branch inside it,
 * pi_b(s) = a (.) beta / sum(a (.) beta) with a = P_k(s)^T F_b and beta = P_k(t_b - s) L_c.  A point at s = 0 or s = t_b repeats
 * the sums of the node there.  The sums over crossing branches and over sub-branches run in edge-row order.
 * An impossible evaluation (loglik -inf) gets NaN in all of its rows and does not fail the call.  A structurally zero q_ij gives
 * 0 exactly.  A model with max(-q_ii) = 0 is served at 2..8 states: pi is constant along a branch and the dwell of a sub-branch
 * is its length on the posterior state.
 * 2..8 states: the models across the lanes, one plan of depths, crossings and sub-branches for every model.  9..64 states: the
 * call is accepted and served one model after another through phm_expected_through_time itself, so each model's values are that
 * entry point's bit for bit and its limits hold (a model that leaves no state is refused there); the state-per-lane form batched
 * over the models is phm_expected_through_time_models_wide of phylomap_hip_ext6.h.
 * Refusals, every one before any device call: phm_loglik_models' (ll_validate) under this entry point's name; x, Q or pid NULL,
 * every output NULL, n_states outside 2..64, and phm_expected_through_time's checks of the counts, of bounds (finite, >= 0,
 * strictly increasing; the 0-based index is named) and of the points (edge row in 0..n_edge-1, position in [0, t_b]; the 0-based
 * point is named) are PHM_ERR_BAD_INPUT; max(-q_ii) * t_b above 1e6 for any model and edge is PHM_ERR_UNSUPPORTED naming both.
 * n_devices / devices[] shard the models; phm_debug_options.expect_chunk caps the chunks of models, sites and items per launch;
 * neither changes an output bit.  phm_last_kernel_ms: device time of the whole call; phase_timing = 1 prints its phases. */
int32_t phm_expected_through_time_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                         int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const phm_options* opt,
                                         int32_t n_bounds, const double* bounds, double* occupancy, double* bin_stats,
                                         int64_t n_points, const int32_t* point_edge, const double* point_pos, double* point_post,
                                         double* loglik);

#ifdef __cplusplus
}
#endif

#endif
