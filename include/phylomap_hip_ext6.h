/*
 * phylomap_hip_ext6.h -- entry points of the C-ABI that were added after phylomap_hip_ext5.h and its symbol list were pinned in
 * their turn (tests/test_time_models_cpu.py holds that header and phylomap_amd/_lib.py's EXT5_EXPORTS to one name).  An entry
 * point added since then is declared here and bound through _lib.EXT6_EXPORTS; when the records are regenerated the seven
 * headers become one.  The types, the status codes, phm_last_error and PHM_VERSION are phylomap_hip.h's.
 */
#ifndef PHYLOMAP_HIP_EXT6_H
#define PHYLOMAP_HIP_EXT6_H

#include "phylomap_hip_ext5.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- exact expectations THROUGH TIME for many rate matrices at 9..64 states, batched over the models ----
 * What the entry point of phylomap_hip_ext5.h returns, with one state per lane and the models, the sites and the items of the
 * plan batched: no loop over the models, no n x n matrix per (model, item), one plan of depths, crossings and sub-branches for
 * every model and device.  The arguments are that entry point's eighteen, one for one, with n_labels and labels inserted after
 * bounds; the outputs, the evaluation order (cross and paired), the NULL rules and the values per evaluation are section 28's.
 *   labels      NULL, or [n_labels][n][n] weight matrices, each laid out as Q is, as phm_expected_branch_stats_models takes
 *               them: entry (i, i) weighs E[dwell_i], entry (i, j) E[N_ij]
 *   bin_stats   labels NULL: [n + n(n-1)][n_bounds - 1][evaluations]; with labels: [n_labels][n_bounds - 1][evaluations], each
 *               value the plain double sum acc = acc + w[col] * row[col] over the columns of the bin's full row, bit for bit
 * The along-branch vectors are section 28's uniformization sums (no Pade matrix per item), so the values agree with
 * phm_expected_through_time's within its bars and not bit for bit: the entry point of ext5 keeps serving 9..64 states model by
 * model for the callers that hold recorded values.  The ends of a branch reuse the stored P_k(t_b): a point at s = 0 or s = t_b
 * repeats the sums of the node there.  One bin over the whole depth is phm_expected_stats_models_wide's totals bit for bit on a
 * tree of at most 16 edge rows (the totals add runs of 16 edge rows).  loglik is phm_loglik_models' value bit for bit.  An
 * impossible evaluation (loglik -inf) gets NaN in all of its rows and does not fail the call; a structurally zero q_ij gives 0
 * exactly; a model with max(-q_ii) = 0 is served (pi constant along a branch, the dwell of a sub-branch its length on the
 * posterior state).
 * Refusals, every one before any device call: x, Q or pid NULL and every output NULL are PHM_ERR_BAD_INPUT; n_states outside
 * 9..64 is PHM_ERR_UNSUPPORTED; then phm_loglik_models' (ll_validate) under this entry point's name, sites * models above 31
 * bits, phm_expected_through_time's checks of the counts, labels without bin_stats, n_labels < 1 or above 65 535 with labels
 * given, a non-finite weight (the label is named), the checks of bounds and of the points with the 0-based index named are
 * PHM_ERR_BAD_INPUT; max(-q_ii) * t_b above 1e6 for any model and edge is PHM_ERR_UNSUPPORTED naming both.
 * n_devices / devices[] shard the models; phm_debug_options.expect_chunk caps the chunks of models, sites and items per launch;
 * neither changes an output bit.  phm_last_kernel_ms: device time of the whole call; phase_timing = 1 prints its phases. */
int32_t phm_expected_through_time_models_wide(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                              int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const phm_options* opt,
                                              int32_t n_bounds, const double* bounds, int32_t n_labels, const double* labels,
                                              double* occupancy, double* bin_stats, int64_t n_points, const int32_t* point_edge,
                                              const double* point_pos, double* point_post, double* loglik);

#ifdef __cplusplus
}
#endif

#endif
