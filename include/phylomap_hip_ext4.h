/*
 * phylomap_hip_ext4.h -- entry points of the C-ABI that were added after phylomap_hip_ext3.h and its symbol list were pinned in
 * their turn (tests/test_scores_wide_cpu.py holds that header and phylomap_amd/_lib.py's EXT3_EXPORTS to one name).  An entry
 * point added since then is declared here and bound through _lib.EXT4_EXPORTS; when the records are regenerated the five
 * headers become one.  The types, the status codes, phm_last_error and PHM_VERSION are phylomap_hip.h's.
 */
#ifndef PHYLOMAP_HIP_EXT4_H
#define PHYLOMAP_HIP_EXT4_H

#include "phylomap_hip_ext3.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- exact expectations PER BRANCH for many rate matrices, 2..64 states ----
 * E[dwell_i | tips_s, Q_k] and E[N_ij | tips_s, Q_k] on each selected branch: where on the tree the changes happened, under K
 * rate matrices in one call.  The first nine arguments are phm_expected_stats_models', one for one, with the same meaning, cross
 * and paired evaluation order and NULL rules.
 *   edges   n_edges 0-based edge rows in any order, repeats allowed; the output follows the list.  NULL: every edge row in row
 *           order (n_edges is ignored).  n_sel below is the length of the list.
 *   labels  NULL: full rows.  Else [n_labels][n][n], each matrix laid out as Q is (column-major): entry (i, i) weighs
 *           E[dwell_i], entry (i, j) weighs E[N_ij] (labelled transitions in the sense of Minin & Suchard).
 *   branch  [C][n_sel][evaluations], column slowest, evaluation fastest.  Full rows: C = n + n(n-1) in phm_expected_stats' column
 *           order.  Labels: C = n_labels.
 *   loglik  [evaluations], or NULL; phm_loglik_models' value bit for bit.
 * A full row is exactly the per-edge value that phm_expected_stats_models and phm_expected_stats_models_wide, at 2..8 and 9..64
 * states, add into their run totals: adding the rows of edge rows 16 r .. 16 r + 15 in order from 0.0, then those sums in order
 * from 0.0, gives their totals bit for bit.  A labelled value is acc = 0.0; for col = 0 .. C - 1: acc = acc + w[col] * row[col],
 * the product and the sum rounded separately (no fma), so plain double arithmetic reproduces it from the full row bit for bit.
 * An impossible evaluation (loglik -inf) gets NaN in all of its rows and does not fail the call.  A structurally zero q_ij gives 0
 * exactly, a zero-length branch a row of exact zeros.  A model with max(-q_ii) = 0 is served at every state count: dwell = t_b on
 * the posterior state, counts exactly 0.
 * Refusals, every one before any device call: phm_loglik_models' (ll_validate) under this entry point's name; n_states outside
 * 2..64, an edge row outside [0, n_edge) (the position is named), n_edges < 1 with edges given, n_labels < 1 or above 65535 with
 * labels given, a non-finite label weight and branch == NULL are PHM_ERR_BAD_INPUT; max(-q_ii) * t_b above 1e6 for any model and
 * SELECTED edge is PHM_ERR_UNSUPPORTED naming both.
 * n_devices / devices[] shard the models; phm_debug_options.expect_chunk caps the chunks of models, sites, level steps and
 * selected edges per branch launch; neither changes an output bit.  phm_last_kernel_ms: device time of the whole call. */
int32_t phm_expected_branch_stats_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                         int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const phm_options* opt,
                                         int32_t n_edges, const int32_t* edges, int32_t n_labels, const double* labels,
                                         double* branch, double* loglik);

#ifdef __cplusplus
}
#endif

#endif
