/*
 * phylomap_hip_ext3.h -- entry points of the C-ABI that were added after phylomap_hip_ext2.h and its symbol list were pinned in
 * their turn (tests/test_gibbs_wide_cpu.py holds that header and phylomap_amd/_lib.py's EXT2_EXPORTS to one name).  An entry
 * point added since then is declared here and bound through _lib.EXT3_EXPORTS; when the records are regenerated the four
 * headers become one.  The types, the status codes, phm_last_error and PHM_VERSION are phylomap_hip.h's.
 */
#ifndef PHYLOMAP_HIP_EXT3_H
#define PHYLOMAP_HIP_EXT3_H

#include "phylomap_hip_ext2.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- exact expectations and log-likelihoods for many rate matrices at 9..64 states ----
 * phm_expected_stats_models' arguments, argument for argument, with the same meaning, output layout and NULL rules for
 * 9 <= n_states <= 64 (amino acids, codons, hidden-rate models), batched over models and sites with one state per lane:
 *   stats  [n + n(n-1)][evaluations] column slowest, E[dwell_i] then E[N_ij] in phm_expected_stats' column order;
 *   loglik [evaluations]; an evaluation is (site, model), the site fastest (cross: S x K), or the model (paired: K).
 * One extension: stats == NULL asks for the log-likelihoods alone -- the matrix exponentials and the up pass, no down pass and no
 * branch stage.  loglik is phm_loglik_models' value bit for bit either way.
 * Refusals, every one before any device call: phm_loglik_models' (ll_validate) under this entry point's name; n_states outside
 * 2..64 is PHM_ERR_BAD_INPUT; 2..8 states is PHM_ERR_UNSUPPORTED naming phm_expected_stats_models; with stats not NULL,
 * max(-q_ii) * t_b above 1e6 for any model and branch is PHM_ERR_UNSUPPORTED naming the model and the edge row.
 * An impossible evaluation, or a model whose Pade denominator met a zero pivot, gets loglik = -inf and a row of NaN and does not
 * fail the call.  A structurally zero q_ij gives E[N_ij] = 0 exactly.  A model with max(-q_ii) = 0 is served: dwell = t_b on the
 * posterior state, counts exactly 0.  n_devices / devices[] shard the models and phm_debug_options.expect_chunk caps the chunks
 * of models, sites, level steps and runs of branches; neither changes an output bit.  phm_last_kernel_ms: device time of the
 * whole call. */
int32_t phm_expected_stats_models_wide(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                       int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const phm_options* opt,
                                       double* stats, double* loglik);

#ifdef __cplusplus
}
#endif

#endif
