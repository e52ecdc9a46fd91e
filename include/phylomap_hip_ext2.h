/*
 * phylomap_hip_ext2.h -- entry points of the C-ABI that were added after phylomap_hip_ext.h and its symbol list were pinned in
 * their turn (tests/test_sample_wide_cpu.py holds that header and phylomap_amd/_lib.py's EXT_EXPORTS to one name).  An entry
 * point added since then is declared here and bound through _lib.EXT2_EXPORTS; when the records are regenerated the three
 * headers become one.  The types, the status codes, phm_last_error and PHM_VERSION are phylomap_hip.h's.
 */
#ifndef PHYLOMAP_HIP_EXT2_H
#define PHYLOMAP_HIP_EXT2_H

#include "phylomap_hip_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- posterior sample of the rates of an index model at 9..64 states ----
 * phm_gibbs_rates' arguments, argument for argument, with the same meaning for 9 <= n_states <= 64 (amino acids, codons,
 * hidden-rate index models): C = n_chains chains in lock-step; iteration i of chain k draws one exact history per site given the
 * tips and Q(theta_k) -- phm_sample_histories_models_wide's draw with draws = 1 and replica_offset + i, addressed by the global
 * evaluation site * n_chains + chain -- and then every rate from its Gamma full conditional.
 *   index:  n x n column-major, entry (i, j) the 1-based parameter of q_ij, 0 a structural zero; the diagonal is ignored.
 *   prior:  Gamma (shape, rate) per parameter, [n_prior][n_params][2], n_prior 1 (shared) or n_chains.
 *   theta0: [n_chains][n_params] starts in (0, theta_max].  theta_max: every rate is confined to (0, theta_max].
 *   site_of_chain NULL (joint): every chain sees all S = n_replicas sites; else (paired) chain k sees site site_of_chain[k] alone.
 *   theta [rows][C][p], loglik [rows][C], stats [rows][C][n + n(n-1)] (NULL: not wanted), rows = ceil(iters / thin): row r is
 *   iteration r * thin; row 0 holds the starts.  rejected [C][p], chain_status [C].
 * The update differs from phm_gibbs_rates' in the order of its sums, and in nothing else.  T is the chain's statistics row SUMMED
 * over its sites on the device: for each of the n + n(n-1) columns, and for the log-likelihood, the per-site doubles added one
 * after the other, sites ascending (the values stats and loglik return).  One pass over the off-diagonal entries (i, j) in
 * row-major order: for c = index(i, j) >= 1, N_c += T[n + i (n-1) + (j > i ? j-1 : j)] and W_c += T[i].  Then for c ascending
 * theta_c <- Gamma(shape_c + N_c, scale 1 / (rate_c + W_c)) from the stream (seed, ENT_RATE | c, chain, i + replica_offset); a
 * draw above theta_max, or not > 0, is rejected and counted, and the old value stays.  theta of row r + 1 is therefore a function
 * of row r's stats.
 * Refusals, every one before any device call: phm_gibbs_rates' (index gaps, priors, theta0, iters, thin, sites) and
 * phm_loglik_models' on Q(theta0), under this entry point's name; n_states outside 2..64 is PHM_ERR_BAD_INPUT; 2..8 states is
 * PHM_ERR_UNSUPPORTED naming phm_gibbs_rates; (most rates in a row) * theta_max * (longest branch) above 32768 is
 * PHM_ERR_UNSUPPORTED naming theta_max.  On the device: a chain's table of (M + 1) * n * n doubles (M the stopping index of the
 * jump-count series at that bound) that does not fit the budget is PHM_ERR_CAPACITY with the bytes; all sites of a chain stay
 * resident, and one chain whose sites do not fit is PHM_ERR_OOM.
 * A chain whose summed log-likelihood is not finite, or whose Pade denominator met a zero pivot, gets chain_status 1 and NaN rows
 * from that iteration on; the other chains go on.  n_devices / devices[] shard the chains and phm_debug_options.expect_chunk
 * caps the chunks of chains; neither changes an output bit.  phm_last_kernel_ms: device time of the whole call;
 * phm_debug_options.q_timing prints the per-iteration split to stderr. */
int32_t phm_gibbs_rates_wide(const phm_tree* x, int32_t n_states, const int32_t* index, int32_t n_params, int32_t n_chains,
                             const double* theta0, const double* prior, int32_t n_prior, double theta_max, const double* pid,
                             int32_t n_pid, const int32_t* observe, const int32_t* site_of_chain, int32_t iters, int32_t thin,
                             const phm_options* opt, double* theta, double* loglik, double* stats, int32_t* rejected,
                             int32_t* chain_status);

#ifdef __cplusplus
}
#endif

#endif
