/*
 * phylomap_hip_ext.h -- entry points of the C-ABI that were added after the symbol list of phylomap_hip.h was recorded.
 *
 * phylomap_hip.h and the list of its symbols are pinned, name for name, by recorded calls of an earlier state of the library
 * (tests/golden/api_calls).  An entry point added since then is declared here and bound through phylomap_amd/_lib.py's
 * EXT_EXPORTS until that record is regenerated; then this header's content moves into phylomap_hip.h.
 * The types, the status codes, phm_last_error and PHM_VERSION are phylomap_hip.h's.
 */
#ifndef PHYLOMAP_HIP_EXT_H
#define PHYLOMAP_HIP_EXT_H

#include "phylomap_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- exact sampler of histories over many rate matrices and sites at 9..64 states ----
 * phm_sample_histories_models' arguments, argument for argument, with the same meaning for 9 <= n_states <= 64 (amino acids,
 * codons, hidden-rate models): D = draws independent histories per evaluation (model k, site s), each an exact draw from
 * p(history | tips_s, Q_k, pid_k).  An evaluation's index e is its index into loglik; history h = e * draws + d;
 * H = evaluations * draws.
 *   loglik: phm_loglik_models' values bit for bit.
 *   stats:  H x (n + n(n-1)), column-major with the history fastest, phm_expected_stats' column order.
 *   nodes:  NULL, or H x (n_tips + n_node) history-major: the 1-based TRUE state of every node by ape node id, tips included.
 *   map_off NULL: no maps.  Otherwise the two-phase contract of phm_simulate_histories_maps with R = H: a sizing call (map_dwell
 *           and map_state NULL) writes the H * n_edge + 1 offsets, a filling call reads them; row h * n_edge + b.
 * The draws are section 19's, number for number: the same random-number addresses (phm_options.seed; replica_offset is added to
 * the draw index d; the global evaluation site * n_models + model), the same categorical rule, jump-count series, jump times and
 * 64-bit fixed-point dwell sums; P_k(t_b) is phm_expected_stats' (Pade(6) with its squaring counts).
 * Refusals, every one before any device call: what phm_loglik_models refuses (n_states outside 2..64 is PHM_ERR_BAD_INPUT);
 * draws < 1; 2..8 states is PHM_ERR_UNSUPPORTED naming phm_sample_histories_models; max(-q_ii) * t_b above 32768 for any model is
 * PHM_ERR_UNSUPPORTED naming the model; the map arguments as phm_simulate_histories_maps checks them.  A model whose table of
 * (M + 1) * n * n doubles (M the stopping index of the jump-count series at max(-q_ii) * max_b t_b) does not fit the device's
 * budget is PHM_ERR_CAPACITY naming the model and the bytes, before any sampling launch.
 * An evaluation whose log-likelihood is -inf, or whose model's Pade denominator met a zero pivot, is not drawn: loglik = -inf,
 * NaN rows of stats, zeros in nodes, empty map rows; it does not fail the call.  n_devices / devices[] shard the models and
 * phm_debug_options.expect_chunk caps the chunks of models, sites, level steps and tiles; neither changes an output bit.
 * phm_last_kernel_ms: device time of the whole call. */
int32_t phm_sample_histories_models_wide(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                         int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, int32_t draws,
                                         const phm_options* opt, double* stats, double* loglik, int32_t* nodes,
                                         int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state);

#ifdef __cplusplus
}
#endif

#endif
