// phm_sim_host.h -- the host front end the two forward simulators share (phm_sim_api.cpp, phm_sim_models_api.cpp; DESIGN.md sections
// 12 and 22): argument checks, a model's tables, root priors, state maps, the capacity refusal and the way a chunk's results go
// home.  `fn` is the entry point's name with ": " for its messages.
#pragma once

#include "phm_internal.h"
#include "phm_sim.h"

namespace phm_sim {

// the pointers no call may leave NULL and the state count; `may_be_null`: the message's list of those that may
inline int32_t check_head(const std::string& fn, const char* may_be_null, const phm_tree* x, int32_t n, const double* Q,
                          const double* pid, const int32_t* tips, const double* stats) {
  if (!x || !Q || !pid || !tips || !stats) return fail(PHM_ERR_BAD_INPUT, fn + "NULL argument (" + may_be_null + ")");
  if (n < 2 || n > phm::SIM_MAX_STATES) return fail(PHM_ERR_BAD_INPUT, fn + "n_states must be in 2..64");
  return PHM_OK;
}

// the tree: its schedule and its checked branch lengths
inline int32_t check_tree(const std::string& fn, const phm_tree* x, phm::Schedule& sched, std::vector<double>& edge_length) {
  if (!x->edge || !x->edge_length) return fail(PHM_ERR_BAD_INPUT, fn + "x$edge and x$edge.length are required");
  std::string serr;
  if (!phm::build_schedule(x->n_tips, x->n_node, x->n_edge, x->edge, sched, serr)) return fail(PHM_ERR_BAD_INPUT, "tree: " + serr);
  const int32_t st = check_edge_lengths(x);
  if (st) return st;
  edge_length.assign(x->edge_length, x->edge_length + x->n_edge);
  return PHM_OK;
}

// One model's tables out of its column-major generator: qoff [n n] jump weights, row-major (from, to), diagonal zeroed; qtot [n] their
// row totals, summed left to right; inv_rate [n] IEEE 1 / (-q_ss), 0 for an absorbing state.  `who` ("" or "model k: ") opens a refusal.
inline int32_t model_tables(const double* Q, int n, const std::string& who, double* qoff, double* qtot, double* inv_rate) {
  std::vector<double> qr;
  const int32_t st = check_generator(Q, n, qr);
  if (st) return fail(st, who + g_phm_err);
  for (int i = 0; i < n; ++i) {
    double* row = &qr[(size_t)i * n];
    const double qii = row[i];
    row[i] = 0.0;
    double off = row[0];
    for (int j = 1; j < n; ++j) off += row[j];
    if (qii < 0.0 && !(off > 0.0)) return fail(PHM_ERR_BAD_INPUT, who + "Q: row " + std::to_string(i + 1) + " leaves its state but has no target");
    qtot[i] = off;
    inv_rate[i] = qii < 0.0 ? 1.0 / (-qii) : 0.0;
  }
  std::copy(qr.begin(), qr.end(), qoff);
  return PHM_OK;
}

// n_pid root priors of n entries, kept as given, and their totals summed left to right; `name_column`: a refusal names its prior
inline int32_t root_priors(const double* pid, int n_pid, int n, bool name_column, std::vector<double>& kept, std::vector<double>& ptot) {
  kept.assign(pid, pid + (size_t)n_pid * n);
  ptot.resize(n_pid);
  for (int k = 0; k < n_pid; ++k) {
    double psum = 0.0;
    const int32_t st = check_root_prior(pid + (size_t)k * n, n, psum);
    if (st) return name_column ? fail(st, "pid column " + std::to_string(k) + ": " + g_phm_err) : st;
    double tot = pid[(size_t)k * n];
    for (int j = 1; j < n; ++j) tot += pid[(size_t)k * n + j];
    ptot[k] = tot;
  }
  return PHM_OK;
}

// 0-based true state -> reported 1-based state: n entries for the tips (through `observe`), then n for the nodes (the identity)
inline int32_t state_maps(const int32_t* observe, int n, std::vector<int32_t>& map) {
  const int32_t st = check_observe(observe, n, map);
  if (st) return st;
  for (int i = 0; i < n; ++i) map.push_back(i + 1);
  return PHM_OK;
}

// the refusal of a branch past SIM_MAX_JUMPS; `who`: "" or "model k: "
inline int32_t capacity_refusal(const std::string& who, uint64_t edge_row) {
  return fail(PHM_ERR_CAPACITY, who + "more than " + std::to_string(phm::SIM_MAX_JUMPS) + " jumps on edge row " + std::to_string(edge_row + 1) +
                                    " (samplethebranch stops there, R/sourceme.R:356)");
}

// `count` histories go home to rows first .. of the caller's matrices: the statistics [col][pad] into the column-major ld_stats x
// cols matrix, the state bytes through the transposing epilogue (`dmap`: state_maps' table, `dtr`: count x rows int32 of scratch).
inline int32_t send_home(const double* dstats, const uint8_t* dnstate, const int32_t* dmap, int32_t* dtr, int n, int T, int rows,
                         int pad, int64_t first, int64_t count, double* stats, int64_t ld_stats, int32_t* tips, int32_t* nodes) {
  const int cols = n + n * n + 1;
  HIPCHK(hipMemcpy2D(stats + first, sizeof(double) * (size_t)ld_stats, dstats, sizeof(double) * (size_t)pad, sizeof(double) * (size_t)count,
                     cols, hipMemcpyDeviceToHost));
  HIPCHK(phm::launch_sim_transpose(dnstate, T, (int)count, pad, dmap, dtr, nullptr));
  HIPCHK(hipMemcpy(tips + first * T, dtr, sizeof(int32_t) * (size_t)count * T, hipMemcpyDeviceToHost));
  if (nodes) {
    HIPCHK(phm::launch_sim_transpose(dnstate, rows, (int)count, pad, dmap + n, dtr, nullptr));
    HIPCHK(hipMemcpy(nodes + first * rows, dtr, sizeof(int32_t) * (size_t)count * rows, hipMemcpyDeviceToHost));
  }
  return PHM_OK;
}

}  // namespace phm_sim
