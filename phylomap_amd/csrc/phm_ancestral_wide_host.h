// phm_ancestral_wide_host.h -- the host core of the entry points that run the tree passes at 9..64 states:
// phm_ancestral_models_wide (phm_ancestral_wide_api.cpp) and phm_sample_histories_models_wide (phm_sample_wide_api.cpp).  The
// chunk plan by free HBM and AwLanes, section 23's device state with its P launches and its tips / up / root launches: what
// LlLanes (phm_loglik_host.h) is for 2..8 states.  The plan is pure host code in this header (tests/native/sample_host_check.cpp
// runs it without a device); everything that makes a HIP call is defined in phm_ancestral_wide_host.cpp.
#pragma once

#include "phm_ancestral_wide.h"
#include "phm_loglik_host.h"

namespace phm_ll {

struct AwPlan {
  int64_t Kc_max = 0, Sc_max = 0;                       // models and sites of a chunk
  int step_max = 0;                                     // level steps (and selected rows) of one launch
  size_t budget = 0, per_model = 0, per_eval = 0;       // the bytes the chunks may take, and what a model and an evaluation take
};

// Chunks of models [.., count) and of their sites in half of free_b bytes.  Section 23's own footprint is counted here: once the
// Pade workspace of one model (the models' launches follow each other on the stream); per model Q, pid, the squaring counts, the
// error word, P and, when paired, its tips; per evaluation L, sL and ll.  The caller adds what it allocates on top.  When not even
// one model with all its sites fits, the sites of a chunk shrink, down to one.  chunk: phm_debug_options.expect_chunk.
inline AwPlan aw_plan(size_t free_b, const LlInput& in, int64_t count, int chunk, size_t fixed, size_t per_model, size_t per_eval) {
  const int n = in.n, NP = phm::aw_lanes(n);
  const size_t nn = (size_t)n * n, E = (size_t)in.E;
  AwPlan pl;
  fixed += sizeof(double) * 5 * nn * E;
  pl.budget = free_b / 2 > fixed ? free_b / 2 - fixed : 0;
  pl.per_model = per_model + sizeof(double) * (E * nn + nn + n) + sizeof(int32_t) * E + sizeof(uint32_t) + (in.paired ? (size_t)in.T : 0);
  pl.per_eval = per_eval + (sizeof(double) * NP + sizeof(int32_t)) * (size_t)in.NT + sizeof(double);
  pl.Sc_max = std::min<int64_t>(in.sites_per_model(), phm::AW_GRID_MAX);
  pl.Kc_max = (int64_t)(pl.budget / (pl.per_model + pl.per_eval * (size_t)pl.Sc_max));
  if (pl.Kc_max < 1) {
    pl.Kc_max = 1;
    pl.Sc_max = std::max<int64_t>(1, std::min<int64_t>(pl.Sc_max, pl.budget > pl.per_model ? (int64_t)((pl.budget - pl.per_model) / pl.per_eval) : 1));
  }
  pl.step_max = phm::AW_GRID_MAX;
  if (chunk > 0) {
    pl.Kc_max = std::min<int64_t>(pl.Kc_max, chunk);
    pl.Sc_max = std::min<int64_t>(pl.Sc_max, chunk);
    pl.step_max = std::min(pl.step_max, chunk);
  }
  pl.Kc_max = std::min<int64_t>({pl.Kc_max, count, (int64_t)phm::AW_GRID_MAX});
  return pl;
}

// The level steps [off[l], off[l + 1]) of every level l, at most step_max of them a launch: launch(k0, count) -> hipError_t
template <class F>
inline int32_t aw_level_steps(const std::vector<int32_t>& off, int step_max, F&& launch) {
  for (size_t l = 0; l + 1 < off.size(); ++l)
    for (int k0 = off[l]; k0 < off[l + 1]; k0 += step_max) HIPCHK(launch(k0, std::min(step_max, off[l + 1] - k0)));
  return PHM_OK;
}

// Section 23's device state for the models [.., ..) of one device.  The order of a driver: upload_tree, its own uploads, aw_plan
// on hipMemGetInfo's free bytes, alloc, then per chunk of models load_models, expm, fetch_bad and params, and per chunk of sites
// stage_tips, passes and fetch_ll.  No call here is timed: the driver brackets the launches with its KernelTimer, next to its own.
struct AwLanes {
  const LlInput& in;
  AwPlan plan;
  DevBuf dt, dobs, dup, dQ, dpid, dsq, dP, dwork, dbad, dL, dsL, dll, dtips;
  std::vector<double> llh;                              // [model][site] of the last fetch_ll
  std::vector<uint8_t> tips_h;
  std::vector<int32_t> sqh;
  std::vector<uint32_t> badh;                           // [model] of the last fetch_bad: not 0 when the model's Pade met a zero pivot
  int64_t m0 = 0, Kc = 0;                               // the loaded chunk: its first model (global index) and its models

  explicit AwLanes(const LlInput& input) : in(input) {}
  int32_t upload_tree();                                // edge lengths, observe, the up steps
  int32_t alloc(const AwPlan& pl);                      // for chunks of pl.Kc_max models x pl.Sc_max sites
  int32_t load_models(int64_t first, int64_t count);    // the chunk's Q, pid and squaring counts, cleared error words; sets m0, Kc
  // the loaded chunk's matrices replaced in place (phm_gibbs_rates_wide: Q(theta) of an iteration): Q [Kc][n * n] row-major and
  // their squaring counts sq [Kc][E] (ex_squarings'), cleared error words; no buffer is reallocated
  int32_t set_models(const double* Q, const int32_t* sq);
  int32_t expm() const;                                 // P_k(t_b) of every edge: one launch_expm_pade per model
  int32_t fetch_bad();                                  // the models' error words -> badh
  phm::AwParams params() const;                         // of the loaded chunk, what every driver sets; Sc is the driver's
  int32_t stage_tips(int64_t s0, int64_t Sc);           // paired: [model][tip] of the chunk's own sites; cross: [site][tip]
  int32_t passes(const phm::AwParams& p) const;         // tips, the up levels in steps of plan.step_max, root
  int32_t fetch_ll(int64_t Sc);                         // ll of Kc models x Sc sites -> llh
  // after fetch_bad and fetch_ll: model k of the chunk has its P and the evaluation at llh[at] a finite log-likelihood
  bool possible(int64_t k, size_t at) const { return !badh[k] && std::isfinite(llh[at]); }
};

}  // namespace phm_ll
