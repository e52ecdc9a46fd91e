// phm_loglik_host.h -- host side shared by the entry points that take many rate matrices in one call (DESIGN.md sections 17 to 21
// and 23): the checked input and its validation, the evaluation index, and for 2..8 states (models across the lanes) the chunk
// plan, the staging of models and tips, and LlLanes, the device state of section 17 with its P and tips / up / root launches.
// The planner and the staging functions are pure host code in this header (tests/native/many_models_host_check.cpp runs them
// without a device); everything that makes a HIP call is defined in phm_loglik_host.cpp.  What the two ancestral entry points
// share beyond this is phm_ancestral_host.h.
#pragma once

#include "phm_expect_host.h"
#include "phm_loglik.h"

namespace phm_ll {

constexpr size_t LL_WORK = size_t(256) << 20;          // 5..8 states: Pade matrices of one P launch

// What every device of a call shares.
struct LlInput {
  int n = 0, T = 0, Nn = 0, E = 0, NT = 0, S = 0, K = 0;
  bool per_site = false, paired = false;
  const int32_t* states = nullptr;
  const int32_t* site_of_model = nullptr;
  phm::Schedule sched;
  std::vector<double> Qr;                               // [K][n * n] row-major
  std::vector<double> pid;                              // [K][n] normalised
  std::vector<double> edge_length;
  std::vector<int32_t> obs;
  std::vector<phm::UpStep> up;                          // grouped by height
  std::vector<int32_t> up_off;
  const int32_t* tips_of(int64_t site) const { return states + (per_site ? site * T : 0); }
  int64_t sites_per_model() const { return paired ? 1 : S; }
};

// tree, models, root priors, tips, observe, site_of_model and option checks (no device call); fn prefixes the messages
int32_t ll_validate(const std::string& fn, const phm_tree* x, int32_t n, int32_t K, const double* Q, const double* pid, int32_t n_pid,
                    const int32_t* observe, const int32_t* site_of_model, const phm_options& o, LlInput& in);

// evaluation index of (site, model): cross S x K with the site fastest, paired K
inline int64_t ll_eval_of(const LlInput& in, int64_t site, int64_t model) { return in.paired ? model : site + (int64_t)in.S * model; }

// ---- 2..8 states: the chunk plan (no HIP call: the caller asks for the free memory) ----
struct LlPlan {
  int64_t Kc_max = 0, Sc_max = 0;                       // models (a multiple of 64) and sites of a chunk
  int ne_max = 0;                                       // edges of one launch_ll_expm
};

// edges of one launch_ll_expm for chunks of Kpm models: 5..8 states share LL_WORK of Pade matrices; chunk: expect_chunk
inline int ll_edges_per_launch(int n, int E, size_t Kpm, int chunk) {
  const size_t nn = (size_t)n * n;
  int ne_max = E;
  if (n > phm::LL_REG_MAX) ne_max = (int)std::max<size_t>(1, std::min<size_t>({(size_t)E, (size_t)65535, LL_WORK / (sizeof(double) * 4 * nn * Kpm)}));
  ne_max = std::min(ne_max, 65535);
  if (chunk > 0) ne_max = std::min(ne_max, chunk);
  return ne_max;
}

// Chunks of models [.., count) and of their sites in half of free_b bytes.  Section 17's own footprint is counted here: the Pade
// workspace once, per model Q, pid, P and the error word, per evaluation L, sL, ll and, when paired, a tip byte per tip (P is
// sized from the free memory too: a 10 000-tip tree at 4 states needs 2.56 MB of it per model).  The caller adds what it
// allocates on top: fixed bytes, bytes per model and bytes per evaluation.  When not even 64 models with all their sites fit,
// the sites of a chunk shrink.  chunk: phm_debug_options.expect_chunk.
inline LlPlan ll_plan(size_t free_b, const LlInput& in, int64_t count, int chunk, size_t fixed, size_t per_model, size_t per_eval) {
  const int n = in.n;
  const size_t nn = (size_t)n * n;
  fixed += n > phm::LL_REG_MAX ? LL_WORK : 0;
  per_model += sizeof(double) * ((size_t)in.E * nn + nn + n) + sizeof(uint32_t);
  per_eval += sizeof(double) * ((size_t)in.NT * (n + 1) + 1) + (in.paired ? (size_t)in.T : 0);
  const size_t budget = free_b / 2 > fixed ? free_b / 2 - fixed : 0;
  LlPlan pl;
  pl.Sc_max = std::min<int64_t>(in.sites_per_model(), 65535);
  pl.Kc_max = (int64_t)(budget / (per_model + per_eval * (size_t)pl.Sc_max)) / 64 * 64;
  if (pl.Kc_max < 64) {
    pl.Kc_max = 64;
    const size_t share = budget / 64;                    // per64: what one of the 64 models may take with its sites
    pl.Sc_max = std::max<int64_t>(1, std::min<int64_t>(pl.Sc_max, share > per_model ? (int64_t)((share - per_model) / per_eval) : 1));
  }
  if (chunk > 0) {
    pl.Kc_max = std::min<int64_t>(pl.Kc_max, ((int64_t)chunk + 63) / 64 * 64);
    pl.Sc_max = std::min<int64_t>(pl.Sc_max, chunk);
  }
  pl.Kc_max = std::min<int64_t>(pl.Kc_max, (count + 63) / 64 * 64);
  pl.ne_max = ll_edges_per_launch(n, in.E, (size_t)pl.Kc_max, chunk);
  return pl;
}

// ---- staging (host only) ----
// Kc rows of len values each -> [len][Kp], the model fastest, the lanes Kc .. Kp - 1 zero: Q ([K][n * n]) and pid ([K][n])
inline void ll_stage_rows(const double* src, size_t len, int64_t Kc, int Kp, std::vector<double>& dst) {
  dst.assign(len * (size_t)Kp, 0.0);
  for (int64_t k = 0; k < Kc; ++k)
    for (size_t e = 0; e < len; ++e) dst[e * Kp + k] = src[(size_t)k * len + e];
}

// paired: [tip][Kp], lane k the tips of the site of model m0 + k, the lanes Kc .. Kp - 1 zero
inline void ll_stage_tips_paired(const LlInput& in, int64_t m0, int64_t Kc, int Kp, std::vector<uint8_t>& dst) {
  const int T = in.T;
  dst.assign((size_t)T * Kp, (uint8_t)0);
  for (int64_t k0 = 0; k0 < Kc; k0 += 64) {              // a tile of 64 models at a time: 64 sequential reads, 64-byte writes
    const int kn = (int)std::min<int64_t>(64, Kc - k0);
    const int32_t* y[64];
    for (int k = 0; k < kn; ++k) y[k] = in.tips_of(in.site_of_model[m0 + k0 + k]);
    for (int t = 0; t < T; ++t)
      for (int k = 0; k < kn; ++k) dst[(size_t)t * Kp + k0 + k] = (uint8_t)y[k][t];
  }
}

// cross: [site][tip] of the sites s0 .. s0 + Sc - 1
inline void ll_stage_tips_sites(const LlInput& in, int64_t s0, int64_t Sc, std::vector<uint8_t>& dst) {
  const int T = in.T;
  dst.resize((size_t)T * Sc);
  for (int64_t s = 0; s < Sc; ++s) {
    const int32_t* y = in.tips_of(s0 + s);
    for (int t = 0; t < T; ++t) dst[(size_t)s * T + t] = (uint8_t)y[t];
  }
}

// ---- 2..8 states: section 17's device state for the models [.., ..) of one device ----
// The order of a driver: upload_tree, its own uploads, ll_plan on hipMemGetInfo's free bytes, alloc, then per chunk of models
// load_models (or load_priors and its own Q), params, expm and, per chunk of sites, stage_tips, passes and fetch_ll.  No call
// here is timed: the driver brackets the launches with its KernelTimer, next to its own.
struct LlLanes {
  const LlInput& in;
  LlPlan plan;
  DevBuf dt, dobs, dup, dQ, dpid, dP, dwork, dbad, dL, dsL, dll, dtips;
  std::vector<double> Qh, pidh, llh;                    // llh: [site][Kp] of the last fetch_ll
  std::vector<uint8_t> tips_h;
  int64_t m0 = 0, Kc = 0;                               // the loaded chunk: its first model (global index) and its models
  int Kp = 0;                                           // ... padded to 64

  explicit LlLanes(const LlInput& input) : in(input) {}
  int32_t upload_tree();                                // edge lengths, observe, the up steps
  int32_t alloc(const LlPlan& pl);                      // for chunks of pl.Kc_max models x pl.Sc_max sites
  int32_t load_priors(int64_t first, int64_t count);    // the chunk's pid, a cleared error word per model; sets m0, Kc, Kp
  int32_t load_models(int64_t first, int64_t count);    // load_priors and the chunk's Q
  phm::LlParams params() const;                         // of the loaded chunk, n_sites = 1
  int32_t expm(const phm::LlParams& p) const;           // P_k(t_b) of every edge, plan.ne_max edges a launch
  int32_t stage_tips(int64_t s0, int64_t Sc);           // paired: the chunk's own sites; cross: sites s0 .. s0 + Sc - 1
  int32_t passes(const phm::LlParams& p) const;         // tips, the up levels, root
  int32_t fetch_ll(int64_t Sc);                         // ll of Sc sites x Kp lanes -> llh
};

}  // namespace phm_ll
