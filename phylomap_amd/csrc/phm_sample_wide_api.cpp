// phm_sample_wide_api.cpp -- C-ABI of the exact sampler of histories over many rate matrices and sites at 9..64 states
// (phm_sample_histories_models_wide): phm_sample_histories_models' arguments, validation and outputs
// (sm_entry of phm_sample_host.h).  Per device and per chunk of models P_k(t_b) by one launch_expm_pade per model and the table of
// mu_k, B_k and beta (a workgroup per model); per chunk of sites section 23's tips / up / root launches (AwLanes of
// phm_ancestral_wide_host.h, section 23a); and per batch of tiles (SmTiles of phm_sample_host.h, section 19b) the root,
// node-level, branch and finish launches of phm_sample_wide.hip, which read P, L and pid in place.  Every draw is addressed by
// its global evaluation and draw index and evaluations are independent, so neither chunks nor shards change an output bit.
#include "phm_ancestral_wide_host.h"
#include "phm_sample_host.h"
#include "phm_sample_wide.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;

const char* const SW_NAME = "phm_sample_histories_models_wide";

// models [first, first + count) on one device
int32_t sw_device(const SmInput& sm, int32_t device, int64_t first, int64_t count, double* stats, double* loglik,
                  phm_maps::Host* mh, size_t si) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = sm.ll;
  const int n = in.n, E = in.E;
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.sites_per_model();
  const double ninf = -std::numeric_limits<double>::infinity();
  KernelTimer tm;
  double t_pade = 0.0, t_table = 0.0, t_pass = 0.0;   // device time of the phases (sampling and map offsets: SmTiles')
  AwLanes ln(in);
  SmTiles tl(sm, SW_NAME, stats, mh, si);
  st = ln.upload_tree();
  if (st) return st;
  st = tl.setup(first, count);
  if (st) return st;

  int depth_max = 0;
  int64_t k_deep = first;
  for (int64_t k = first; k < first + count; ++k)
    if (sm.depth[k] > depth_max) { depth_max = sm.depth[k]; k_deep = k; }
  const size_t tab_stride = phm::sw_table_doubles(n, depth_max), tab_b = sizeof(double) * tab_stride;

  // On top of section 23's footprint.  Once: a share of an eighth for the tiles (up to n + n (n - 1) columns of accumulators and
  // output per history: 3.3 MB a tile at 64 states).  Per model: mu, B, the depth and the table.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  phm::SwParams sp = {};
  st = tl.alloc(free_b, count, phm::SW_ITEMS_MAX / E, sp.core);
  if (st) return st;
  const AwPlan pl = aw_plan(free_b, in, count, g_phm_debug.expect_chunk, tl.batch_b, sizeof(double) * (nn + 1) + sizeof(int32_t) + tab_b, 0);
  if (pl.budget < pl.per_model + pl.per_eval)            // before anything of the plan is used: not one evaluation fits
    return fail(PHM_ERR_CAPACITY, tl.fn + "model " + std::to_string(k_deep) + ": its table of " + std::to_string(tab_b) + " bytes (" +
                                      std::to_string(depth_max + 1) + " rows of " + std::to_string(nn) + " doubles) does not fit in the " +
                                      std::to_string(pl.budget) + " bytes of HBM this call may use");

  SwModels md;
  st = ln.alloc(pl);
  if (st) return st;
  st = md.alloc(n, (size_t)pl.Kc_max, tab_stride);
  if (st) return st;
  md.fill(sp, ln);
  const SmTiles::Launch launch = [&]() { return phm::launch_sw_sample(sp, sm.level_off, tl.maps_mode(), nullptr); };

  for (int64_t c0 = 0; c0 < count; c0 += pl.Kc_max) {
    const int64_t Kc = std::min<int64_t>(pl.Kc_max, count - c0);
    const int64_t m0 = first + c0;                       // global index of this chunk's first model
    st = ln.load_models(m0, Kc);
    if (st) return st;
    HIPCHK(hipMemcpy(md.ddepth.p, sm.depth.data() + m0, sizeof(int32_t) * Kc, hipMemcpyHostToDevice));
    sp.Kc = (int)Kc;
    HIPCHK(tm.start());
    st = ln.expm();
    if (st) return st;
    HIPCHK(tm.stop());
    st = ln.fetch_bad();
    if (st) return st;
    HIPCHK(tm.add_to(t_pade));
    HIPCHK(tm.start());
    HIPCHK(phm::launch_sw_table(sp, nullptr));
    HIPCHK(tm.stop());
    HIPCHK(tm.add_to(t_table));

    phm::AwParams p = ln.params();
    for (int64_t s0 = 0; s0 < S_eval; s0 += pl.Sc_max) {
      const int64_t Sc = std::min<int64_t>(pl.Sc_max, S_eval - s0);
      p.Sc = (int)Sc;
      sp.Ev = (size_t)Sc * Kc;
      st = ln.stage_tips(s0, Sc);
      if (st) return st;
      HIPCHK(tm.start());
      st = ln.passes(p);
      if (st) return st;
      HIPCHK(tm.stop());
      st = ln.fetch_ll(Sc);
      if (st) return st;
      HIPCHK(tm.add_to(t_pass));
      for (int64_t k = 0; k < Kc; ++k)
        for (int64_t s = 0; s < Sc; ++s) {
          const size_t at = (size_t)k * Sc + s;
          const int64_t site = in.paired ? in.site_of_model[m0 + k] : s0 + s;
          const int64_t ev = ll_eval_of(in, s0 + s, m0 + k);
          // an impossible evaluation (or a model whose Pade met a zero pivot) is not drawn: -inf, NaN rows, zero nodes, empty map rows
          const bool possible = ln.possible(k, at);
          loglik[ev] = possible ? ln.llh[at] : ninf;
          st = tl.add(ev, site, m0 + k, (int32_t)at, (int32_t)k, possible, launch);
          if (st) return st;
        }
      st = tl.flush(launch);                             // L of this chunk of sites is overwritten by the next
      if (st) return st;
    }
  }
  st = tl.finish_maps();
  if (st) return st;
  if (g_phm_debug.phase_timing)
    std::fprintf(stderr, "phm_sample_histories_models_wide: Pade %.3f ms, table %.3f ms, passes %.3f ms, sampling %.3f ms, map offsets %.3f ms\n",
                 t_pade, t_table, t_pass, tl.sample_ms, tl.offsets_ms);
  g_phm_last_kernel_ms = t_pade + t_table + t_pass + tl.sample_ms + tl.offsets_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

int32_t phm_sample_histories_models_wide(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                         int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, int32_t draws,
                                         const phm_options* opt, double* stats, double* loglik, int32_t* nodes,
                                         int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state) {
  return sm_entry(SW_NAME, phm::AW_MIN_STATES, phm::EX_MAX_STATES, "9..64 states only: 2..8 states go to phm_sample_histories_models",
                  sw_device, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, draws, opt, stats, loglik, nodes, map_off,
                  map_cap, map_dwell, map_state);
}

}  // extern "C"
