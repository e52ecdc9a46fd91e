// phm_sample_api.cpp -- C-ABI of the exact sampler of histories over many rate matrices and sites
// (phm_sample_histories_models): phm_loglik_models' validation (ll_validate), then per device and per chunk
// of models P_k(t_b) (section 17) and the table of mu_k, B_k and beta; per chunk of sites section 17's tips / up / root launches;
// and per batch of tiles the root, node-level, branch and finish launches of phm_sample.hip, which read P, L and pid in place.
// Histories are addressed by their global index h = e D + d (e: the evaluation's index into loglik), so a shard of models is a
// contiguous range of histories and section 14's per-shard map buffers serve unchanged.  The entry body and the tile driver are
// phm_sample_host.h's (section 19b), shared with phm_sample_wide_api.cpp.
#include "phm_sample_host.h"

namespace {

using namespace phm_ex;
using namespace phm_ll;

const char* const SM_NAME = "phm_sample_histories_models";

int32_t sm_device(const SmInput& sm, int32_t device, int64_t first, int64_t count, double* stats, double* loglik,
                  phm_maps::Host* mh, size_t si) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = sm.ll;
  const int n = in.n, E = in.E;
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.sites_per_model();
  KernelTimer tm;
  double kernel_ms = 0.0;
  LlLanes ln(in);
  SmTiles tl(sm, SM_NAME, stats, mh, si);
  st = ln.upload_tree();
  if (st) return st;
  st = tl.setup(first, count);
  if (st) return st;

  int depth_max = 0;
  for (int64_t k = first; k < first + count; ++k) depth_max = std::max(depth_max, sm.depth[k]);

  // On top of section 17's footprint: mu, B, the table and its depth per model, and a fixed share for the tiles.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  phm::SmParams sp = {};
  st = tl.alloc(free_b, count, INT64_MAX, sp.core);
  if (st) return st;
  const LlPlan pl = ll_plan(free_b, in, count, g_phm_debug.expect_chunk, tl.batch_b,
                            sizeof(double) * (nn + 1 + ((size_t)depth_max + 1) * nn) + sizeof(int32_t), 0);
  const size_t Kpm = (size_t)pl.Kc_max;

  DevBuf dmu, dB, dbeta, ddepth;
  st = ln.alloc(pl);
  if (st) return st;
  HIPCHK(dmu.alloc(sizeof(double) * Kpm)); HIPCHK(dB.alloc(sizeof(double) * nn * Kpm));
  HIPCHK(dbeta.alloc(sizeof(double) * ((size_t)depth_max + 1) * nn * Kpm)); HIPCHK(ddepth.alloc(sizeof(int32_t) * Kpm));
  std::vector<int32_t> depth_h(Kpm);
  phm::LlParams& p = sp.ll;
  sp.mu = dmu.as<double>(); sp.B = dB.as<double>(); sp.beta = dbeta.as<double>(); sp.depth_of = ddepth.as<int32_t>();
  const SmTiles::Launch launch = [&]() {
    const int branch_blocks = (int)std::min<int64_t>(((int64_t)E * sp.core.n_tiles + 3) / 4, 2048);
    return phm::launch_sm_sample(sp, sm.level_off, branch_blocks, tl.maps_mode(), nullptr);
  };

  for (int64_t c0 = 0; c0 < count; c0 += pl.Kc_max) {
    const int64_t Kc = std::min<int64_t>(pl.Kc_max, count - c0);
    st = ln.load_models(first + c0, Kc);
    if (st) return st;
    const int Kp = ln.Kp;
    const int64_t m0 = ln.m0;                            // global index of this chunk's first model
    std::fill(depth_h.begin(), depth_h.end(), 0);
    std::copy_n(sm.depth.begin() + m0, Kc, depth_h.begin());
    HIPCHK(hipMemcpy(ddepth.p, depth_h.data(), sizeof(int32_t) * Kp, hipMemcpyHostToDevice));
    p = ln.params();
    sp.depth = *std::max_element(depth_h.begin(), depth_h.begin() + Kc);
    HIPCHK(tm.start());
    st = ln.expm(p);
    if (st) return st;
    HIPCHK(phm::launch_sm_table(sp, nullptr));
    HIPCHK(tm.stop());
    HIPCHK(tm.add_to(kernel_ms));

    for (int64_t s0 = 0; s0 < S_eval; s0 += pl.Sc_max) {
      const int64_t Sc = std::min<int64_t>(pl.Sc_max, S_eval - s0);
      p.n_sites = (int)Sc;
      st = ln.stage_tips(s0, Sc);
      if (st) return st;
      HIPCHK(tm.start());
      st = ln.passes(p);
      if (st) return st;
      HIPCHK(tm.stop());
      st = ln.fetch_ll(Sc);
      if (st) return st;
      HIPCHK(tm.add_to(kernel_ms));
      for (int64_t s = 0; s < Sc; ++s)
        for (int64_t k = 0; k < Kc; ++k) {
          const int64_t site = in.paired ? in.site_of_model[m0 + k] : s0 + s;
          const int64_t ev = ll_eval_of(in, s0 + s, m0 + k);
          const double ll = ln.llh[(size_t)s * Kp + k];
          loglik[ev] = ll;
          st = tl.add(ev, site, m0 + k, (int32_t)(s * Kp + k), (int32_t)k, std::isfinite(ll), launch);
          if (st) return st;
        }
      st = tl.flush(launch);                             // L of this chunk of sites is overwritten by the next
      if (st) return st;
    }
  }
  st = tl.finish_maps();
  if (st) return st;
  g_phm_last_kernel_ms = kernel_ms + tl.sample_ms + tl.offsets_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

int32_t phm_sample_histories_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                    int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, int32_t draws,
                                    const phm_options* opt, double* stats, double* loglik, int32_t* nodes,
                                    int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state) {
  return sm_entry(SM_NAME, 2, phm::LL_LANE_MAX, "more than 8 states are not supported", sm_device, x, n_states, n_models, Q, pid, n_pid,
                  observe, site_of_model, draws, opt, stats, loglik, nodes, map_off, map_cap, map_dwell, map_state);
}

}  // extern "C"
