// phm_loglik_api.cpp -- C-ABI of the batched log-likelihood over many rate matrices (phm_loglik_models):
// validation on the host (ll_validate), then per device and per chunk of models
// P_k(t_b) once and, per chunk of sites, the tips / up / root launches of phm_loglik.hip.  2..8 states run with the models across
// the lanes.  9..64 states are NOT batched: the models go one after the other through section 13's own launches
// (ex_device_setup, and the tips / up / root part of ex_run_passes), for correctness only.
// The checked input, its validation and the lanes' device state are the many-model host core's (phm_loglik_host.h).
#include "phm_loglik_host.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;

const std::string LL_FN = "phm_loglik_models: ";

// 2..8 states: models [first, first + count) on one device, models across the lanes
int32_t ll_lanes_device(const LlInput& in, int32_t device, int64_t first, int64_t count, double* out) {
  int32_t st = select_device(device);
  if (st) return st;
  const int64_t S_eval = in.sites_per_model();
  KernelTimer tm;
  double kernel_ms = 0.0;
  LlLanes ln(in);
  st = ln.upload_tree();
  if (st) return st;
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const LlPlan pl = ll_plan(free_b, in, count, g_phm_debug.expect_chunk, 0, 0, 0);
  st = ln.alloc(pl);
  if (st) return st;

  for (int64_t c0 = 0; c0 < count; c0 += pl.Kc_max) {
    const int64_t Kc = std::min<int64_t>(pl.Kc_max, count - c0);
    st = ln.load_models(first + c0, Kc);
    if (st) return st;
    phm::LlParams p = ln.params();
    HIPCHK(tm.start());
    st = ln.expm(p);
    if (st) return st;
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
        for (int64_t k = 0; k < Kc; ++k) out[ll_eval_of(in, s0 + s, ln.m0 + k)] = ln.llh[(size_t)s * ln.Kp + k];
    }
  }
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

// 9..64 states: one model at a time through section 13's P, tips, up and root launches (not batched)
int32_t ll_wide_device(const LlInput& in, int32_t device, int64_t first, int64_t count, double* out) {
  int32_t st = select_device(device);
  if (st) return st;
  const int n = in.n, T = in.T;
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.paired ? 1 : in.S;
  const double ninf = -std::numeric_limits<double>::infinity();
  ExInput ex;
  ex.n = n; ex.T = T; ex.Nn = in.Nn; ex.E = in.E; ex.NT = in.NT; ex.S = in.S; ex.cols = n + n * (n - 1);
  ex.per_site = in.per_site; ex.states = in.states; ex.sched = in.sched;
  ex.edge_length = in.edge_length; ex.obs = in.obs; ex.up = in.up; ex.up_off = in.up_off;
  ex.sq.resize(in.E);
  int64_t Sc_max = 0;
  st = ex_sites_per_chunk(ex_pass_bytes(ex), S_eval, Sc_max);
  if (st) return st;
  ExPasses ps;
  st = ps.alloc(ex, (size_t)Sc_max);
  if (st) return st;
  KernelTimer tm;
  double kernel_ms = 0.0;
  for (int64_t m = first; m < first + count; ++m) {
    ex.Qr.assign(in.Qr.begin() + (size_t)m * nn, in.Qr.begin() + (size_t)(m + 1) * nn);
    ex.pid.assign(in.pid.begin() + (size_t)m * n, in.pid.begin() + (size_t)(m + 1) * n);
    for (int b = 0; b < in.E; ++b) ex.sq[b] = ex_squarings(ex.Qr.data(), n, ex.edge_length[b]);
    ExDevice dev;
    st = ex_device_setup(LL_FN, ex, dev, tm, kernel_ms);
    const bool singular = st == PHM_ERR_BAD_INPUT;       // the one input failure left after ll_validate: a zero pivot in some P
    if (st && !singular) return st;
    for (int64_t s0 = 0; s0 < S_eval; s0 += Sc_max) {
      const int64_t Sc = std::min<int64_t>(Sc_max, S_eval - s0);
      if (singular) {
        for (int64_t s = 0; s < Sc; ++s) out[ll_eval_of(in, s0 + s, m)] = ninf;
        continue;
      }
      const int Sp = (int)((Sc + 63) / 64 * 64);
      std::fill(ps.tips_h.begin(), ps.tips_h.end(), (uint8_t)0);
      for (int64_t s = 0; s < Sc; ++s) {
        const int32_t* y = in.tips_of(in.paired ? in.site_of_model[m] : s0 + s);
        for (int t = 0; t < T; ++t) ps.tips_h[(size_t)t * Sp + s] = (uint8_t)y[t];
      }
      HIPCHK(hipMemcpy(ps.dtips.p, ps.tips_h.data(), (size_t)T * Sp, hipMemcpyHostToDevice));
      const phm::ExPassParams pp = ps.params(ex, dev, Sp);
      HIPCHK(tm.start());
      HIPCHK(phm::launch_ex_tips(pp, ps.dtips.as<uint8_t>(), dev.dobs.as<int32_t>(), nullptr));
      for (size_t l = 0; l + 1 < ex.up_off.size(); ++l)
        HIPCHK(phm::launch_ex_up(pp, dev.dup.as<phm::UpStep>() + ex.up_off[l], ex.up_off[l + 1] - ex.up_off[l], nullptr));
      HIPCHK(phm::launch_ex_root(pp, T + ex.sched.root, dev.dpid.as<double>(), nullptr));
      HIPCHK(tm.stop());
      HIPCHK(hipMemcpy(ps.ll_h.data(), ps.dll.p, sizeof(double) * Sc, hipMemcpyDeviceToHost));
      HIPCHK(tm.add_to(kernel_ms));
      for (int64_t s = 0; s < Sc; ++s) out[ll_eval_of(in, s0 + s, m)] = std::isfinite(ps.ll_h[s]) ? ps.ll_h[s] : ninf;
    }
  }
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Models are independent: with phm_options.n_devices > 1 device d computes a contiguous range of them (phm_plan_shards,
// run_shards); every output value is the one-device value bit for bit.
int32_t phm_loglik_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid, int32_t n_pid,
                          const int32_t* observe, const int32_t* site_of_model, const phm_options* opt, double* out) {
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid || !out) return fail(PHM_ERR_BAD_INPUT, LL_FN + "NULL argument (only observe, site_of_model and opt may be NULL)");
  LlInput in;
  int32_t st = ll_validate(LL_FN, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, o, in);
  if (st) return st;
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, in.K, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) {
    return in.n <= phm::LL_LANE_MAX ? ll_lanes_device(in, sh.device, sh.first, sh.count, out)
                                    : ll_wide_device(in, sh.device, sh.first, sh.count, out);
  });
}

}  // extern "C"
