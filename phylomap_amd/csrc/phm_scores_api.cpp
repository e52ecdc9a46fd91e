// phm_scores_api.cpp -- C-ABI of the exact conditional expectations for many rate matrices in one call
// (phm_expected_stats_models): phm_loglik_models' validation (ll_validate) and its limit on mu t_b, then per
// device and per chunk of models P_k(t_b) once and, per chunk of sites, section 17's tips / up / root launches (LlLanes) followed by the
// down pass, the branch stage and the run totals of phm_scores.hip.  2..8 states run with the models across the lanes.  9..64
// states are NOT batched: the models go one after the other through phm_expected_stats itself, for correctness only.
#include "phm_loglik_host.h"
#include "phm_scores.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;

const std::string SC_FN = "phm_expected_stats_models: ";
constexpr size_t SC_SCRATCH = size_t(256) << 20;       // run totals of one branch-stage launch

struct ScInput {
  LlInput ll;
  int cols = 0;
  int64_t n_eval = 0;                                   // S * K (cross) or K (paired): rows of stats, values of loglik
  std::vector<phm::ExDown> down;                        // grouped by the depth of the parent
  std::vector<int32_t> down_off, child_row;
  const double* Q = nullptr;                            // the caller's arrays (9..64 states hand them on)
  const double* pid = nullptr;
  const int32_t* observe = nullptr;
  int32_t n_pid = 0;
  const phm_tree* x = nullptr;
  phm_options opt;
};

int32_t sc_prepare(ScInput& sc) {
  LlInput& in = sc.ll;
  const int n = in.n;
  sc.cols = n + n * (n - 1);
  sc.n_eval = in.paired ? in.K : (int64_t)in.S * in.K;
  const size_t nn = (size_t)n * n;
  for (int k = 0; k < in.K; ++k) {
    double mu = 0.0;
    for (int i = 0; i < n; ++i) mu = std::max(mu, -in.Qr[(size_t)k * nn + (size_t)i * n + i]);
    if (n > phm::LL_LANE_MAX && !(mu > 0.0))
      return fail(PHM_ERR_UNSUPPORTED, SC_FN + "model " + std::to_string(k) + " leaves no state: not supported with more than 8 states");
    for (int b = 0; b < in.E; ++b)
      if (mu * in.edge_length[b] > EX_MAX_JUMP_MEAN)
        return fail(PHM_ERR_UNSUPPORTED, "model " + std::to_string(k) + ", edge row " + std::to_string(b + 1) + ": max(-q_ii) * t_b above 1e6");
  }
  ex_down_schedule(in.sched, in.T, sc.down, sc.down_off, &sc.child_row);
  return PHM_OK;
}

// 2..8 states: models [first, first + count) on one device, models across the lanes
int32_t sc_lanes_device(const ScInput& sc, int32_t device, int64_t first, int64_t count, double* stats, double* loglik) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = sc.ll;
  const int n = in.n, E = in.E, NT = in.NT, cols = sc.cols;
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.sites_per_model();
  const int n_runs = (E + phm::SC_RUN - 1) / phm::SC_RUN;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  KernelTimer tm;
  double kernel_ms = 0.0;
  LlLanes ln(in);
  DevBuf ddown, dchild;
  st = ln.upload_tree();
  if (st) return st;
  HIPCHK(upload(ddown, sc.down)); HIPCHK(upload(dchild, sc.child_row));

  // On top of section 17's footprint: per model mu and B; per evaluation O, F with their exponents, lam and the totals.  The run
  // totals of one branch-stage launch take a fixed share.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const bool ws = n > phm::LL_REG_MAX;
  const int chunk = g_phm_debug.expect_chunk;
  const LlPlan pl = ll_plan(free_b, in, count, chunk, SC_SCRATCH, sizeof(double) * (nn + 1),
                            sizeof(double) * ((size_t)NT * (n + 1) + (size_t)E * (n + 1) + 1 + cols));
  const size_t Kpm = (size_t)pl.Kc_max, Evm = Kpm * (size_t)pl.Sc_max;
  int nr_max = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n_runs, (size_t)65535, SC_SCRATCH / (sizeof(double) * cols * Evm)}));
  if (chunk > 0) nr_max = std::min(nr_max, std::max(1, chunk / phm::SC_RUN));

  DevBuf dmu, dB, dO, dsO, dF, dsF, dlam, druns, dtot;
  st = ln.alloc(pl);
  if (st) return st;
  HIPCHK(dmu.alloc(sizeof(double) * Kpm));
  if (ws) HIPCHK(dB.alloc(sizeof(double) * nn * Kpm));
  HIPCHK(dO.alloc(sizeof(double) * (size_t)NT * n * Evm)); HIPCHK(dsO.alloc(sizeof(double) * (size_t)NT * Evm));
  HIPCHK(dF.alloc(sizeof(double) * (size_t)E * n * Evm)); HIPCHK(dsF.alloc(sizeof(double) * (size_t)E * Evm));
  HIPCHK(dlam.alloc(sizeof(double) * Evm));
  HIPCHK(druns.alloc(sizeof(double) * cols * (size_t)nr_max * Evm)); HIPCHK(dtot.alloc(sizeof(double) * cols * Evm));
  std::vector<double> toth((size_t)cols * Evm);

  for (int64_t c0 = 0; c0 < count; c0 += pl.Kc_max) {
    const int64_t Kc = std::min<int64_t>(pl.Kc_max, count - c0);
    st = ln.load_models(first + c0, Kc);
    if (st) return st;
    const int Kp = ln.Kp;
    const int64_t m0 = ln.m0;                            // global index of this chunk's first model
    phm::ScParams sp = {};
    phm::LlParams& p = sp.ll;
    p = ln.params();
    sp.n_edge = E; sp.root = in.T + in.sched.root; sp.mu = dmu.as<double>(); sp.B = ws ? dB.as<double>() : nullptr;
    sp.child = dchild.as<int32_t>(); sp.O = dO.as<double>(); sp.sO = dsO.as<double>(); sp.F = dF.as<double>();
    sp.sF = dsF.as<double>(); sp.lam = dlam.as<double>(); sp.runs = druns.as<double>(); sp.tot = dtot.as<double>();
    HIPCHK(tm.start());
    st = ln.expm(p);
    if (st) return st;
    HIPCHK(phm::launch_sc_model(sp, nullptr));
    HIPCHK(tm.stop());
    HIPCHK(tm.add_to(kernel_ms));

    for (int64_t s0 = 0; s0 < S_eval; s0 += pl.Sc_max) {
      const int64_t Sc = std::min<int64_t>(pl.Sc_max, S_eval - s0);
      p.n_sites = (int)Sc;
      const size_t Ev = (size_t)Sc * Kp;
      st = ln.stage_tips(s0, Sc);
      if (st) return st;
      HIPCHK(hipMemset(dtot.p, 0, sizeof(double) * cols * Ev));
      HIPCHK(tm.start());
      st = ln.passes(p);
      if (st) return st;
      HIPCHK(phm::launch_sc_root(sp, nullptr));
      for (size_t l = 0; l + 1 < sc.down_off.size(); ++l)
        HIPCHK(phm::launch_sc_down(sp, ddown.as<phm::ExDown>() + sc.down_off[l], sc.down_off[l + 1] - sc.down_off[l], nullptr));
      for (int r0 = 0; r0 < n_runs; r0 += nr_max) {
        const int nr = std::min(nr_max, n_runs - r0);
        HIPCHK(phm::launch_sc_branch(sp, r0, nr, nullptr));
        HIPCHK(phm::launch_sc_total(sp, nr, nullptr));
      }
      HIPCHK(tm.stop());
      st = ln.fetch_ll(Sc);
      if (st) return st;
      HIPCHK(hipMemcpy(toth.data(), dtot.p, sizeof(double) * cols * Ev, hipMemcpyDeviceToHost));
      HIPCHK(tm.add_to(kernel_ms));
      for (int64_t s = 0; s < Sc; ++s)
        for (int64_t k = 0; k < Kc; ++k) {
          const int64_t ev = ll_eval_of(in, s0 + s, m0 + k);
          const double ll = ln.llh[(size_t)s * Kp + k];
          loglik[ev] = ll;
          const bool possible = std::isfinite(ll);       // an impossible evaluation: -inf and a row of NaN
          for (int col = 0; col < cols; ++col)
            stats[ev + sc.n_eval * col] = possible ? toth[(size_t)col * Ev + (size_t)s * Kp + k] : nan;
        }
    }
  }
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

// 9..64 states: one model at a time through phm_expected_stats (not batched).  An impossible site fails that call as a whole, so a
// model with one is run again site by site.
int32_t sc_wide_device(const ScInput& sc, int32_t device, int64_t first, int64_t count, double* stats, double* loglik) {
  const LlInput& in = sc.ll;
  const int n = in.n, cols = sc.cols;
  const size_t nn = (size_t)n * n;
  const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  const int64_t S_eval = in.paired ? 1 : in.S;
  std::vector<double> st_h((size_t)S_eval * cols), ll_h((size_t)S_eval);
  double kernel_ms = 0.0;
  for (int64_t m = first; m < first + count; ++m) {
    const double* Qm = sc.Q + (size_t)m * nn;
    const double* pm = sc.pid + (sc.n_pid == 1 ? 0 : (size_t)m * n);
    // sites [lo, lo + cnt) of the model (paired: its own site) into st_h / ll_h at [0, cnt)
    auto run = [&](int64_t lo, int64_t cnt) -> int32_t {
      phm_tree t = *sc.x;
      phm_options o = sc.opt;
      o.device = device; o.n_devices = 0;
      t.states = in.tips_of(in.paired ? in.site_of_model[m] : lo);
      o.n_replicas = (int32_t)cnt;
      o.tips_per_replica = (!in.paired && in.per_site) ? 1 : 0;
      const int32_t st = phm_expected_stats(&t, n, Qm, pm, sc.observe, &o, st_h.data(), ll_h.data(), nullptr, nullptr);
      kernel_ms += g_phm_last_kernel_ms;
      return st;
    };
    auto put = [&](int64_t lo, int64_t cnt, bool ok) {
      for (int64_t s = 0; s < cnt; ++s) {
        const int64_t ev = ll_eval_of(in, lo + s, m);
        loglik[ev] = ok ? ll_h[s] : ninf;
        for (int col = 0; col < cols; ++col) stats[ev + sc.n_eval * col] = ok ? st_h[(size_t)s + (size_t)cnt * col] : nan;
      }
    };
    int32_t st = run(0, S_eval);
    if (st == PHM_OK) { put(0, S_eval, true); continue; }
    if (st == PHM_ERR_BAD_INPUT) { put(0, S_eval, false); continue; }      // the one input failure left: a zero pivot in some P
    if (st != PHM_ERR_ZERO_PROB) return st;
    for (int64_t s = 0; s < S_eval; ++s) {
      st = S_eval == 1 ? PHM_ERR_ZERO_PROB : run(s, 1);
      if (st && st != PHM_ERR_ZERO_PROB) return st;
      put(s, 1, st == PHM_OK);
    }
  }
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Models are independent: with phm_options.n_devices > 1 device d computes a contiguous range of them (phm_plan_shards,
// run_shards); every output value is the one-device value bit for bit.
int32_t phm_expected_stats_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                  int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const phm_options* opt,
                                  double* stats, double* loglik) {
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid || !stats || !loglik)
    return fail(PHM_ERR_BAD_INPUT, SC_FN + "NULL argument (only observe, site_of_model and opt may be NULL)");
  ScInput sc;
  int32_t st = ll_validate(SC_FN, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, o, sc.ll);
  if (st) return st;
  sc.Q = Q; sc.pid = pid; sc.observe = observe; sc.n_pid = n_pid; sc.x = x; sc.opt = o;
  st = sc_prepare(sc);
  if (st) return st;
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, sc.ll.K, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) {
    return sc.ll.n <= phm::LL_LANE_MAX ? sc_lanes_device(sc, sh.device, sh.first, sh.count, stats, loglik)
                                       : sc_wide_device(sc, sh.device, sh.first, sh.count, stats, loglik);
  });
}

}  // extern "C"
