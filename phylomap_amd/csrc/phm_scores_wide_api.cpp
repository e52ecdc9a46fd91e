// phm_scores_wide_api.cpp -- C-ABI of the exact conditional expectations for many rate matrices at 9..64 states
// (phm_expected_stats_models_wide): phm_expected_stats_models' arguments, validation (ll_validate) and its
// limit on mu t_b, then per device and per chunk of models P_k(t_b) and, per chunk of sites, section 23's tips / up / root
// launches (AwLanes, phm_ancestral_wide_host.h; the root stores lam) and section 23's down pass with F stored, followed by the
// branch stage and the run totals of phm_scores_wide.hip.  stats == NULL asks for the log-likelihoods alone: the Pade launches and
// AwLanes' passes, no down pass and no branch stage.  Which form of the branch stage a (model, edge) item takes is decided here
// (sw_form_terms) and uploaded as one int32 per item.  An evaluation touches no other evaluation's buffers and the sums over the
// branches are grouped by compile-time constants, so neither the chunks nor the shards change an output bit.
#include "phm_ancestral_wide_host.h"
#include "phm_scores_wide.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;

const std::string SCW_FN = "phm_expected_stats_models_wide: ";
constexpr size_t SCW_SCRATCH = size_t(256) << 20;      // run totals of one branch-stage launch

struct ScwInput {
  LlInput ll;
  int cols = 0;
  int64_t n_eval = 0;                                   // S * K (cross) or K (paired): rows of stats, values of loglik
  std::vector<double> mu;                               // [K] max_i(-q_ii)
  std::vector<phm::ExDown> down;                        // grouped by the depth of the parent
  std::vector<int32_t> down_off, child_row;
};

// full: the statistics are asked for.  The limit on mu t_b is the branch stage's (it runs ~mu t_b steps), so the log-likelihoods alone
// are not held to it: api.loglik_models keeps phm_loglik_models' domain.
int32_t scw_prepare(ScwInput& sc, bool full) {
  LlInput& in = sc.ll;
  const int n = in.n;
  sc.cols = n + n * (n - 1);
  sc.n_eval = in.paired ? in.K : (int64_t)in.S * in.K;
  const size_t nn = (size_t)n * n;
  sc.mu.assign(in.K, 0.0);
  for (int k = 0; k < in.K; ++k) {
    double mu = 0.0;
    for (int i = 0; i < n; ++i) mu = std::max(mu, -in.Qr[(size_t)k * nn + (size_t)i * n + i]);
    sc.mu[k] = mu;
    for (int b = 0; b < in.E; ++b)
      if (full && mu * in.edge_length[b] > EX_MAX_JUMP_MEAN)
        return fail(PHM_ERR_UNSUPPORTED, SCW_FN + "model " + std::to_string(k) + ", edge row " + std::to_string(b + 1) + ": max(-q_ii) * t_b above 1e6");
  }
  if (full) ex_down_schedule(in.sched, in.T, sc.down, sc.down_off, &sc.child_row);
  return PHM_OK;
}

// models [first, first + count) on one device; stats NULL: the log-likelihoods alone
int32_t scw_device(const ScwInput& sc, int32_t device, int64_t first, int64_t count, double* stats, double* loglik) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = sc.ll;
  const int n = in.n, E = in.E, NT = in.NT, cols = sc.cols, NP = phm::aw_lanes(n);
  const size_t nn = (size_t)n * n;
  const bool full = stats != nullptr;
  const int64_t S_eval = in.sites_per_model();
  const int n_runs = (E + phm::SC_RUN - 1) / phm::SC_RUN;
  const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  KernelTimer tm;
  double kernel_ms = 0.0;
  AwLanes ln(in);
  DevBuf ddown, dchild;
  st = ln.upload_tree();
  if (st) return st;
  if (full) { HIPCHK(upload(ddown, sc.down)); HIPCHK(upload(dchild, sc.child_row)); }

  // On top of section 23's footprint: per model mu, B and the form words; per evaluation O, F with their exponents, lam and the
  // totals.  The run totals of one branch-stage launch take a fixed share, and a chunk's totals never more than that share.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const int chunk = g_phm_debug.expect_chunk;
  const size_t vec_b = sizeof(double) * NP + sizeof(int32_t);
  AwPlan pl = aw_plan(free_b, in, count, chunk, full ? SCW_SCRATCH : 0, full ? sizeof(double) * (nn + 1) + sizeof(int32_t) * (size_t)E : 0,
                      full ? vec_b * (size_t)NT + vec_b * (size_t)E + sizeof(double) * (1 + (size_t)cols) : 0);
  if (full) {
    const size_t row_b = sizeof(double) * (size_t)cols;
    if (row_b * (size_t)pl.Kc_max * (size_t)pl.Sc_max > SCW_SCRATCH) {
      pl.Kc_max = std::max<int64_t>(1, (int64_t)(SCW_SCRATCH / (row_b * (size_t)pl.Sc_max)));
      if (pl.Kc_max == 1) pl.Sc_max = std::min<int64_t>(pl.Sc_max, (int64_t)(SCW_SCRATCH / row_b));
    }
  }
  const int step_max = pl.step_max;
  const size_t Km = (size_t)pl.Kc_max, Evm = Km * (size_t)pl.Sc_max;
  int nr_max = 1;
  if (full) {
    nr_max = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n_runs, (size_t)phm::AW_GRID_MAX, SCW_SCRATCH / (sizeof(double) * cols * Evm)}));
    if (chunk > 0) nr_max = std::min(nr_max, std::max(1, chunk / phm::SC_RUN));
  }

  DevBuf dmu, dB, dform, dO, dsO, dF, dsF, dlam, druns, dtot;
  st = ln.alloc(pl);
  if (st) return st;
  if (full) {
    HIPCHK(dmu.alloc(sizeof(double) * Km)); HIPCHK(dB.alloc(sizeof(double) * nn * Km)); HIPCHK(dform.alloc(sizeof(int32_t) * (size_t)E * Km));
    HIPCHK(dO.alloc(sizeof(double) * (size_t)NT * NP * Evm)); HIPCHK(dsO.alloc(sizeof(int32_t) * (size_t)NT * Evm));
    HIPCHK(dF.alloc(sizeof(double) * (size_t)E * NP * Evm)); HIPCHK(dsF.alloc(sizeof(int32_t) * (size_t)E * Evm));
    HIPCHK(dlam.alloc(sizeof(double) * Evm));
    HIPCHK(druns.alloc(sizeof(double) * cols * (size_t)nr_max * Evm)); HIPCHK(dtot.alloc(sizeof(double) * cols * Evm));
  }
  std::vector<double> toth(full ? (size_t)cols * Evm : 0);
  std::vector<int32_t> formh(full ? (size_t)E * Km : 0);

  for (int64_t c0 = 0; c0 < count; c0 += pl.Kc_max) {
    const int64_t Kc = std::min<int64_t>(pl.Kc_max, count - c0);
    const int64_t m0 = first + c0;                       // global index of this chunk's first model
    st = ln.load_models(m0, Kc);
    if (st) return st;
    phm::ScwParams sp = {};
    phm::AwParams& p = sp.aw;
    p = ln.params();
    p.Sc = 1;
    if (full) {
      for (int64_t k = 0; k < Kc; ++k)
        for (int b = 0; b < E; ++b) formh[(size_t)k * E + b] = phm::sw_form_terms(sc.mu[m0 + k] * in.edge_length[b], phm::SW_M_CAP);
      HIPCHK(hipMemcpy(dform.p, formh.data(), sizeof(int32_t) * (size_t)E * Kc, hipMemcpyHostToDevice));
      p.O = dO.as<double>(); p.sO = dsO.as<int32_t>(); p.F = dF.as<double>(); p.sF = dsF.as<int32_t>(); p.lam = dlam.as<double>();
      sp.Q = ln.dQ.as<double>(); sp.t = ln.dt.as<double>(); sp.child = dchild.as<int32_t>(); sp.mu = dmu.as<double>();
      sp.B = dB.as<double>(); sp.form = dform.as<int32_t>(); sp.runs = druns.as<double>(); sp.tot = dtot.as<double>();
    }
    HIPCHK(tm.start());
    st = ln.expm();
    if (st) return st;
    if (full) HIPCHK(phm::launch_scw_model(sp, nullptr));
    HIPCHK(tm.stop());
    st = ln.fetch_bad();
    if (st) return st;
    HIPCHK(tm.add_to(kernel_ms));

    for (int64_t s0 = 0; s0 < S_eval; s0 += pl.Sc_max) {
      const int64_t Sc = std::min<int64_t>(pl.Sc_max, S_eval - s0);
      p.Sc = (int)Sc;
      const size_t Ev = (size_t)Sc * Kc;
      st = ln.stage_tips(s0, Sc);
      if (st) return st;
      if (full) HIPCHK(hipMemset(dtot.p, 0, sizeof(double) * cols * Ev));
      const phm::ExDown* down = ddown.as<phm::ExDown>();
      HIPCHK(tm.start());
      st = ln.passes(p);
      if (st) return st;
      if (full) {
        st = aw_level_steps(sc.down_off, step_max, [&](int k0, int cnt) { return phm::launch_aw_down(p, down + k0, cnt, nullptr); });
        if (st) return st;
        for (int r0 = 0; r0 < n_runs; r0 += nr_max) {
          const int nr = std::min(nr_max, n_runs - r0);
          HIPCHK(phm::launch_scw_branch(sp, r0, nr, nullptr));
          HIPCHK(phm::launch_scw_total(sp, nr, nullptr));
        }
      }
      HIPCHK(tm.stop());
      st = ln.fetch_ll(Sc);
      if (st) return st;
      if (full) HIPCHK(hipMemcpy(toth.data(), dtot.p, sizeof(double) * cols * Ev, hipMemcpyDeviceToHost));
      HIPCHK(tm.add_to(kernel_ms));
      // the output stage; an impossible evaluation (or a model whose Pade met a zero pivot) gets -inf and a row of NaN
      for (int64_t k = 0; k < Kc; ++k)
        for (int64_t s = 0; s < Sc; ++s) {
          const size_t at = (size_t)k * Sc + s;
          const int64_t ev = ll_eval_of(in, s0 + s, m0 + k);
          const bool possible = ln.possible(k, at);
          loglik[ev] = possible ? ln.llh[at] : ninf;
          if (full)
            for (int col = 0; col < cols; ++col) stats[ev + sc.n_eval * col] = possible ? toth[at * cols + col] : nan;
        }
    }
  }
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Models are independent: with phm_options.n_devices > 1 device d computes a contiguous range of them (phm_plan_shards,
// run_shards); every output value is the one-device value bit for bit.
int32_t phm_expected_stats_models_wide(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                       int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const phm_options* opt,
                                       double* stats, double* loglik) {
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid || !loglik)
    return fail(PHM_ERR_BAD_INPUT, SCW_FN + "NULL argument (only observe, site_of_model, opt and stats may be NULL)");
  ScwInput sc;
  int32_t st = ll_validate(SCW_FN, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, o, sc.ll);
  if (st) return st;
  if (sc.ll.n < phm::AW_MIN_STATES) return fail(PHM_ERR_UNSUPPORTED, SCW_FN + "9..64 states only: 2..8 states go to phm_expected_stats_models");
  if ((int64_t)sc.ll.S * sc.ll.K > (int64_t)INT32_MAX) return fail(PHM_ERR_BAD_INPUT, SCW_FN + "sites * models must fit in 31 bits");
  st = scw_prepare(sc, stats != nullptr);
  if (st) return st;
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, sc.ll.K, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) { return scw_device(sc, sh.device, sh.first, sh.count, stats, loglik); });
}

}  // extern "C"
