// phm_loglik_api.cpp -- C-ABI of the batched log-likelihood over many rate matrices (phm_loglik_models):
// validation on the host with the helpers phm_expected_stats' ex_validate is made of, then per device and per chunk of models
// P_k(t_b) once and, per chunk of sites, the tips / up / root launches of phm_loglik.hip.  2..8 states run with the models across
// the lanes.  9..64 states are NOT batched: the models go one after the other through section 13's own launches
// (ex_device_setup, and the tips / up / root part of ex_run_passes), for correctness only.
// The checked input and its validation (phm_loglik_host.h) are shared with phm_expected_stats_models (section 18) and defined here.
#include "phm_loglik_host.h"

#include <limits>

namespace phm_ll {

using namespace phm_ex;

int32_t ll_validate(const std::string& fn, const phm_tree* x, int32_t n, int32_t K, const double* Q, const double* pid, int32_t n_pid,
                    const int32_t* observe, const int32_t* site_of_model, const phm_options& o, LlInput& in) {
  if (n < 2 || n > phm::EX_MAX_STATES) return fail(PHM_ERR_BAD_INPUT, fn + "n_states must be in 2..64");
  if (K < 1) return fail(PHM_ERR_BAD_INPUT, fn + "n_models must be >= 1");
  if (n_pid != 1 && n_pid != K) return fail(PHM_ERR_BAD_INPUT, fn + "n_pid must be 1 (shared) or n_models");
  if (o.reduce != 0) return fail(PHM_ERR_BAD_INPUT, fn + "reduce must be 0");
  if (o.n_replicas < 0 || o.n_replicas > (1 << 22)) return fail(PHM_ERR_BAD_INPUT, fn + "n_replicas must be in 0..4194304");
  if (!x->edge || !x->edge_length || !x->states) return fail(PHM_ERR_BAD_INPUT, fn + "x$edge, x$edge.length and x$states are required");
  std::string serr;
  if (!phm::build_schedule(x->n_tips, x->n_node, x->n_edge, x->edge, in.sched, serr)) return fail(PHM_ERR_BAD_INPUT, "tree: " + serr);
  in.n = n; in.K = K; in.T = x->n_tips; in.Nn = x->n_node; in.E = x->n_edge; in.NT = in.T + in.Nn;
  in.S = std::max(1, (int)o.n_replicas);
  in.per_site = o.tips_per_replica != 0;
  in.paired = site_of_model != nullptr;
  in.states = x->states;
  in.site_of_model = site_of_model;
  int32_t st = check_edge_lengths(x);
  if (st) return st;
  in.edge_length.assign(x->edge_length, x->edge_length + in.E);
  const size_t nn = (size_t)n * n;
  in.Qr.resize((size_t)K * nn);
  std::vector<double> qr;
  for (int k = 0; k < K; ++k) {                          // a model that leaves no state (P = I) is legal here
    st = check_generator(Q + (size_t)k * nn, n, qr);
    if (st) return fail(st, "model " + std::to_string(k) + ": " + g_phm_err);
    std::copy(qr.begin(), qr.end(), in.Qr.begin() + (size_t)k * nn);
  }
  in.pid.resize((size_t)K * n);
  for (int k = 0; k < n_pid; ++k) {
    double psum = 0.0;
    st = check_root_prior(pid + (size_t)k * n, n, psum);
    if (st) return fail(st, "pid column " + std::to_string(k) + ": " + g_phm_err);
    for (int i = 0; i < n; ++i) in.pid[(size_t)k * n + i] = pid[(size_t)k * n + i] / psum;
  }
  for (int k = n_pid; k < K; ++k) std::copy(in.pid.begin(), in.pid.begin() + n, in.pid.begin() + (size_t)k * n);
  st = check_observe(observe, n, in.obs);
  if (st) return st;
  const int64_t n_states_in = (int64_t)(in.per_site ? in.S : 1) * in.T;
  for (int64_t k = 0; k < n_states_in; ++k)
    if (in.states[k] < 0 || in.states[k] > n) return fail(PHM_ERR_BAD_INPUT, "x$states must be in 0..n (0: missing)");
  if (site_of_model)
    for (int k = 0; k < K; ++k)
      if (site_of_model[k] < 0 || site_of_model[k] >= in.S)
        return fail(PHM_ERR_BAD_INPUT, fn + "site_of_model[" + std::to_string(k) + "] must be in 0..S-1");
  std::vector<int32_t> order;
  phm::height_levels(in.sched.up, order, in.up_off);
  for (int32_t k : order) in.up.push_back(in.sched.up[k]);
  return PHM_OK;
}

}  // namespace phm_ll

namespace {

using namespace phm_ex;
using namespace phm_ll;

const std::string LL_FN = "phm_loglik_models: ";

// 2..8 states: models [first, first + count) on one device, models across the lanes
int32_t ll_lanes_device(const LlInput& in, int32_t device, int64_t first, int64_t count, double* out) {
  int32_t st = select_device(device);
  if (st) return st;
  const int n = in.n, E = in.E, NT = in.NT, T = in.T;
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.paired ? 1 : in.S;           // sites per model
  KernelTimer tm;
  double kernel_ms = 0.0, ms = 0.0;
  DevBuf dt, dobs, dup;
  HIPCHK(upload(dt, in.edge_length)); HIPCHK(upload(dobs, in.obs)); HIPCHK(upload(dup, in.up));

  // Chunks by free HBM: per model Q, pid and P; per evaluation L, sL, ll (and a tip byte per tip when paired).  P is sized from
  // the free memory too: a 10 000-tip tree at 4 states needs 2.56 MB of it per model.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const bool ws = n > phm::LL_REG_MAX;
  const size_t budget = free_b / 2 > (ws ? LL_WORK : 0) ? free_b / 2 - (ws ? LL_WORK : 0) : 0;
  const size_t per_model = sizeof(double) * ((size_t)E * nn + nn + n) + sizeof(uint32_t);
  const size_t per_eval = sizeof(double) * ((size_t)NT * (n + 1) + 1) + (in.paired ? (size_t)T : 0);
  int64_t Sc_max = std::min<int64_t>(S_eval, 65535);
  int64_t Kc_max = (int64_t)(budget / (per_model + per_eval * (size_t)Sc_max)) / 64 * 64;
  if (Kc_max < 64) {
    Kc_max = 64;
    const size_t per64 = budget / 64;
    Sc_max = std::max<int64_t>(1, std::min<int64_t>(Sc_max, per64 > per_model ? (int64_t)((per64 - per_model) / per_eval) : 1));
  }
  const int chunk = g_phm_debug.expect_chunk;
  if (chunk > 0) {
    Kc_max = std::min<int64_t>(Kc_max, ((int64_t)chunk + 63) / 64 * 64);
    Sc_max = std::min<int64_t>(Sc_max, chunk);
  }
  Kc_max = std::min<int64_t>(Kc_max, (count + 63) / 64 * 64);
  const size_t Kpm = (size_t)Kc_max, Evm = Kpm * (size_t)Sc_max;
  int ne_max = E;
  if (ws) ne_max = (int)std::max<size_t>(1, std::min<size_t>({(size_t)E, (size_t)65535, LL_WORK / (sizeof(double) * 4 * nn * Kpm)}));
  ne_max = std::min(ne_max, 65535);
  if (chunk > 0) ne_max = std::min(ne_max, chunk);

  DevBuf dQ, dpid, dP, dwork, dbad, dL, dsL, dll, dtips;
  HIPCHK(dQ.alloc(sizeof(double) * nn * Kpm)); HIPCHK(dpid.alloc(sizeof(double) * n * Kpm));
  HIPCHK(dP.alloc(sizeof(double) * (size_t)E * nn * Kpm)); HIPCHK(dbad.alloc(sizeof(uint32_t) * Kpm));
  if (ws) HIPCHK(dwork.alloc(sizeof(double) * 4 * nn * Kpm * (size_t)ne_max));
  HIPCHK(dL.alloc(sizeof(double) * (size_t)NT * n * Evm)); HIPCHK(dsL.alloc(sizeof(double) * (size_t)NT * Evm));
  HIPCHK(dll.alloc(sizeof(double) * Evm));
  HIPCHK(dtips.alloc(in.paired ? (size_t)T * Kpm : (size_t)T * (size_t)Sc_max));
  std::vector<double> Qh(nn * Kpm), pidh((size_t)n * Kpm), llh(Evm);
  std::vector<uint8_t> tips_h(in.paired ? (size_t)T * Kpm : (size_t)T * (size_t)Sc_max);

  for (int64_t c0 = 0; c0 < count; c0 += Kc_max) {
    const int64_t Kc = std::min<int64_t>(Kc_max, count - c0);
    const int Kp = (int)((Kc + 63) / 64 * 64);
    const int64_t m0 = first + c0;                       // global index of this chunk's first model
    std::fill(Qh.begin(), Qh.end(), 0.0);
    std::fill(pidh.begin(), pidh.end(), 0.0);
    for (int64_t k = 0; k < Kc; ++k) {
      for (size_t e = 0; e < nn; ++e) Qh[e * Kp + k] = in.Qr[(size_t)(m0 + k) * nn + e];
      for (int i = 0; i < n; ++i) pidh[(size_t)i * Kp + k] = in.pid[(size_t)(m0 + k) * n + i];
    }
    HIPCHK(hipMemcpy(dQ.p, Qh.data(), sizeof(double) * nn * Kp, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dpid.p, pidh.data(), sizeof(double) * n * Kp, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dbad.p, 0, sizeof(uint32_t) * Kp));
    phm::LlParams p = {};
    p.n = n; p.n_tips = T; p.Kp = Kp; p.Kc = (int)Kc; p.paired = in.paired ? 1 : 0;
    p.Q = dQ.as<double>(); p.pid = dpid.as<double>(); p.t = dt.as<double>(); p.P = dP.as<double>();
    p.work = ws ? dwork.as<double>() : nullptr; p.bad = dbad.as<uint32_t>(); p.tips = dtips.as<uint8_t>();
    p.obs = dobs.as<int32_t>(); p.L = dL.as<double>(); p.sL = dsL.as<double>(); p.ll = dll.as<double>();
    p.n_sites = 1;
    HIPCHK(tm.start());
    for (int e0 = 0; e0 < E; e0 += ne_max) HIPCHK(phm::launch_ll_expm(p, e0, std::min(ne_max, E - e0), nullptr));
    HIPCHK(tm.stop());
    HIPCHK(tm.elapsed(ms));
    kernel_ms += ms;

    for (int64_t s0 = 0; s0 < S_eval; s0 += Sc_max) {
      const int64_t Sc = std::min<int64_t>(Sc_max, S_eval - s0);
      p.n_sites = (int)Sc;
      if (in.paired) {                                   // [tip][Kp]: lane k reads the tips of its own site
        std::fill(tips_h.begin(), tips_h.end(), (uint8_t)0);
        for (int64_t k0 = 0; k0 < Kc; k0 += 64) {         // a tile of 64 models at a time: 64 sequential reads, 64-byte writes
          const int kn = (int)std::min<int64_t>(64, Kc - k0);
          const int32_t* y[64];
          for (int k = 0; k < kn; ++k) y[k] = in.tips_of(in.site_of_model[m0 + k0 + k]);
          for (int t = 0; t < T; ++t)
            for (int k = 0; k < kn; ++k) tips_h[(size_t)t * Kp + k0 + k] = (uint8_t)y[k][t];
        }
        HIPCHK(hipMemcpy(dtips.p, tips_h.data(), (size_t)T * Kp, hipMemcpyHostToDevice));
      } else {                                           // [site][tip]
        for (int64_t s = 0; s < Sc; ++s) {
          const int32_t* y = in.tips_of(s0 + s);
          for (int t = 0; t < T; ++t) tips_h[(size_t)s * T + t] = (uint8_t)y[t];
        }
        HIPCHK(hipMemcpy(dtips.p, tips_h.data(), (size_t)T * Sc, hipMemcpyHostToDevice));
      }
      HIPCHK(tm.start());
      HIPCHK(phm::launch_ll_tips(p, nullptr));
      for (size_t l = 0; l + 1 < in.up_off.size(); ++l)
        HIPCHK(phm::launch_ll_up(p, dup.as<phm::UpStep>() + in.up_off[l], in.up_off[l + 1] - in.up_off[l], nullptr));
      HIPCHK(phm::launch_ll_root(p, T + in.sched.root, nullptr));
      HIPCHK(tm.stop());
      HIPCHK(hipMemcpy(llh.data(), dll.p, sizeof(double) * (size_t)Sc * Kp, hipMemcpyDeviceToHost));
      HIPCHK(tm.elapsed(ms));
      kernel_ms += ms;
      for (int64_t s = 0; s < Sc; ++s)
        for (int64_t k = 0; k < Kc; ++k) ll_out(in, out, s0 + s, m0 + k) = llh[(size_t)s * Kp + k];
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
  double kernel_ms = 0.0, ms = 0.0;
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
        for (int64_t s = 0; s < Sc; ++s) ll_out(in, out, s0 + s, m) = ninf;
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
      HIPCHK(tm.elapsed(ms));
      kernel_ms += ms;
      for (int64_t s = 0; s < Sc; ++s) ll_out(in, out, s0 + s, m) = std::isfinite(ps.ll_h[s]) ? ps.ll_h[s] : ninf;
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
