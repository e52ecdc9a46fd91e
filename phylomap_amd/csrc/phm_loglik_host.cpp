// phm_loglik_host.cpp -- the host core of the many-model entry points (phm_loglik_host.h): the one
// validation, LlLanes (section 17's device buffers, the upload of a chunk of models and of a chunk's tips, the P launches and the
// tips / up / root launches of phm_loglik.hip).
#include "phm_loglik_host.h"

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

int32_t LlLanes::upload_tree() {
  HIPCHK(upload(dt, in.edge_length)); HIPCHK(upload(dobs, in.obs)); HIPCHK(upload(dup, in.up));
  return PHM_OK;
}

int32_t LlLanes::alloc(const LlPlan& pl) {
  plan = pl;
  const int n = in.n;
  const size_t nn = (size_t)n * n, E = (size_t)in.E, NT = (size_t)in.NT;
  const size_t Kpm = (size_t)pl.Kc_max, Evm = Kpm * (size_t)pl.Sc_max;
  HIPCHK(dQ.alloc(sizeof(double) * nn * Kpm)); HIPCHK(dpid.alloc(sizeof(double) * n * Kpm));
  HIPCHK(dP.alloc(sizeof(double) * E * nn * Kpm)); HIPCHK(dbad.alloc(sizeof(uint32_t) * Kpm));
  if (n > phm::LL_REG_MAX) HIPCHK(dwork.alloc(sizeof(double) * 4 * nn * Kpm * (size_t)pl.ne_max));
  HIPCHK(dL.alloc(sizeof(double) * NT * n * Evm)); HIPCHK(dsL.alloc(sizeof(double) * NT * Evm));
  HIPCHK(dll.alloc(sizeof(double) * Evm));
  HIPCHK(dtips.alloc((size_t)in.T * (in.paired ? Kpm : (size_t)pl.Sc_max)));
  return PHM_OK;
}

int32_t LlLanes::load_priors(int64_t first, int64_t count) {
  m0 = first; Kc = count; Kp = (int)((count + 63) / 64 * 64);
  ll_stage_rows(in.pid.data() + (size_t)m0 * in.n, (size_t)in.n, Kc, Kp, pidh);
  HIPCHK(hipMemcpy(dpid.p, pidh.data(), sizeof(double) * pidh.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dbad.p, 0, sizeof(uint32_t) * Kp));
  return PHM_OK;
}

int32_t LlLanes::load_models(int64_t first, int64_t count) {
  const size_t nn = (size_t)in.n * in.n;
  ll_stage_rows(in.Qr.data() + (size_t)first * nn, nn, count, (int)((count + 63) / 64 * 64), Qh);
  HIPCHK(hipMemcpy(dQ.p, Qh.data(), sizeof(double) * Qh.size(), hipMemcpyHostToDevice));
  return load_priors(first, count);
}

phm::LlParams LlLanes::params() const {
  phm::LlParams p = {};
  p.n = in.n; p.n_tips = in.T; p.Kp = Kp; p.Kc = (int)Kc; p.paired = in.paired ? 1 : 0;
  p.Q = dQ.as<double>(); p.pid = dpid.as<double>(); p.t = dt.as<double>(); p.P = dP.as<double>();
  p.work = in.n > phm::LL_REG_MAX ? dwork.as<double>() : nullptr; p.bad = dbad.as<uint32_t>(); p.tips = dtips.as<uint8_t>();
  p.obs = dobs.as<int32_t>(); p.L = dL.as<double>(); p.sL = dsL.as<double>(); p.ll = dll.as<double>();
  p.n_sites = 1;
  return p;
}

int32_t LlLanes::expm(const phm::LlParams& p) const {
  for (int e0 = 0; e0 < in.E; e0 += plan.ne_max) HIPCHK(phm::launch_ll_expm(p, e0, std::min(plan.ne_max, in.E - e0), nullptr));
  return PHM_OK;
}

int32_t LlLanes::stage_tips(int64_t s0, int64_t Sc) {
  if (in.paired) ll_stage_tips_paired(in, m0, Kc, Kp, tips_h);       // [tip][Kp]: lane k reads the tips of its own site
  else ll_stage_tips_sites(in, s0, Sc, tips_h);                     // [site][tip]
  HIPCHK(hipMemcpy(dtips.p, tips_h.data(), tips_h.size(), hipMemcpyHostToDevice));
  return PHM_OK;
}

int32_t LlLanes::passes(const phm::LlParams& p) const {
  HIPCHK(phm::launch_ll_tips(p, nullptr));
  for (size_t l = 0; l + 1 < in.up_off.size(); ++l)
    HIPCHK(phm::launch_ll_up(p, dup.as<phm::UpStep>() + in.up_off[l], in.up_off[l + 1] - in.up_off[l], nullptr));
  HIPCHK(phm::launch_ll_root(p, in.T + in.sched.root, nullptr));
  return PHM_OK;
}

int32_t LlLanes::fetch_ll(int64_t Sc) {
  llh.resize((size_t)Sc * Kp);
  HIPCHK(hipMemcpy(llh.data(), dll.p, sizeof(double) * llh.size(), hipMemcpyDeviceToHost));
  return PHM_OK;
}

}  // namespace phm_ll
