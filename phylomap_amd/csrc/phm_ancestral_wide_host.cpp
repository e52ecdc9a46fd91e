// phm_ancestral_wide_host.cpp -- AwLanes (phm_ancestral_wide_host.h): section 23's device buffers, the
// upload of a chunk of models and of a chunk's tips, one launch_expm_pade per model (section 13's kernel, ex_squarings' counts,
// each model with its own error word) and the tips / up / root launches of phm_ancestral_wide.hip.
#include "phm_ancestral_wide_host.h"

#include "phm_exp.h"

namespace phm_ll {

using namespace phm_ex;

int32_t AwLanes::upload_tree() {
  HIPCHK(upload(dt, in.edge_length)); HIPCHK(upload(dobs, in.obs)); HIPCHK(upload(dup, in.up));
  return PHM_OK;
}

int32_t AwLanes::alloc(const AwPlan& pl) {
  plan = pl;
  const int n = in.n, NP = phm::aw_lanes(n);
  const size_t nn = (size_t)n * n, E = (size_t)in.E, NT = (size_t)in.NT;
  const size_t Km = (size_t)pl.Kc_max, Evm = Km * (size_t)pl.Sc_max;
  const size_t tips_b = (size_t)in.T * (in.paired ? Km : (size_t)pl.Sc_max);
  HIPCHK(dQ.alloc(sizeof(double) * nn * Km)); HIPCHK(dpid.alloc(sizeof(double) * n * Km));
  HIPCHK(dsq.alloc(sizeof(int32_t) * E * Km)); HIPCHK(dbad.alloc(sizeof(uint32_t) * Km));
  HIPCHK(dP.alloc(sizeof(double) * E * nn * Km)); HIPCHK(dwork.alloc(sizeof(double) * 5 * nn * E));
  HIPCHK(dL.alloc(sizeof(double) * NT * NP * Evm)); HIPCHK(dsL.alloc(sizeof(int32_t) * NT * Evm));
  HIPCHK(dll.alloc(sizeof(double) * Evm));
  HIPCHK(dtips.alloc(tips_b));
  llh.resize(Evm); tips_h.resize(tips_b); sqh.resize(E * Km); badh.resize(Km);
  return PHM_OK;
}

int32_t AwLanes::load_models(int64_t first, int64_t count) {
  m0 = first; Kc = count;
  const int n = in.n, E = in.E;
  const size_t nn = (size_t)n * n;
  for (int64_t k = 0; k < Kc; ++k)
    for (int b = 0; b < E; ++b) sqh[(size_t)k * E + b] = ex_squarings(in.Qr.data() + (size_t)(m0 + k) * nn, n, in.edge_length[b]);
  HIPCHK(hipMemcpy(dQ.p, in.Qr.data() + (size_t)m0 * nn, sizeof(double) * nn * Kc, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dpid.p, in.pid.data() + (size_t)m0 * n, sizeof(double) * n * Kc, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dsq.p, sqh.data(), sizeof(int32_t) * (size_t)E * Kc, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dbad.p, 0, sizeof(uint32_t) * Kc));
  return PHM_OK;
}

int32_t AwLanes::set_models(const double* Q, const int32_t* sq) {
  const size_t nn = (size_t)in.n * in.n;
  HIPCHK(hipMemcpy(dQ.p, Q, sizeof(double) * nn * Kc, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dsq.p, sq, sizeof(int32_t) * (size_t)in.E * Kc, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dbad.p, 0, sizeof(uint32_t) * Kc));
  return PHM_OK;
}

int32_t AwLanes::expm() const {
  const int n = in.n, E = in.E;
  const size_t nn = (size_t)n * n;
  for (int64_t k = 0; k < Kc; ++k)
    HIPCHK(phm::launch_expm_pade(n, dQ.as<double>() + (size_t)k * nn, dt.as<double>(), dsq.as<int32_t>() + (size_t)k * E, E,
                                 dwork.as<double>(), dP.as<double>() + (size_t)k * E * nn, dbad.as<uint32_t>() + k, nullptr));
  return PHM_OK;
}

int32_t AwLanes::fetch_bad() {
  HIPCHK(hipMemcpy(badh.data(), dbad.p, sizeof(uint32_t) * Kc, hipMemcpyDeviceToHost));
  return PHM_OK;
}

phm::AwParams AwLanes::params() const {
  phm::AwParams p = {};
  p.n = in.n; p.NP = phm::aw_lanes(in.n); p.n_tips = in.T; p.n_edge = in.E; p.root = in.T + in.sched.root; p.Kc = (int)Kc;
  p.tip_model = in.paired ? 1 : 0; p.tip_site = in.paired ? 0 : 1;
  p.P = dP.as<double>(); p.pid = dpid.as<double>(); p.tips = dtips.as<uint8_t>(); p.obs = dobs.as<int32_t>();
  p.L = dL.as<double>(); p.sL = dsL.as<int32_t>(); p.ll = dll.as<double>();
  return p;
}

int32_t AwLanes::stage_tips(int64_t s0, int64_t Sc) {
  const int T = in.T;
  if (in.paired) {                                     // [model][tip]
    for (int64_t k = 0; k < Kc; ++k) {
      const int32_t* y = in.tips_of(in.site_of_model[m0 + k]);
      for (int t = 0; t < T; ++t) tips_h[(size_t)k * T + t] = (uint8_t)y[t];
    }
    HIPCHK(hipMemcpy(dtips.p, tips_h.data(), (size_t)T * Kc, hipMemcpyHostToDevice));
  } else {
    ll_stage_tips_sites(in, s0, Sc, tips_h);           // [site][tip]
    HIPCHK(hipMemcpy(dtips.p, tips_h.data(), (size_t)T * Sc, hipMemcpyHostToDevice));
  }
  return PHM_OK;
}

int32_t AwLanes::passes(const phm::AwParams& p) const {
  const phm::UpStep* up = dup.as<phm::UpStep>();
  HIPCHK(phm::launch_aw_tips(p, nullptr));
  const int32_t st = aw_level_steps(in.up_off, plan.step_max, [&](int k0, int cnt) { return phm::launch_aw_up(p, up + k0, cnt, false, nullptr); });
  if (st) return st;
  HIPCHK(phm::launch_aw_root(p, nullptr));
  return PHM_OK;
}

int32_t AwLanes::fetch_ll(int64_t Sc) {
  HIPCHK(hipMemcpy(llh.data(), dll.p, sizeof(double) * (size_t)Sc * Kc, hipMemcpyDeviceToHost));
  return PHM_OK;
}

}  // namespace phm_ll
