// phm_ancestral_api.cpp -- C-ABI of the ancestral states for many rate matrices in one call (phm_ancestral_models, DESIGN.md
// section 21): the checks, the node selection and the shards are an_entry's (phm_ancestral_host.h), shared with
// phm_ancestral_models_wide; then per device and per chunk of models P_k(t_b) once and, per chunk of sites, section 17's tips / up /
// root launches (LlLanes) followed by what was asked for: section
// 18's root and down launches with the node-posterior kernel, and the max-product up pass, root and traceback of
// phm_ancestral.hip.  The output stage is on the HOST: the selected posterior rows ([selected][state][Ev]) and the state bytes
// ([node row][Ev]) are copied back and written into the caller's [evaluation][node][state] layout here.
#include "phm_ancestral.h"
#include "phm_ancestral_host.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;

const std::string AN_FN = "phm_ancestral_models: ";

// models [first, first + count) on one device, models across the lanes
int32_t an_device(const AnInput& an, int32_t device, int64_t first, int64_t count, double* loglik, double* node_post,
                  int32_t* joint_states, double* joint_logp) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = an.ll;
  const int n = in.n, E = in.E, NT = in.NT, T = in.T, Nn = in.Nn, J = an.J;
  const bool marg = node_post != nullptr, joint = joint_states != nullptr;
  const int64_t S_eval = in.sites_per_model();
  const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  KernelTimer tm;
  double kernel_ms = 0.0;
  LlLanes ln(in);
  DevBuf ddown, dsel;
  st = ln.upload_tree();
  if (st) return st;
  HIPCHK(upload(ddown, an.down));
  if (marg) HIPCHK(upload(dsel, an.sel));

  // On top of section 17's footprint: for the marginals O and F with their exponents, lam and the selected posterior rows; for
  // the joint reconstruction M, sM, a pointer word per edge, a state byte per node and the log of the maximum.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  size_t per_eval = 0;
  if (marg) per_eval += sizeof(double) * ((size_t)NT * (n + 1) + (size_t)E * (n + 1) + 1 + (size_t)J * n);
  if (joint) per_eval += sizeof(double) * ((size_t)Nn * (n + 1) + 1) + sizeof(uint32_t) * (size_t)E + (size_t)NT;
  const int chunk = g_phm_debug.expect_chunk;
  const LlPlan pl = ll_plan(free_b, in, count, chunk, 0, 0, per_eval);
  const size_t Evm = (size_t)pl.Kc_max * (size_t)pl.Sc_max;
  const int step_max = chunk > 0 ? std::min(65535, chunk) : 65535;      // level steps (and selected rows) of one launch

  DevBuf dO, dsO, dF, dsF, dlam, dpost, dM, dsM, dptr, dx, djl;
  st = ln.alloc(pl);
  if (st) return st;
  if (marg) {
    HIPCHK(dO.alloc(sizeof(double) * (size_t)NT * n * Evm)); HIPCHK(dsO.alloc(sizeof(double) * (size_t)NT * Evm));
    HIPCHK(dF.alloc(sizeof(double) * (size_t)E * n * Evm)); HIPCHK(dsF.alloc(sizeof(double) * (size_t)E * Evm));
    HIPCHK(dlam.alloc(sizeof(double) * Evm)); HIPCHK(dpost.alloc(sizeof(double) * (size_t)J * n * Evm));
  }
  if (joint) {
    HIPCHK(dM.alloc(sizeof(double) * (size_t)Nn * n * Evm)); HIPCHK(dsM.alloc(sizeof(double) * (size_t)Nn * Evm));
    HIPCHK(dptr.alloc(sizeof(uint32_t) * (size_t)E * Evm)); HIPCHK(dx.alloc((size_t)NT * Evm));
    HIPCHK(djl.alloc(sizeof(double) * Evm));
  }
  std::vector<double> posth(marg ? (size_t)J * n * Evm : 0), jlh(joint ? Evm : 0);
  std::vector<uint8_t> xh(joint ? (size_t)NT * Evm : 0);
  const std::vector<double>& llh = ln.llh;
  const phm::UpStep* up = ln.dup.as<phm::UpStep>();

  for (int64_t c0 = 0; c0 < count; c0 += pl.Kc_max) {
    const int64_t Kc = std::min<int64_t>(pl.Kc_max, count - c0);
    st = ln.load_models(first + c0, Kc);
    if (st) return st;
    const int Kp = ln.Kp;
    const int64_t m0 = ln.m0;                            // global index of this chunk's first model
    phm::ScParams sp = {};
    phm::LlParams& p = sp.ll;
    p = ln.params();
    sp.n_edge = E; sp.root = T + in.sched.root;
    if (marg) {
      sp.O = dO.as<double>(); sp.sO = dsO.as<double>(); sp.F = dF.as<double>(); sp.sF = dsF.as<double>(); sp.lam = dlam.as<double>();
    }
    phm::AnParams ap = {};
    ap.root = sp.root;
    if (marg) { ap.O = dO.as<double>(); ap.sel = dsel.as<int32_t>(); ap.post = dpost.as<double>(); }
    if (joint) {
      ap.M = dM.as<double>(); ap.sM = dsM.as<double>(); ap.ptr = dptr.as<uint32_t>(); ap.x = dx.as<uint8_t>();
      ap.jlogp = djl.as<double>();
    }
    HIPCHK(tm.start());
    st = ln.expm(p);
    if (st) return st;
    HIPCHK(tm.stop());
    HIPCHK(tm.add_to(kernel_ms));

    for (int64_t s0 = 0; s0 < S_eval; s0 += pl.Sc_max) {
      const int64_t Sc = std::min<int64_t>(pl.Sc_max, S_eval - s0);
      p.n_sites = (int)Sc;
      const size_t Ev = (size_t)Sc * Kp;
      st = ln.stage_tips(s0, Sc);
      if (st) return st;
      ap.ll = p;
      HIPCHK(tm.start());
      st = ln.passes(p);
      if (st) return st;
      if (marg) {
        HIPCHK(phm::launch_sc_root(sp, nullptr));
        for (size_t l = 0; l + 1 < an.down_off.size(); ++l)
          HIPCHK(phm::launch_sc_down(sp, ddown.as<phm::ExDown>() + an.down_off[l], an.down_off[l + 1] - an.down_off[l], nullptr));
        for (int j0 = 0; j0 < J; j0 += step_max) HIPCHK(phm::launch_an_post(ap, j0, std::min(step_max, J - j0), nullptr));
      }
      if (joint) {
        for (size_t l = 0; l + 1 < in.up_off.size(); ++l)
          for (int k0 = in.up_off[l]; k0 < in.up_off[l + 1]; k0 += step_max)
            HIPCHK(phm::launch_an_up(ap, up + k0, std::min(step_max, in.up_off[l + 1] - k0), nullptr));
        HIPCHK(phm::launch_an_root(ap, nullptr));
        for (size_t l = 0; l + 1 < an.down_off.size(); ++l)
          for (int k0 = an.down_off[l]; k0 < an.down_off[l + 1]; k0 += step_max)
            HIPCHK(phm::launch_an_trace(ap, ddown.as<phm::ExDown>() + k0, std::min(step_max, an.down_off[l + 1] - k0), nullptr));
      }
      HIPCHK(tm.stop());
      st = ln.fetch_ll(Sc);
      if (st) return st;
      if (marg) HIPCHK(hipMemcpy(posth.data(), dpost.p, sizeof(double) * (size_t)J * n * Ev, hipMemcpyDeviceToHost));
      if (joint) {
        HIPCHK(hipMemcpy(xh.data(), dx.p, (size_t)NT * Ev, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(jlh.data(), djl.p, sizeof(double) * Ev, hipMemcpyDeviceToHost));
      }
      HIPCHK(tm.add_to(kernel_ms));
      // the output stage: [row][state][Ev] -> [evaluation][node][state]; an impossible evaluation gets NaN / 0 / -inf
      for (int64_t s = 0; s < Sc; ++s) {
        if (marg)                                        // eight models at a time: one cache line of a row feeds eight output rows
          for (int64_t k0 = 0; k0 < Kc; k0 += 8) {
            const int kn = (int)std::min<int64_t>(8, Kc - k0);
            double* out[8];
            bool possible[8];
            for (int k = 0; k < kn; ++k) {
              out[k] = node_post + (size_t)ll_eval_of(in, s0 + s, m0 + k0 + k) * J * n;
              possible[k] = std::isfinite(llh[(size_t)s * Kp + k0 + k]);
            }
            const double* src = posth.data() + (size_t)s * Kp + k0;
            const size_t rows = (size_t)J * n;
            if (kn == 8) {                               // a full group: a fixed trip count, so that the eight stores are unrolled
              for (size_t c = 0; c < rows; ++c)
                for (int k = 0; k < 8; ++k) out[k][c] = possible[k] ? src[c * Ev + k] : nan;
            } else {                                     // the ragged last group of a chunk
              for (size_t c = 0; c < rows; ++c)
                for (int k = 0; k < kn; ++k) out[k][c] = possible[k] ? src[c * Ev + k] : nan;
            }
          }
        for (int64_t k = 0; k < Kc; ++k) {
          const int64_t ev = ll_eval_of(in, s0 + s, m0 + k);
          const size_t at = (size_t)s * Kp + k;
          const double ll = llh[at];
          loglik[ev] = ll;
          const bool possible = std::isfinite(ll);
          if (joint) {
            int32_t* out = joint_states + (size_t)ev * J;
            for (int j = 0; j < J; ++j) out[j] = possible ? (int32_t)xh[(size_t)an.sel[j] * Ev + at] + 1 : 0;
            if (joint_logp) joint_logp[ev] = possible ? jlh[at] : ninf;
          }
        }
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
int32_t phm_ancestral_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                             int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const int32_t* node_sel,
                             int32_t n_sel, const phm_options* opt, double* loglik, double* node_post, int32_t* joint_states,
                             double* joint_logp) {
  return an_entry(AN_FN, 2, phm::LL_LANE_MAX, "more than 8 states are not supported", an_device, x, n_states, n_models, Q, pid, n_pid,
                  observe, site_of_model, node_sel, n_sel, opt, loglik, node_post, joint_states, joint_logp);
}

}  // extern "C"
