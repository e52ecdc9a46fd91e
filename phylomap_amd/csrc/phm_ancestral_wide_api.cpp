// phm_ancestral_wide_api.cpp -- C-ABI of the ancestral states for many rate matrices at 9..64 states
// (phm_ancestral_models_wide): phm_ancestral_models' arguments, validation (an_entry of phm_ancestral_host.h:
// ll_validate, then the node selection) and outputs.  The chunk plan, the device state, P_k(t_b) of a chunk of models and the
// tips / up / root launches of a chunk of sites are AwLanes' (phm_ancestral_wide_host.h, section 23a); this driver adds what was
// asked for: the down pass with the node posteriors, and the max-product up pass, root and traceback.  The output stage
// is on the HOST.  An evaluation is independent of every other one and P_k of every other model, so neither the chunks nor the
// shards change an output bit.
#include "phm_ancestral_host.h"
#include "phm_ancestral_wide_host.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;

const std::string AW_FN = "phm_ancestral_models_wide: ";

// models [first, first + count) on one device
int32_t aw_device(const AnInput& an, int32_t device, int64_t first, int64_t count, double* loglik, double* node_post,
                  int32_t* joint_states, double* joint_logp) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = an.ll;
  const int n = in.n, E = in.E, NT = in.NT, Nn = in.Nn, J = an.J, NP = phm::aw_lanes(in.n);
  const bool marg = node_post != nullptr, joint = joint_states != nullptr;
  const int64_t S_eval = in.sites_per_model();
  const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  KernelTimer tm;
  double kernel_ms = 0.0;
  AwLanes ln(in);
  DevBuf ddown, dsel;
  st = ln.upload_tree();
  if (st) return st;
  HIPCHK(upload(ddown, an.down));
  if (marg) HIPCHK(upload(dsel, an.sel));

  // On top of section 23's footprint, per evaluation: for the marginals O, sO and the selected posterior rows; for the joint
  // reconstruction M, sM, a pointer byte per (edge, parent state), a state byte per node and the log of the maximum.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  size_t per_eval = 0;
  if (marg) per_eval += (sizeof(double) * NP + sizeof(int32_t)) * (size_t)NT + sizeof(double) * (size_t)J * n;
  if (joint) per_eval += (sizeof(double) * NP + sizeof(int32_t)) * (size_t)Nn + (size_t)E * NP + (size_t)NT + sizeof(double);
  const AwPlan pl = aw_plan(free_b, in, count, g_phm_debug.expect_chunk, 0, 0, per_eval);
  const int step_max = pl.step_max;
  const size_t Evm = (size_t)pl.Kc_max * (size_t)pl.Sc_max;

  DevBuf dO, dsO, dpost, dM, dsM, dptr, dx, djl;
  st = ln.alloc(pl);
  if (st) return st;
  if (marg) {
    HIPCHK(dO.alloc(sizeof(double) * (size_t)NT * NP * Evm)); HIPCHK(dsO.alloc(sizeof(int32_t) * (size_t)NT * Evm));
    HIPCHK(dpost.alloc(sizeof(double) * (size_t)J * n * Evm));
  }
  if (joint) {
    HIPCHK(dM.alloc(sizeof(double) * (size_t)Nn * NP * Evm)); HIPCHK(dsM.alloc(sizeof(int32_t) * (size_t)Nn * Evm));
    HIPCHK(dptr.alloc((size_t)E * NP * Evm)); HIPCHK(dx.alloc((size_t)NT * Evm));
    HIPCHK(djl.alloc(sizeof(double) * Evm));
  }
  std::vector<double> posth(marg ? (size_t)J * n * Evm : 0), jlh(joint ? Evm : 0);
  std::vector<uint8_t> xh(joint ? (size_t)NT * Evm : 0);

  for (int64_t c0 = 0; c0 < count; c0 += pl.Kc_max) {
    const int64_t Kc = std::min<int64_t>(pl.Kc_max, count - c0);
    const int64_t m0 = first + c0;                       // global index of this chunk's first model
    st = ln.load_models(m0, Kc);
    if (st) return st;
    HIPCHK(tm.start());
    st = ln.expm();
    if (st) return st;
    HIPCHK(tm.stop());
    st = ln.fetch_bad();
    if (st) return st;
    HIPCHK(tm.add_to(kernel_ms));

    phm::AwParams p = ln.params();
    if (marg) {
      p.O = dO.as<double>(); p.sO = dsO.as<int32_t>(); p.sel = dsel.as<int32_t>(); p.J = J; p.post = dpost.as<double>();
    }
    if (joint) {
      p.M = dM.as<double>(); p.sM = dsM.as<int32_t>(); p.ptr = dptr.as<uint8_t>(); p.x = dx.as<uint8_t>(); p.jlogp = djl.as<double>();
    }

    for (int64_t s0 = 0; s0 < S_eval; s0 += pl.Sc_max) {
      const int64_t Sc = std::min<int64_t>(pl.Sc_max, S_eval - s0);
      p.Sc = (int)Sc;
      const size_t Ev = (size_t)Sc * Kc;
      st = ln.stage_tips(s0, Sc);
      if (st) return st;
      const phm::UpStep* up = ln.dup.as<phm::UpStep>();
      const phm::ExDown* down = ddown.as<phm::ExDown>();
      HIPCHK(tm.start());
      st = ln.passes(p);
      if (st) return st;
      if (marg) {
        st = aw_level_steps(an.down_off, step_max, [&](int k0, int cnt) { return phm::launch_aw_down(p, down + k0, cnt, nullptr); });
        if (st) return st;
        for (int j0 = 0; j0 < J; j0 += step_max) HIPCHK(phm::launch_aw_post(p, j0, std::min(step_max, J - j0), nullptr));
      }
      if (joint) {
        st = aw_level_steps(in.up_off, step_max, [&](int k0, int cnt) { return phm::launch_aw_up(p, up + k0, cnt, true, nullptr); });
        if (st) return st;
        HIPCHK(phm::launch_aw_jroot(p, nullptr));
        st = aw_level_steps(an.down_off, step_max, [&](int k0, int cnt) { return phm::launch_aw_trace(p, down + k0, cnt, nullptr); });
        if (st) return st;
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
      // the output stage; an impossible evaluation (or a model whose Pade met a zero pivot) gets -inf / NaN / 0 / -inf
      const size_t row = (size_t)J * n;
      for (int64_t k = 0; k < Kc; ++k)
        for (int64_t s = 0; s < Sc; ++s) {
          const size_t at = (size_t)k * Sc + s;
          const int64_t ev = ll_eval_of(in, s0 + s, m0 + k);
          const bool possible = ln.possible(k, at);
          loglik[ev] = possible ? ln.llh[at] : ninf;
          if (marg) {
            double* out = node_post + (size_t)ev * row;
            if (possible) std::copy(posth.begin() + at * row, posth.begin() + (at + 1) * row, out);
            else std::fill(out, out + row, nan);
          }
          if (joint) {
            int32_t* out = joint_states + (size_t)ev * J;
            for (int j = 0; j < J; ++j) out[j] = possible ? (int32_t)xh[(size_t)an.sel[j] * Ev + at] + 1 : 0;
            if (joint_logp) joint_logp[ev] = possible ? jlh[at] : ninf;
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
int32_t phm_ancestral_models_wide(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                  int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const int32_t* node_sel,
                                  int32_t n_sel, const phm_options* opt, double* loglik, double* node_post, int32_t* joint_states,
                                  double* joint_logp) {
  return an_entry(AW_FN, phm::AW_MIN_STATES, phm::EX_MAX_STATES, "9..64 states only: 2..8 states go to phm_ancestral_models", aw_device, x,
                  n_states, n_models, Q, pid, n_pid, observe, site_of_model, node_sel, n_sel, opt, loglik, node_post, joint_states,
                  joint_logp);
}

}  // extern "C"
