// phm_ancestral_wide_api.cpp -- C-ABI of the ancestral states for many rate matrices at 9..64 states
// (phm_ancestral_models_wide): phm_ancestral_models' arguments, validation (an_entry of phm_ancestral_host.h:
// ll_validate, then the node selection) and outputs.  Per device and per chunk of models P_k(t_b) by one launch_expm_pade per model (section 13's kernel and
// ex_squarings' counts, each model with its own error word), then per chunk of sites the tips / up / root launches followed by
// what was asked for: the down pass with the node posteriors, and the max-product up pass, root and traceback.  The output stage
// is on the HOST.  An evaluation is independent of every other one and P_k of every other model, so neither the chunks nor the
// shards change an output bit.
#include "phm_ancestral_wide.h"
#include "phm_exp.h"
#include "phm_ancestral_host.h"

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
  const int n = in.n, E = in.E, NT = in.NT, T = in.T, Nn = in.Nn, J = an.J, NP = phm::aw_lanes(in.n);
  const bool marg = node_post != nullptr, joint = joint_states != nullptr;
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.sites_per_model();
  const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  KernelTimer tm;
  double kernel_ms = 0.0, ms = 0.0;
  DevBuf dt, dobs, dup, ddown, dsel;
  HIPCHK(upload(dt, in.edge_length)); HIPCHK(upload(dobs, in.obs)); HIPCHK(upload(dup, in.up));
  HIPCHK(upload(ddown, an.down));
  if (marg) HIPCHK(upload(dsel, an.sel));

  // Chunks by free HBM.  Once: the Pade workspace of one model (the models' launches follow each other on the stream).  Per
  // model: Q, pid, the squaring counts, the error word, P and, when paired, its tips.  Per evaluation: L, sL and ll; for the
  // marginals O, sO and the selected posterior rows; for the joint reconstruction M, sM, a pointer byte per (edge, parent state),
  // a state byte per node and the log of the maximum.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const size_t work_b = sizeof(double) * 5 * nn * (size_t)E;
  const size_t budget = free_b / 2 > work_b ? free_b / 2 - work_b : 0;
  const size_t per_model = sizeof(double) * ((size_t)E * nn + nn + n) + sizeof(int32_t) * (size_t)E + sizeof(uint32_t) + (in.paired ? (size_t)T : 0);
  size_t per_eval = (sizeof(double) * NP + sizeof(int32_t)) * (size_t)NT + sizeof(double);
  if (marg) per_eval += (sizeof(double) * NP + sizeof(int32_t)) * (size_t)NT + sizeof(double) * (size_t)J * n;
  if (joint) per_eval += (sizeof(double) * NP + sizeof(int32_t)) * (size_t)Nn + (size_t)E * NP + (size_t)NT + sizeof(double);
  int64_t Sc_max = std::min<int64_t>(S_eval, phm::AW_GRID_MAX);
  int64_t Kc_max = (int64_t)(budget / (per_model + per_eval * (size_t)Sc_max));
  if (Kc_max < 1) {
    Kc_max = 1;
    Sc_max = std::max<int64_t>(1, std::min<int64_t>(Sc_max, budget > per_model ? (int64_t)((budget - per_model) / per_eval) : 1));
  }
  int step_max = phm::AW_GRID_MAX;                       // level steps (and selected rows) of one launch
  const int chunk = g_phm_debug.expect_chunk;
  if (chunk > 0) {
    Kc_max = std::min<int64_t>(Kc_max, chunk);
    Sc_max = std::min<int64_t>(Sc_max, chunk);
    step_max = std::min(step_max, chunk);
  }
  Kc_max = std::min<int64_t>({Kc_max, count, (int64_t)phm::AW_GRID_MAX});
  const size_t Km = (size_t)Kc_max, Evm = Km * (size_t)Sc_max;

  DevBuf dQ, dpid, dsq, dP, dwork, dbad, dL, dsL, dll, dtips, dO, dsO, dpost, dM, dsM, dptr, dx, djl;
  HIPCHK(dQ.alloc(sizeof(double) * nn * Km)); HIPCHK(dpid.alloc(sizeof(double) * n * Km));
  HIPCHK(dsq.alloc(sizeof(int32_t) * (size_t)E * Km)); HIPCHK(dbad.alloc(sizeof(uint32_t) * Km));
  HIPCHK(dP.alloc(sizeof(double) * (size_t)E * nn * Km)); HIPCHK(dwork.alloc(work_b));
  HIPCHK(dL.alloc(sizeof(double) * (size_t)NT * NP * Evm)); HIPCHK(dsL.alloc(sizeof(int32_t) * (size_t)NT * Evm));
  HIPCHK(dll.alloc(sizeof(double) * Evm));
  HIPCHK(dtips.alloc(in.paired ? (size_t)T * Km : (size_t)T * (size_t)Sc_max));
  if (marg) {
    HIPCHK(dO.alloc(sizeof(double) * (size_t)NT * NP * Evm)); HIPCHK(dsO.alloc(sizeof(int32_t) * (size_t)NT * Evm));
    HIPCHK(dpost.alloc(sizeof(double) * (size_t)J * n * Evm));
  }
  if (joint) {
    HIPCHK(dM.alloc(sizeof(double) * (size_t)Nn * NP * Evm)); HIPCHK(dsM.alloc(sizeof(int32_t) * (size_t)Nn * Evm));
    HIPCHK(dptr.alloc((size_t)E * NP * Evm)); HIPCHK(dx.alloc((size_t)NT * Evm));
    HIPCHK(djl.alloc(sizeof(double) * Evm));
  }
  std::vector<double> llh(Evm), posth(marg ? (size_t)J * n * Evm : 0), jlh(joint ? Evm : 0);
  std::vector<uint8_t> tips_h(in.paired ? (size_t)T * Km : (size_t)T * (size_t)Sc_max), xh(joint ? (size_t)NT * Evm : 0);
  std::vector<int32_t> sqh((size_t)E * Km);
  std::vector<uint32_t> badh(Km);

  for (int64_t c0 = 0; c0 < count; c0 += Kc_max) {
    const int64_t Kc = std::min<int64_t>(Kc_max, count - c0);
    const int64_t m0 = first + c0;                       // global index of this chunk's first model
    for (int64_t k = 0; k < Kc; ++k)
      for (int b = 0; b < E; ++b) sqh[(size_t)k * E + b] = ex_squarings(in.Qr.data() + (size_t)(m0 + k) * nn, n, in.edge_length[b]);
    HIPCHK(hipMemcpy(dQ.p, in.Qr.data() + (size_t)m0 * nn, sizeof(double) * nn * Kc, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dpid.p, in.pid.data() + (size_t)m0 * n, sizeof(double) * n * Kc, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsq.p, sqh.data(), sizeof(int32_t) * (size_t)E * Kc, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dbad.p, 0, sizeof(uint32_t) * Kc));
    HIPCHK(tm.start());
    for (int64_t k = 0; k < Kc; ++k)
      HIPCHK(phm::launch_expm_pade(n, dQ.as<double>() + (size_t)k * nn, dt.as<double>(), dsq.as<int32_t>() + (size_t)k * E, E,
                                   dwork.as<double>(), dP.as<double>() + (size_t)k * E * nn, dbad.as<uint32_t>() + k, nullptr));
    HIPCHK(tm.stop());
    HIPCHK(hipMemcpy(badh.data(), dbad.p, sizeof(uint32_t) * Kc, hipMemcpyDeviceToHost));
    HIPCHK(tm.elapsed(ms));
    kernel_ms += ms;

    phm::AwParams p = {};
    p.n = n; p.NP = NP; p.n_tips = T; p.n_edge = E; p.root = T + in.sched.root; p.Kc = (int)Kc;
    p.tip_model = in.paired ? 1 : 0; p.tip_site = in.paired ? 0 : 1;
    p.P = dP.as<double>(); p.pid = dpid.as<double>(); p.tips = dtips.as<uint8_t>(); p.obs = dobs.as<int32_t>();
    p.L = dL.as<double>(); p.sL = dsL.as<int32_t>(); p.ll = dll.as<double>();
    if (marg) {
      p.O = dO.as<double>(); p.sO = dsO.as<int32_t>(); p.sel = dsel.as<int32_t>(); p.J = J; p.post = dpost.as<double>();
    }
    if (joint) {
      p.M = dM.as<double>(); p.sM = dsM.as<int32_t>(); p.ptr = dptr.as<uint8_t>(); p.x = dx.as<uint8_t>(); p.jlogp = djl.as<double>();
    }

    for (int64_t s0 = 0; s0 < S_eval; s0 += Sc_max) {
      const int64_t Sc = std::min<int64_t>(Sc_max, S_eval - s0);
      p.Sc = (int)Sc;
      const size_t Ev = (size_t)Sc * Kc;
      if (in.paired) {                                   // [model][tip]
        for (int64_t k = 0; k < Kc; ++k) {
          const int32_t* y = in.tips_of(in.site_of_model[m0 + k]);
          for (int t = 0; t < T; ++t) tips_h[(size_t)k * T + t] = (uint8_t)y[t];
        }
        HIPCHK(hipMemcpy(dtips.p, tips_h.data(), (size_t)T * Kc, hipMemcpyHostToDevice));
      } else {
        ll_stage_tips_sites(in, s0, Sc, tips_h);         // [site][tip]
        HIPCHK(hipMemcpy(dtips.p, tips_h.data(), (size_t)T * Sc, hipMemcpyHostToDevice));
      }
      const phm::UpStep* up = dup.as<phm::UpStep>();
      const phm::ExDown* down = ddown.as<phm::ExDown>();
      HIPCHK(tm.start());
      HIPCHK(phm::launch_aw_tips(p, nullptr));
      for (size_t l = 0; l + 1 < in.up_off.size(); ++l)
        for (int k0 = in.up_off[l]; k0 < in.up_off[l + 1]; k0 += step_max)
          HIPCHK(phm::launch_aw_up(p, up + k0, std::min(step_max, in.up_off[l + 1] - k0), false, nullptr));
      HIPCHK(phm::launch_aw_root(p, nullptr));
      if (marg) {
        for (size_t l = 0; l + 1 < an.down_off.size(); ++l)
          for (int k0 = an.down_off[l]; k0 < an.down_off[l + 1]; k0 += step_max)
            HIPCHK(phm::launch_aw_down(p, down + k0, std::min(step_max, an.down_off[l + 1] - k0), nullptr));
        for (int j0 = 0; j0 < J; j0 += step_max) HIPCHK(phm::launch_aw_post(p, j0, std::min(step_max, J - j0), nullptr));
      }
      if (joint) {
        for (size_t l = 0; l + 1 < in.up_off.size(); ++l)
          for (int k0 = in.up_off[l]; k0 < in.up_off[l + 1]; k0 += step_max)
            HIPCHK(phm::launch_aw_up(p, up + k0, std::min(step_max, in.up_off[l + 1] - k0), true, nullptr));
        HIPCHK(phm::launch_aw_jroot(p, nullptr));
        for (size_t l = 0; l + 1 < an.down_off.size(); ++l)
          for (int k0 = an.down_off[l]; k0 < an.down_off[l + 1]; k0 += step_max)
            HIPCHK(phm::launch_aw_trace(p, down + k0, std::min(step_max, an.down_off[l + 1] - k0), nullptr));
      }
      HIPCHK(tm.stop());
      HIPCHK(hipMemcpy(llh.data(), dll.p, sizeof(double) * Ev, hipMemcpyDeviceToHost));
      if (marg) HIPCHK(hipMemcpy(posth.data(), dpost.p, sizeof(double) * (size_t)J * n * Ev, hipMemcpyDeviceToHost));
      if (joint) {
        HIPCHK(hipMemcpy(xh.data(), dx.p, (size_t)NT * Ev, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(jlh.data(), djl.p, sizeof(double) * Ev, hipMemcpyDeviceToHost));
      }
      HIPCHK(tm.elapsed(ms));
      kernel_ms += ms;
      // the output stage; an impossible evaluation (or a model whose Pade met a zero pivot) gets -inf / NaN / 0 / -inf
      const size_t row = (size_t)J * n;
      for (int64_t k = 0; k < Kc; ++k)
        for (int64_t s = 0; s < Sc; ++s) {
          const size_t at = (size_t)k * Sc + s;
          const int64_t ev = ll_eval_of(in, s0 + s, m0 + k);
          const bool possible = !badh[k] && std::isfinite(llh[at]);
          loglik[ev] = possible ? llh[at] : ninf;
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
