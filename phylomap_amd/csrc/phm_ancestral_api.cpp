// phm_ancestral_api.cpp -- C-ABI of the ancestral states for many rate matrices in one call (phm_ancestral_models, DESIGN.md
// section 21): phm_loglik_models' validation (ll_validate) and the checks of the node selection, then per device and per chunk of
// models P_k(t_b) once and, per chunk of sites, section 17's tips / up / root launches followed by what was asked for: section
// 18's root and down launches with the node-posterior kernel, and the max-product up pass, root and traceback of
// phm_ancestral.hip.  The output stage is on the HOST: the selected posterior rows ([selected][state][Ev]) and the state bytes
// ([node row][Ev]) are copied back and written into the caller's [evaluation][node][state] layout here.
#include "phm_ancestral.h"
#include "phm_loglik_host.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;

const std::string AN_FN = "phm_ancestral_models: ";

struct AnInput {
  LlInput ll;
  int64_t n_eval = 0;                                   // S * K (cross) or K (paired)
  int J = 0;                                            // reported nodes
  std::vector<int32_t> sel;                             // their node rows (node id - 1), in the caller's order
  std::vector<phm::ExDown> down;                        // grouped by the depth of the parent
  std::vector<int32_t> down_off;
};

inline int64_t eval_of(const LlInput& in, int64_t site, int64_t model) { return in.paired ? model : site + (int64_t)in.S * model; }

int32_t an_prepare(AnInput& an, const int32_t* node_sel, int32_t n_sel) {
  LlInput& in = an.ll;
  if (in.n > phm::LL_LANE_MAX) return fail(PHM_ERR_UNSUPPORTED, AN_FN + "more than 8 states are not supported");
  if ((int64_t)in.S * in.K > (int64_t)INT32_MAX) return fail(PHM_ERR_BAD_INPUT, AN_FN + "sites * models must fit in 31 bits");
  an.n_eval = in.paired ? in.K : (int64_t)in.S * in.K;
  if (n_sel == 0) {
    an.sel.resize(in.NT);
    for (int r = 0; r < in.NT; ++r) an.sel[r] = r;
  } else {
    an.sel.resize(n_sel);
    for (int j = 0; j < n_sel; ++j) {
      if (node_sel[j] < 1 || node_sel[j] > in.NT)
        return fail(PHM_ERR_BAD_INPUT, AN_FN + "node_sel[" + std::to_string(j) + "] must be in 1.." + std::to_string(in.NT));
      an.sel[j] = node_sel[j] - 1;
    }
  }
  an.J = (int)an.sel.size();
  const phm::Schedule& s = in.sched;
  const int T = in.T;
  std::vector<int32_t> order, up_of(s.n_node, -1);
  for (int k = 0; k < s.n_node; ++k) up_of[s.up[k].parent] = k;
  auto row_of = [T](int32_t c) { return c >= 0 ? T + c : ~c; };
  phm::depth_levels(s, order, an.down_off);
  for (int32_t k : order) {
    const phm::DownStep& d = s.down[k];
    const phm::UpStep& u = s.up[up_of[d.parent]];
    const int side = u.edge[0] == d.edge ? 1 : 0;                  // the sibling branch
    phm::ExDown x = {};
    x.edge = d.edge; x.parent = T + d.parent; x.child = row_of(d.child);
    x.sib_edge = u.edge[side]; x.sib_child = row_of(u.child[side]);
    an.down.push_back(x);
  }
  return PHM_OK;
}

// models [first, first + count) on one device, models across the lanes
int32_t an_device(const AnInput& an, int32_t device, int64_t first, int64_t count, double* loglik, double* node_post,
                  int32_t* joint_states, double* joint_logp) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = an.ll;
  const int n = in.n, E = in.E, NT = in.NT, T = in.T, Nn = in.Nn, J = an.J;
  const bool marg = node_post != nullptr, joint = joint_states != nullptr;
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.paired ? 1 : in.S;           // sites per model
  const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  KernelTimer tm;
  double kernel_ms = 0.0, ms = 0.0;
  DevBuf dt, dobs, dup, ddown, dsel;
  HIPCHK(upload(dt, in.edge_length)); HIPCHK(upload(dobs, in.obs)); HIPCHK(upload(dup, in.up));
  HIPCHK(upload(ddown, an.down));
  if (marg) HIPCHK(upload(dsel, an.sel));

  // Chunks by free HBM: section 17's footprint (per model Q, pid and P; per evaluation L, sL, ll and a tip byte per tip when
  // paired); for the marginals O and F with their exponents, lam and the selected posterior rows; for the joint reconstruction
  // M, sM, a pointer word per edge, a state byte per node and the log of the maximum.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const bool ws = n > phm::LL_REG_MAX;
  const size_t budget = free_b / 2 > (ws ? LL_WORK : 0) ? free_b / 2 - (ws ? LL_WORK : 0) : 0;
  const size_t per_model = sizeof(double) * ((size_t)E * nn + nn + n) + sizeof(uint32_t);
  size_t per_eval = sizeof(double) * ((size_t)NT * (n + 1) + 1) + (in.paired ? (size_t)T : 0);
  if (marg) per_eval += sizeof(double) * ((size_t)NT * (n + 1) + (size_t)E * (n + 1) + 1 + (size_t)J * n);
  if (joint) per_eval += sizeof(double) * ((size_t)Nn * (n + 1) + 1) + sizeof(uint32_t) * (size_t)E + (size_t)NT;
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
  int step_max = 65535;                                  // level steps (and selected rows) of one launch
  if (chunk > 0) { ne_max = std::min(ne_max, chunk); step_max = std::min(step_max, chunk); }

  DevBuf dQ, dpid, dP, dwork, dbad, dL, dsL, dll, dtips, dO, dsO, dF, dsF, dlam, dpost, dM, dsM, dptr, dx, djl;
  HIPCHK(dQ.alloc(sizeof(double) * nn * Kpm)); HIPCHK(dpid.alloc(sizeof(double) * n * Kpm));
  HIPCHK(dP.alloc(sizeof(double) * (size_t)E * nn * Kpm)); HIPCHK(dbad.alloc(sizeof(uint32_t) * Kpm));
  if (ws) HIPCHK(dwork.alloc(sizeof(double) * 4 * nn * Kpm * (size_t)ne_max));
  HIPCHK(dL.alloc(sizeof(double) * (size_t)NT * n * Evm)); HIPCHK(dsL.alloc(sizeof(double) * (size_t)NT * Evm));
  HIPCHK(dll.alloc(sizeof(double) * Evm));
  HIPCHK(dtips.alloc(in.paired ? (size_t)T * Kpm : (size_t)T * (size_t)Sc_max));
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
  std::vector<double> Qh(nn * Kpm), pidh((size_t)n * Kpm), llh(Evm), posth(marg ? (size_t)J * n * Evm : 0), jlh(joint ? Evm : 0);
  std::vector<uint8_t> tips_h(in.paired ? (size_t)T * Kpm : (size_t)T * (size_t)Sc_max), xh(joint ? (size_t)NT * Evm : 0);

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
    phm::ScParams sp = {};
    phm::LlParams& p = sp.ll;
    p.n = n; p.n_tips = T; p.Kp = Kp; p.Kc = (int)Kc; p.paired = in.paired ? 1 : 0;
    p.Q = dQ.as<double>(); p.pid = dpid.as<double>(); p.t = dt.as<double>(); p.P = dP.as<double>();
    p.work = ws ? dwork.as<double>() : nullptr; p.bad = dbad.as<uint32_t>(); p.tips = dtips.as<uint8_t>();
    p.obs = dobs.as<int32_t>(); p.L = dL.as<double>(); p.sL = dsL.as<double>(); p.ll = dll.as<double>();
    p.n_sites = 1;
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
    for (int e0 = 0; e0 < E; e0 += ne_max) HIPCHK(phm::launch_ll_expm(p, e0, std::min(ne_max, E - e0), nullptr));
    HIPCHK(tm.stop());
    HIPCHK(tm.elapsed(ms));
    kernel_ms += ms;

    for (int64_t s0 = 0; s0 < S_eval; s0 += Sc_max) {
      const int64_t Sc = std::min<int64_t>(Sc_max, S_eval - s0);
      p.n_sites = (int)Sc;
      const size_t Ev = (size_t)Sc * Kp;
      if (in.paired) {                                   // [tip][Kp]: lane k reads the tips of its own site
        std::fill(tips_h.begin(), tips_h.end(), (uint8_t)0);
        for (int64_t k = 0; k < Kc; ++k) {
          const int32_t* y = in.tips_of(in.site_of_model[m0 + k]);
          for (int t = 0; t < T; ++t) tips_h[(size_t)t * Kp + k] = (uint8_t)y[t];
        }
        HIPCHK(hipMemcpy(dtips.p, tips_h.data(), (size_t)T * Kp, hipMemcpyHostToDevice));
      } else {                                           // [site][tip]
        for (int64_t s = 0; s < Sc; ++s) {
          const int32_t* y = in.tips_of(s0 + s);
          for (int t = 0; t < T; ++t) tips_h[(size_t)s * T + t] = (uint8_t)y[t];
        }
        HIPCHK(hipMemcpy(dtips.p, tips_h.data(), (size_t)T * Sc, hipMemcpyHostToDevice));
      }
      ap.ll = p;
      HIPCHK(tm.start());
      HIPCHK(phm::launch_ll_tips(p, nullptr));
      for (size_t l = 0; l + 1 < in.up_off.size(); ++l)
        HIPCHK(phm::launch_ll_up(p, dup.as<phm::UpStep>() + in.up_off[l], in.up_off[l + 1] - in.up_off[l], nullptr));
      HIPCHK(phm::launch_ll_root(p, sp.root, nullptr));
      if (marg) {
        HIPCHK(phm::launch_sc_root(sp, nullptr));
        for (size_t l = 0; l + 1 < an.down_off.size(); ++l)
          HIPCHK(phm::launch_sc_down(sp, ddown.as<phm::ExDown>() + an.down_off[l], an.down_off[l + 1] - an.down_off[l], nullptr));
        for (int j0 = 0; j0 < J; j0 += step_max) HIPCHK(phm::launch_an_post(ap, j0, std::min(step_max, J - j0), nullptr));
      }
      if (joint) {
        for (size_t l = 0; l + 1 < in.up_off.size(); ++l)
          for (int k0 = in.up_off[l]; k0 < in.up_off[l + 1]; k0 += step_max)
            HIPCHK(phm::launch_an_up(ap, dup.as<phm::UpStep>() + k0, std::min(step_max, in.up_off[l + 1] - k0), nullptr));
        HIPCHK(phm::launch_an_root(ap, nullptr));
        for (size_t l = 0; l + 1 < an.down_off.size(); ++l)
          for (int k0 = an.down_off[l]; k0 < an.down_off[l + 1]; k0 += step_max)
            HIPCHK(phm::launch_an_trace(ap, ddown.as<phm::ExDown>() + k0, std::min(step_max, an.down_off[l + 1] - k0), nullptr));
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
      // the output stage: [row][state][Ev] -> [evaluation][node][state]; an impossible evaluation gets NaN / 0 / -inf
      for (int64_t s = 0; s < Sc; ++s) {
        if (marg)                                        // eight models at a time: one cache line of a row feeds eight output rows
          for (int64_t k0 = 0; k0 < Kc; k0 += 8) {
            const int kn = (int)std::min<int64_t>(8, Kc - k0);
            double* out[8];
            bool possible[8];
            for (int k = 0; k < kn; ++k) {
              out[k] = node_post + (size_t)eval_of(in, s0 + s, m0 + k0 + k) * J * n;
              possible[k] = std::isfinite(llh[(size_t)s * Kp + k0 + k]);
            }
            for (size_t c = 0; c < (size_t)J * n; ++c) {
              const double* row = posth.data() + c * Ev + (size_t)s * Kp + k0;
              for (int k = 0; k < kn; ++k) out[k][c] = possible[k] ? row[k] : nan;
            }
          }
        for (int64_t k = 0; k < Kc; ++k) {
          const int64_t ev = eval_of(in, s0 + s, m0 + k);
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
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid || !loglik)
    return fail(PHM_ERR_BAD_INPUT, AN_FN + "NULL argument (x, Q, pid and loglik are required)");
  if (!node_post && !joint_states) return fail(PHM_ERR_BAD_INPUT, AN_FN + "node_post and joint_states are both NULL: nothing to compute");
  if (joint_logp && !joint_states) return fail(PHM_ERR_BAD_INPUT, AN_FN + "joint_logp needs joint_states");
  if (n_sel < 0) return fail(PHM_ERR_BAD_INPUT, AN_FN + "n_sel must be >= 0");
  if (n_sel > 0 && !node_sel) return fail(PHM_ERR_BAD_INPUT, AN_FN + "node_sel is NULL with n_sel > 0");
  AnInput an;
  int32_t st = ll_validate(AN_FN, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, o, an.ll);
  if (st) return st;
  st = an_prepare(an, node_sel, n_sel);
  if (st) return st;
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, an.ll.K, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) {
    return an_device(an, sh.device, sh.first, sh.count, loglik, node_post, joint_states, joint_logp);
  });
}

}  // extern "C"
