// phm_time_models_wide_api.cpp -- C-ABI of the exact expectations through time for many rate matrices at 9..64 states, batched
// over the models (phm_expected_through_time_models_wide).  phm_expected_through_time_models' arguments and
// checks (ll_validate, section 16's checks of the bounds and the points and its plan, phm_time_models_host.h, shared by every model
// and device) plus section 27's labels (phm_branch_rows_host.h).  Per device and per chunk of models P_k(t_b) by Pade and mu_k, B_k
// (launch_scw_model); per chunk of sites section 23's tips / up / root launches with lam stored and its down pass with F stored
// (AwLanes), all unchanged; then per launch of items the along-branch vectors, the sub-branch rows and the fixed-order sums of
// phm_time_models_wide.hip, and per chunk the labelled sums of the bins' total rows (br_label_kernel).  An evaluation touches no
// other evaluation's buffers and the sums run over the items in item order whatever the launches, so neither the chunks nor the
// shards change an output bit.
#include "phm_ancestral_wide_host.h"
#include "phm_branch_rows.h"
#include "phm_time_models_wide.h"
#include "phm_time_models_wide_host.h"

#include "../../include/phylomap_hip_ext6.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;
using namespace phm_tm;
using namespace phm_tmw;

const std::string TMW_FN = "phm_expected_through_time_models_wide: ";

struct TmwInput {
  LlInput ll;
  TmPlan plan;
  phm_br::BrSelection lab;                              // the labels (its edge list is not used)
  int64_t n_eval = 0;                                   // S * K (cross) or K (paired): the fastest axis of every output
  int64_t n_points = 0;
  std::vector<phm::ExDown> down;                        // grouped by the depth of the parent
  std::vector<int32_t> down_off, child_row;
};

struct TmwOut {
  double* occupancy;
  double* bin_stats;
  double* point_post;
  double* loglik;
};

// An evaluation of a chunk: where its values lie in the chunk's rows, where they go in the caller's arrays, and whether it is
// possible (an impossible one gets NaN).
struct TmwLive { size_t at; int64_t ev; bool ok; };

// models [first, first + count) on one device, one state per lane
int32_t tmw_device(const TmwInput& tmi, int32_t device, int64_t first, int64_t count, const TmwOut& o) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = tmi.ll;
  const TmPlan& pl = tmi.plan;
  const int n = in.n, E = in.E, NT = in.NT, NP = phm::aw_lanes(n), L = tmi.lab.n_labels;
  const int KB = pl.n_bounds, NB = std::max(0, KB - 1);
  const size_t nn = (size_t)n * n, n_eval = (size_t)tmi.n_eval;
  const int64_t S_eval = in.sites_per_model();
  const int64_t NPt = (int64_t)pl.pts.size(), NS = (int64_t)pl.sub.size();
  const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  KernelTimer tm;
  double t_pass = 0.0, t_along = 0.0, t_branch = 0.0, t_reduce = 0.0;
  AwLanes ln(in);
  DevBuf ddown, dchild, dpts, dsub, dcoff, dboff, dw;
  st = ln.upload_tree();
  if (st) return st;
  HIPCHK(upload(ddown, tmi.down)); HIPCHK(upload(dchild, tmi.child_row));
  HIPCHK(upload(dpts, pl.pts)); HIPCHK(upload(dsub, pl.sub)); HIPCHK(upload(dcoff, pl.cross_off)); HIPCHK(upload(dboff, pl.bin_off));
  if (L > 0) HIPCHK(upload(dw, tmi.lab.w));

  // On top of section 23's footprint: per model mu and B; per evaluation O, F with their exponents, lam and the sums per boundary,
  // per bin and per labelled bin.  What the stages of one launch write takes a fixed share: the posteriors, and a, beta and the rows.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const int chunk = g_phm_debug.expect_chunk;
  AwPlan ap = aw_plan(free_b, in, count, chunk, 2 * TM_SCRATCH, sizeof(double) * (nn + 1),
                      tmw_per_eval_bytes(n, NT, E, KB, o.occupancy != nullptr, o.bin_stats != nullptr, L));
  const TmwLaunch lc = tmw_launches(n, NPt, NS, chunk, ap.Kc_max, ap.Sc_max);
  const int step_max = ap.step_max, np_max = lc.np_max, ns_max = lc.ns_max;
  const size_t Km = (size_t)ap.Kc_max, Evm = Km * (size_t)ap.Sc_max;

  DevBuf dmu, dB, dO, dsO, dF, dsF, dlam, dpost, docc, da, dsa, dbe, dsbe, drows, dtot, dlab;
  st = ln.alloc(ap);
  if (st) return st;
  HIPCHK(dmu.alloc(sizeof(double) * Km)); HIPCHK(dB.alloc(sizeof(double) * nn * Km));
  HIPCHK(dO.alloc(sizeof(double) * (size_t)NT * NP * Evm)); HIPCHK(dsO.alloc(sizeof(int32_t) * (size_t)NT * Evm));
  HIPCHK(dF.alloc(sizeof(double) * (size_t)E * NP * Evm)); HIPCHK(dsF.alloc(sizeof(int32_t) * (size_t)E * Evm));
  HIPCHK(dlam.alloc(sizeof(double) * Evm));
  if (NPt) HIPCHK(dpost.alloc(sizeof(double) * n * (size_t)np_max * Evm));
  if (o.occupancy) HIPCHK(docc.alloc(sizeof(double) * n * (size_t)KB * Evm));
  if (NS) {
    HIPCHK(da.alloc(sizeof(double) * NP * (size_t)ns_max * Evm)); HIPCHK(dsa.alloc(sizeof(int32_t) * (size_t)ns_max * Evm));
    HIPCHK(dbe.alloc(sizeof(double) * NP * (size_t)ns_max * Evm)); HIPCHK(dsbe.alloc(sizeof(int32_t) * (size_t)ns_max * Evm));
    HIPCHK(drows.alloc(sizeof(double) * nn * (size_t)ns_max * Evm));
  }
  if (o.bin_stats) HIPCHK(dtot.alloc(sizeof(double) * nn * (size_t)NB * Evm));
  if (o.bin_stats && L > 0) HIPCHK(dlab.alloc(sizeof(double) * (size_t)L * (size_t)NB * Evm));
  // the rows copied out of one launch or one chunk; left uninitialised: every value read was copied in
  const size_t host_rows = std::max({(size_t)n * (size_t)np_max, (size_t)n * (size_t)KB, (L > 0 ? (size_t)L : nn) * (size_t)NB, (size_t)1});
  const std::unique_ptr<double[]> host(new double[host_rows * Evm]);
  std::vector<TmwLive> live;

  for (int64_t c0 = 0; c0 < count; c0 += ap.Kc_max) {
    const int64_t Kc = std::min<int64_t>(ap.Kc_max, count - c0);
    const int64_t m0 = first + c0;                       // global index of this chunk's first model
    st = ln.load_models(m0, Kc);
    if (st) return st;
    phm::TmwParams tp = {};
    phm::ScwParams& sp = tp.sc;
    phm::AwParams& p = sp.aw;
    p = ln.params();
    p.Sc = 1;
    p.O = dO.as<double>(); p.sO = dsO.as<int32_t>(); p.F = dF.as<double>(); p.sF = dsF.as<int32_t>(); p.lam = dlam.as<double>();
    sp.Q = ln.dQ.as<double>(); sp.t = ln.dt.as<double>(); sp.child = dchild.as<int32_t>(); sp.mu = dmu.as<double>();
    sp.B = dB.as<double>();
    // the totals kernels' form words and buffers: launch_scw_model asks for them, no launch here touches them
    sp.form = dchild.as<int32_t>(); sp.runs = dlam.as<double>(); sp.tot = dlam.as<double>();
    HIPCHK(tm.start());
    st = ln.expm();
    if (st) return st;
    HIPCHK(phm::launch_scw_model(sp, nullptr));
    HIPCHK(tm.stop());
    st = ln.fetch_bad();
    if (st) return st;
    HIPCHK(tm.add_to(t_pass));

    for (int64_t s0 = 0; s0 < S_eval; s0 += ap.Sc_max) {
      const int64_t Sc = std::min<int64_t>(ap.Sc_max, S_eval - s0);
      p.Sc = (int)Sc;
      const size_t Ev = (size_t)Sc * (size_t)Kc;
      st = ln.stage_tips(s0, Sc);
      if (st) return st;
      const phm::ExDown* down = ddown.as<phm::ExDown>();
      HIPCHK(tm.start());
      st = ln.passes(p);
      if (st) return st;
      st = aw_level_steps(tmi.down_off, step_max, [&](int k0, int cnt) { return phm::launch_aw_down(p, down + k0, cnt, nullptr); });
      if (st) return st;
      HIPCHK(tm.stop());
      st = ln.fetch_ll(Sc);
      if (st) return st;
      HIPCHK(tm.add_to(t_pass));
      live.clear();
      for (int64_t k = 0; k < Kc; ++k)
        for (int64_t s = 0; s < Sc; ++s) {
          const size_t at = (size_t)k * (size_t)Sc + (size_t)s;
          const int64_t ev = ll_eval_of(in, s0 + s, m0 + k);
          // an impossible evaluation, or a model whose Pade met a zero pivot: -inf and NaN rows
          const bool ok = ln.possible(k, at);
          if (o.loglik) o.loglik[ev] = ok ? ln.llh[at] : ninf;
          live.push_back({at, ev, ok});
        }
      // host[r][Ev][cols] -> dst[col][row0 + r][n_eval] for rows r of a block of `rows` rows of `n_rows` in all
      auto scatter = [&](size_t rows, size_t cols, double* dst, size_t n_rows, size_t row0) {
        for (size_t r = 0; r < rows; ++r)
          for (size_t c = 0; c < cols; ++c) {
            double* d = dst + (c * n_rows + row0 + r) * n_eval;
            const double* src = host.get() + r * Ev * cols + c;
            for (const TmwLive& v : live) d[v.ev] = v.ok ? src[v.at * cols] : nan;
          }
      };

      // posteriors at the crossings (summed per boundary) and at the caller's points: [item][Ev][state]
      if (o.occupancy) HIPCHK(hipMemset(docc.p, 0, sizeof(double) * n * (size_t)KB * Ev));
      tp.post = dpost.as<double>();
      for (int64_t q0 = 0; q0 < NPt; q0 += np_max) {
        const int nq = (int)std::min<int64_t>(np_max, NPt - q0);
        tp.items = dpts.as<phm::TmItem>() + q0;
        HIPCHK(tm.start());
        HIPCHK(phm::launch_tmw_along(tp, nq, nullptr));
        HIPCHK(tm.stop());
        HIPCHK(tm.add_to(t_along));
        if (o.occupancy && q0 < pl.n_cross) {
          int r0 = 0, r1 = 0;
          tm_ranges(pl.cross_off, q0, q0 + nq, r0, r1);
          HIPCHK(tm.start());
          HIPCHK(phm::launch_tmw_range_sum(dpost.as<double>(), (int64_t)Ev * n, nq, q0, dcoff.as<int64_t>(), r0, r1, KB, docc.as<double>(), nullptr));
          HIPCHK(tm.stop());
          HIPCHK(tm.add_to(t_reduce));
        }
        if (o.point_post && q0 + nq > pl.n_cross) {
          const int64_t a0 = std::max(q0, pl.n_cross), na = q0 + nq - a0;   // items a0 .. of the launch are the caller's points
          HIPCHK(hipMemcpy(host.get(), dpost.as<double>() + (size_t)(a0 - q0) * n * Ev, sizeof(double) * (size_t)na * n * Ev, hipMemcpyDeviceToHost));
          scatter((size_t)na, (size_t)n, o.point_post, (size_t)tmi.n_points, (size_t)(a0 - pl.n_cross));
        }
      }
      if (o.occupancy) {                                   // [bound][Ev][state]
        HIPCHK(hipMemcpy(host.get(), docc.p, sizeof(double) * n * (size_t)KB * Ev, hipMemcpyDeviceToHost));
        scatter((size_t)KB, (size_t)n, o.occupancy, (size_t)KB, 0);
      }

      // sub-branch rows and their sums per bin: [bin][Ev][col]
      if (o.bin_stats) {
        HIPCHK(hipMemset(dtot.p, 0, sizeof(double) * nn * (size_t)NB * Ev));
        tp.post = nullptr; tp.a = da.as<double>(); tp.sa = dsa.as<int32_t>(); tp.beta = dbe.as<double>(); tp.sbeta = dsbe.as<int32_t>();
        tp.rows = drows.as<double>();
        for (int64_t k0 = 0; k0 < NS; k0 += ns_max) {
          const int nk = (int)std::min<int64_t>(ns_max, NS - k0);
          tp.items = dsub.as<phm::TmItem>() + k0;
          HIPCHK(tm.start());
          HIPCHK(phm::launch_tmw_along(tp, nk, nullptr));
          HIPCHK(tm.stop());
          HIPCHK(tm.add_to(t_along));
          HIPCHK(tm.start());
          HIPCHK(phm::launch_tmw_branch(tp, nk, nullptr));
          HIPCHK(tm.stop());
          HIPCHK(tm.add_to(t_branch));
          int r0 = 0, r1 = 0;
          tm_ranges(pl.bin_off, k0, k0 + nk, r0, r1);
          HIPCHK(tm.start());
          HIPCHK(phm::launch_tmw_range_sum(drows.as<double>(), (int64_t)Ev * (int64_t)nn, nk, k0, dboff.as<int64_t>(), r0, r1, NB, dtot.as<double>(), nullptr));
          HIPCHK(tm.stop());
          HIPCHK(tm.add_to(t_reduce));
        }
        if (L > 0) {                                       // each bin's total row reduced to its labelled sums: [bin][label][Ev]
          HIPCHK(tm.start());
          for (int b0 = 0; b0 < NB; b0 += phm::BR_GRID_MAX) {
            phm::BrLabelParams lp = {};
            lp.rows = dtot.as<double>() + (size_t)b0 * Ev * nn; lp.w = dw.as<double>(); lp.out = dlab.as<double>() + (size_t)b0 * L * Ev;
            lp.cols = (int)nn; lp.n_labels = L; lp.count = std::min(phm::BR_GRID_MAX, NB - b0); lp.n_ev = (int64_t)Ev;
            lp.row_j = (int64_t)Ev * (int64_t)nn; lp.row_ev = (int64_t)nn; lp.row_col = 1;
            HIPCHK(phm::launch_br_labels(lp, nullptr));
          }
          HIPCHK(tm.stop());
          HIPCHK(tm.add_to(t_reduce));
          HIPCHK(hipMemcpy(host.get(), dlab.p, sizeof(double) * (size_t)L * (size_t)NB * Ev, hipMemcpyDeviceToHost));
          for (int b = 0; b < NB; ++b)
            for (int l = 0; l < L; ++l) {
              double* d = o.bin_stats + ((size_t)l * NB + b) * n_eval;
              const double* src = host.get() + ((size_t)b * L + l) * Ev;
              for (const TmwLive& v : live) d[v.ev] = v.ok ? src[v.at] : nan;
            }
        } else {
          HIPCHK(hipMemcpy(host.get(), dtot.p, sizeof(double) * nn * (size_t)NB * Ev, hipMemcpyDeviceToHost));
          scatter((size_t)NB, nn, o.bin_stats, (size_t)NB, 0);
        }
      }
    }
  }
  if (g_phm_debug.phase_timing)
    std::fprintf(stderr, "phm_expected_through_time_models_wide: passes %.3f ms, along-branch vectors %.3f ms, branch stage %.3f ms, reductions %.3f ms\n",
                 t_pass, t_along, t_branch, t_reduce);
  g_phm_last_kernel_ms = t_pass + t_along + t_branch + t_reduce;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Models are independent: with phm_options.n_devices > 1 device d computes a contiguous range of them (phm_plan_shards,
// run_shards); every output value is the one-device value bit for bit.
int32_t phm_expected_through_time_models_wide(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                              int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const phm_options* opt,
                                              int32_t n_bounds, const double* bounds, int32_t n_labels, const double* labels,
                                              double* occupancy, double* bin_stats, int64_t n_points, const int32_t* point_edge,
                                              const double* point_pos, double* point_post, double* loglik) {
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid)
    return fail(PHM_ERR_BAD_INPUT, TMW_FN + "NULL argument (x, Q and pid are required)");
  if (!occupancy && !bin_stats && !point_post && !loglik)
    return fail(PHM_ERR_BAD_INPUT, TMW_FN + "no output requested (occupancy, bin_stats, point_post and loglik are all NULL)");
  if (!tmw_serves(n_states))
    return fail(PHM_ERR_UNSUPPORTED, TMW_FN + "9..64 states only: 2..8 states go to phm_expected_through_time_models");
  TmwInput tmi;
  LlInput& in = tmi.ll;
  int32_t st = ll_validate(TMW_FN, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, o, in);
  if (st) return st;
  if ((int64_t)in.S * in.K > (int64_t)INT32_MAX) return fail(PHM_ERR_BAD_INPUT, TMW_FN + "sites * models must fit in 31 bits");
  std::string err;
  st = tm_check_counts(n_bounds, bounds, occupancy != nullptr, bin_stats != nullptr, n_points, point_edge, point_pos, point_post != nullptr, err);
  if (st) return fail(st, TMW_FN + err);
  if (labels && !bin_stats) return fail(PHM_ERR_BAD_INPUT, TMW_FN + "labels need bin_stats");
  st = phm_br::br_select(in.n, in.E, 0, nullptr, n_labels, labels, tmi.lab, err);
  if (st) return fail(st, TMW_FN + err);
  std::vector<double> mu;
  phm_br::br_model_mu(in.Qr.data(), in.n, in.K, mu);
  // every edge row carries the passes and a sum of about mu t_b terms: all are held to the limit (tmi.lab lists every edge row)
  st = phm_br::br_check_jump_mean(mu, in.edge_length.data(), tmi.lab, EX_MAX_JUMP_MEAN, err);
  if (st) return fail(st, TMW_FN + err);
  tmi.n_eval = in.paired ? in.K : (int64_t)in.S * in.K;
  tmi.n_points = n_points;
  ex_down_schedule(in.sched, in.T, tmi.down, tmi.down_off, &tmi.child_row);
  TmTree tr;
  tr.E = in.E; tr.NT = in.NT; tr.root = in.T + in.sched.root; tr.t = in.edge_length.data();
  tr.parent.assign((size_t)in.E, 0);
  tr.child = tmi.child_row;
  for (const phm::ExDown& d : tmi.down) {
    tr.order.push_back(d.edge);
    tr.parent[d.edge] = d.parent;
  }
  st = tm_plan(tr, n_bounds, bounds, occupancy != nullptr, bin_stats != nullptr, n_points, point_edge, point_pos, point_post != nullptr,
               tmi.plan, err);
  if (st) return fail(st, TMW_FN + err);
  const TmwOut out = {occupancy, bin_stats, point_post, loglik};
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, in.K, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) { return tmw_device(tmi, sh.device, sh.first, sh.count, out); });
}

}  // extern "C"
