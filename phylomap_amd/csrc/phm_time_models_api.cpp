// phm_time_models_api.cpp -- C-ABI of the exact expectations through time for many rate matrices in one call
// (phm_expected_through_time_models), 2..64 states.  phm_loglik_models' validation (ll_validate), section
// 16's checks of the bounds and the points and its plan (phm_time_models_host.h), shared by every model and device.  2..8 states:
// per device and per chunk of models P_k(t_b) once and, per chunk of sites, the passes of phm_expected_stats_models launched
// unchanged (LlLanes with phm_scores.hip's model, root and down kernels, the models across the lanes), then per launch of items
// the along-branch vectors, the sub-branch rows and the fixed-order sums of phm_time_models.hip.  9..64 states: one model after
// another through phm_expected_through_time itself.  An evaluation touches no other evaluation's buffers and the sums run over
// the items in item order whatever the launches, so neither the chunks nor the shards change an output bit.
#include "phm_branch_rows_host.h"
#include "phm_loglik_host.h"
#include "phm_time_models.h"
#include "phm_time_models_host.h"

#include "../../include/phylomap_hip_ext5.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;
using namespace phm_tm;

const std::string TM_FN = "phm_expected_through_time_models: ";

struct TmInput {
  LlInput ll;
  TmPlan plan;
  int64_t n_eval = 0;                                   // S * K (cross) or K (paired): the fastest axis of every output
  int64_t n_points = 0;
  std::vector<phm::ExDown> down;                        // grouped by the depth of the parent
  std::vector<int32_t> down_off, child_row;
};

struct TmOut {
  double* occupancy;
  double* bin_stats;
  double* point_post;
  double* loglik;
};

// An evaluation of a chunk: where its values lie in the chunk's rows, where they go in the caller's arrays, and whether it is
// possible (an impossible one gets NaN).
struct TmLive { int64_t src, ev; bool ok; };

// host[r][Eo] -> dst[(row0 + r)][n_eval] for `rows` rows
void tm_scatter(const double* host, size_t rows, size_t Eo, const std::vector<TmLive>& live, double* dst, size_t n_eval) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t r = 0; r < rows; ++r) {
    const double* src = host + r * Eo;
    double* d = dst + r * n_eval;
    for (const TmLive& v : live) d[v.ev] = v.ok ? src[v.src] : nan;
  }
}

// 2..8 states: models [first, first + count) on one device, models across the lanes
int32_t tm_lanes_device(const TmInput& tmi, int32_t device, int64_t first, int64_t count, const TmOut& o) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = tmi.ll;
  const TmPlan& pl = tmi.plan;
  const int n = in.n, E = in.E, NT = in.NT, NB = std::max(0, pl.n_bounds - 1), KB = pl.n_bounds;
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.sites_per_model();
  const int64_t NP = (int64_t)pl.pts.size(), NS = (int64_t)pl.sub.size();
  KernelTimer tm;
  double t_pass = 0.0, t_along = 0.0, t_branch = 0.0, t_reduce = 0.0;
  LlLanes ln(in);
  DevBuf ddown, dchild, dpts, dsub, dcoff, dboff;
  st = ln.upload_tree();
  if (st) return st;
  HIPCHK(upload(ddown, tmi.down)); HIPCHK(upload(dchild, tmi.child_row));
  HIPCHK(upload(dpts, pl.pts)); HIPCHK(upload(dsub, pl.sub)); HIPCHK(upload(dcoff, pl.cross_off)); HIPCHK(upload(dboff, pl.bin_off));

  // On top of section 17's footprint: per model mu and B; per evaluation O, F with their exponents, lam and the sums per boundary
  // and per bin.  What the stages of one launch write takes a fixed share: the posteriors, and a, beta and the rows.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const bool ws = n > phm::LL_REG_MAX;
  const int chunk = g_phm_debug.expect_chunk;
  const size_t cell_p = (size_t)n, cell_s = 2 * (size_t)n + 2 + nn;        // doubles per (item, evaluation): points, sub-branches
  LlPlan lp = ll_plan(free_b, in, count, chunk, 2 * TM_SCRATCH, sizeof(double) * (nn + 1),
                      sizeof(double) * ((size_t)NT * (n + 1) + (size_t)E * (n + 1) + 1 + (o.occupancy ? (size_t)n * KB : 0) +
                                        (o.bin_stats ? nn * (size_t)NB : 0)));
  phm_br::br_fit_chunk(NS ? cell_s : cell_p, 64, lp.Kc_max, lp.Sc_max);   // one item of a chunk fits in the scratch
  const size_t Kpm = (size_t)lp.Kc_max, Evm = Kpm * (size_t)lp.Sc_max;
  // the stages' buffers hold a chunk's models without the lanes that pad them to 64: Eom evaluations at most
  const size_t Eom = (size_t)std::min<int64_t>(lp.Kc_max, count) * (size_t)lp.Sc_max;
  const int np_max = NP ? tm_items_per_launch(NP, cell_p, Eom, chunk) : 0;
  const int ns_max = NS ? tm_items_per_launch(NS, cell_s, Eom, chunk) : 0;

  DevBuf dmu, dB, dO, dsO, dF, dsF, dlam, dpost, docc, da, dsa, dbe, dsbe, drows, dtot;
  st = ln.alloc(lp);
  if (st) return st;
  HIPCHK(dmu.alloc(sizeof(double) * Kpm));
  if (ws) HIPCHK(dB.alloc(sizeof(double) * nn * Kpm));
  HIPCHK(dO.alloc(sizeof(double) * (size_t)NT * n * Evm)); HIPCHK(dsO.alloc(sizeof(double) * (size_t)NT * Evm));
  HIPCHK(dF.alloc(sizeof(double) * (size_t)E * n * Evm)); HIPCHK(dsF.alloc(sizeof(double) * (size_t)E * Evm));
  HIPCHK(dlam.alloc(sizeof(double) * Evm));
  if (NP) HIPCHK(dpost.alloc(sizeof(double) * n * (size_t)np_max * Eom));
  if (o.occupancy) HIPCHK(docc.alloc(sizeof(double) * n * (size_t)KB * Eom));
  if (NS) {
    HIPCHK(da.alloc(sizeof(double) * n * (size_t)ns_max * Eom)); HIPCHK(dsa.alloc(sizeof(double) * (size_t)ns_max * Eom));
    HIPCHK(dbe.alloc(sizeof(double) * n * (size_t)ns_max * Eom)); HIPCHK(dsbe.alloc(sizeof(double) * (size_t)ns_max * Eom));
    HIPCHK(drows.alloc(sizeof(double) * nn * (size_t)ns_max * Eom));
  }
  if (o.bin_stats) HIPCHK(dtot.alloc(sizeof(double) * nn * (size_t)NB * Eom));
  // the rows copied out of one launch or one chunk; left uninitialised: every value read was copied in
  const size_t host_rows = std::max({(size_t)n * (size_t)np_max, (size_t)n * (size_t)KB, nn * (size_t)NB, (size_t)1});
  const std::unique_ptr<double[]> host(new double[host_rows * Eom]);
  std::vector<TmLive> live;

  for (int64_t c0 = 0; c0 < count; c0 += lp.Kc_max) {
    const int64_t Kc = std::min<int64_t>(lp.Kc_max, count - c0);
    st = ln.load_models(first + c0, Kc);
    if (st) return st;
    const int Kp = ln.Kp;
    const int64_t m0 = ln.m0;                            // global index of this chunk's first model
    phm::TmParams tp = {};
    phm::ScParams& sp = tp.sc;
    phm::LlParams& p = sp.ll;
    p = ln.params();
    sp.n_edge = E; sp.root = in.T + in.sched.root; sp.mu = dmu.as<double>(); sp.B = ws ? dB.as<double>() : nullptr;
    sp.child = dchild.as<int32_t>(); sp.O = dO.as<double>(); sp.sO = dsO.as<double>(); sp.F = dF.as<double>();
    sp.sF = dsF.as<double>(); sp.lam = dlam.as<double>();
    HIPCHK(tm.start());
    st = ln.expm(p);
    if (st) return st;
    HIPCHK(phm::launch_sc_model(sp, nullptr));
    HIPCHK(tm.stop());
    HIPCHK(tm.add_to(t_pass));

    for (int64_t s0 = 0; s0 < S_eval; s0 += lp.Sc_max) {
      const int64_t Sc = std::min<int64_t>(lp.Sc_max, S_eval - s0);
      p.n_sites = (int)Sc;
      const size_t Eo = (size_t)Sc * (size_t)Kc;
      st = ln.stage_tips(s0, Sc);
      if (st) return st;
      HIPCHK(tm.start());
      st = ln.passes(p);
      if (st) return st;
      HIPCHK(phm::launch_sc_root(sp, nullptr));
      for (size_t l = 0; l + 1 < tmi.down_off.size(); ++l)
        HIPCHK(phm::launch_sc_down(sp, ddown.as<phm::ExDown>() + tmi.down_off[l], tmi.down_off[l + 1] - tmi.down_off[l], nullptr));
      HIPCHK(tm.stop());
      st = ln.fetch_ll(Sc);
      if (st) return st;
      HIPCHK(tm.add_to(t_pass));
      live.clear();
      for (int64_t k = 0; k < Kc; ++k)
        for (int64_t s = 0; s < Sc; ++s) {
          const double ll = ln.llh[(size_t)s * Kp + (size_t)k];              // in the passes' padded buffers
          const int64_t ev = ll_eval_of(in, s0 + s, m0 + k);
          if (o.loglik) o.loglik[ev] = ll;
          live.push_back({(int64_t)((size_t)s * (size_t)Kc + (size_t)k), ev, std::isfinite(ll)});
        }

      // posteriors at the crossings (summed per boundary) and at the caller's points: [item][state][Eo]
      if (o.occupancy) HIPCHK(hipMemset(docc.p, 0, sizeof(double) * n * (size_t)KB * Eo));
      tp.post = dpost.as<double>();
      for (int64_t q0 = 0; q0 < NP; q0 += np_max) {
        const int nq = (int)std::min<int64_t>(np_max, NP - q0);
        tp.items = dpts.as<phm::TmItem>() + q0;
        HIPCHK(tm.start());
        HIPCHK(phm::launch_tm_along(tp, nq, nullptr));
        HIPCHK(tm.stop());
        HIPCHK(tm.add_to(t_along));
        if (o.occupancy && q0 < pl.n_cross) {
          int r0 = 0, r1 = 0;
          tm_ranges(pl.cross_off, q0, q0 + nq, r0, r1);
          HIPCHK(tm.start());
          HIPCHK(phm::launch_tm_range_sum(dpost.as<double>(), n, nq, q0, dcoff.as<int64_t>(), r0, r1, KB, (int64_t)Eo, docc.as<double>(), nullptr));
          HIPCHK(tm.stop());
          HIPCHK(tm.add_to(t_reduce));
        }
        if (o.point_post && q0 + nq > pl.n_cross) {
          const int64_t a0 = std::max(q0, pl.n_cross), na = q0 + nq - a0;   // items a0 .. of the launch are the caller's points
          HIPCHK(hipMemcpy(host.get(), dpost.as<double>() + (size_t)(a0 - q0) * n * Eo, sizeof(double) * (size_t)na * n * Eo, hipMemcpyDeviceToHost));
          for (int64_t j = 0; j < na; ++j)
            for (int i = 0; i < n; ++i)
              tm_scatter(host.get() + ((size_t)j * n + i) * Eo, 1, Eo, live,
                         o.point_post + ((size_t)i * (size_t)tmi.n_points + (size_t)(a0 - pl.n_cross + j)) * (size_t)tmi.n_eval, (size_t)tmi.n_eval);
        }
      }
      if (o.occupancy) {                                   // [state][bound][Eo]
        HIPCHK(hipMemcpy(host.get(), docc.p, sizeof(double) * n * (size_t)KB * Eo, hipMemcpyDeviceToHost));
        tm_scatter(host.get(), (size_t)n * KB, Eo, live, o.occupancy, (size_t)tmi.n_eval);
      }

      // sub-branch rows and their sums per bin: [col][bin][Eo]
      if (o.bin_stats) {
        HIPCHK(hipMemset(dtot.p, 0, sizeof(double) * nn * (size_t)NB * Eo));
        tp.post = nullptr; tp.a = da.as<double>(); tp.sa = dsa.as<double>(); tp.beta = dbe.as<double>(); tp.sbeta = dsbe.as<double>();
        tp.rows = drows.as<double>();
        for (int64_t k0 = 0; k0 < NS; k0 += ns_max) {
          const int nk = (int)std::min<int64_t>(ns_max, NS - k0);
          tp.items = dsub.as<phm::TmItem>() + k0;
          HIPCHK(tm.start());
          HIPCHK(phm::launch_tm_along(tp, nk, nullptr));
          HIPCHK(tm.stop());
          HIPCHK(tm.add_to(t_along));
          HIPCHK(tm.start());
          HIPCHK(phm::launch_tm_branch(tp, nk, nullptr));
          HIPCHK(tm.stop());
          HIPCHK(tm.add_to(t_branch));
          int r0 = 0, r1 = 0;
          tm_ranges(pl.bin_off, k0, k0 + nk, r0, r1);
          HIPCHK(tm.start());
          HIPCHK(phm::launch_tm_range_sum(drows.as<double>(), (int)nn, nk, k0, dboff.as<int64_t>(), r0, r1, NB, (int64_t)Eo, dtot.as<double>(), nullptr));
          HIPCHK(tm.stop());
          HIPCHK(tm.add_to(t_reduce));
        }
        HIPCHK(hipMemcpy(host.get(), dtot.p, sizeof(double) * nn * (size_t)NB * Eo, hipMemcpyDeviceToHost));
        tm_scatter(host.get(), nn * (size_t)NB, Eo, live, o.bin_stats, (size_t)tmi.n_eval);
      }
    }
  }
  if (g_phm_debug.phase_timing)
    std::fprintf(stderr, "phm_expected_through_time_models: passes %.3f ms, along-branch vectors %.3f ms, branch stage %.3f ms, reductions %.3f ms\n",
                 t_pass, t_along, t_branch, t_reduce);
  g_phm_last_kernel_ms = t_pass + t_along + t_branch + t_reduce;
  return PHM_OK;
}

// 9..64 states: models [first, first + count) on one device, one after another through phm_expected_through_time.  Its outputs
// for S sites are [row][S], which is the run of model k's evaluations inside each row of this entry point's outputs in the cross
// order; a paired model is one call on its own site.
int32_t tm_wide_device(const TmInput& tmi, const phm_tree* x, const double* Q, const double* pid, int32_t n_pid, const int32_t* observe,
                       const phm_options& opt, int32_t device, int64_t first, int64_t count, const double* bounds,
                       const int32_t* point_edge, const double* point_pos, const TmOut& o) {
  const LlInput& in = tmi.ll;
  const int n = in.n, KB = tmi.plan.n_bounds, NB = std::max(0, KB - 1);
  const size_t nn = (size_t)n * n, n_eval = (size_t)tmi.n_eval, P = (size_t)tmi.n_points;
  const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  double kernel_ms = 0.0;
  phm_options ok = opt;
  ok.n_devices = 0;
  ok.device = device;
  // sites [s0, s0 + Sn) of model k in one call; the rows land at evaluation ev0 ..
  std::vector<double> occ, bins, post, ll;
  auto run = [&](int64_t k, int64_t s0, int64_t Sn, size_t ev0) -> int32_t {
    phm_tree xt = *x;
    phm_options os = ok;
    xt.states = x->states + (in.per_site ? s0 * in.T : 0);
    os.n_replicas = (int32_t)Sn;
    if (o.occupancy) occ.assign((size_t)n * KB * Sn, 0.0);
    if (o.bin_stats) bins.assign(nn * (size_t)NB * Sn, 0.0);
    if (o.point_post) post.assign((size_t)n * P * Sn, 0.0);
    ll.assign((size_t)Sn, 0.0);
    const int32_t st = phm_expected_through_time(&xt, n, Q + (size_t)k * nn, pid + (n_pid == 1 ? 0 : (size_t)k * n), observe, &os, KB, bounds,
                                                 o.occupancy ? occ.data() : nullptr, o.bin_stats ? bins.data() : nullptr, (int64_t)P,
                                                 point_edge, point_pos, o.point_post ? post.data() : nullptr, ll.data());
    kernel_ms += g_phm_last_kernel_ms;
    const bool zero = st == PHM_ERR_ZERO_PROB && Sn == 1;   // one impossible evaluation: -inf and NaN rows
    if (st && !zero) return st;
    auto rows = [&](const std::vector<double>& src, size_t n_rows, double* dst) {
      for (size_t r = 0; r < n_rows; ++r)
        for (int64_t s = 0; s < Sn; ++s) dst[r * n_eval + ev0 + (size_t)s] = zero ? nan : src[r * (size_t)Sn + (size_t)s];
    };
    if (o.occupancy) rows(occ, (size_t)n * KB, o.occupancy);
    if (o.bin_stats) rows(bins, nn * (size_t)NB, o.bin_stats);
    if (o.point_post) rows(post, (size_t)n * P, o.point_post);
    if (o.loglik)
      for (int64_t s = 0; s < Sn; ++s) o.loglik[ev0 + (size_t)s] = zero ? ninf : ll[(size_t)s];
    return PHM_OK;
  };
  for (int64_t k = first; k < first + count; ++k) {
    if (in.paired) {
      const int32_t st = run(k, in.site_of_model[k], 1, (size_t)k);
      if (st) return st;
      continue;
    }
    int32_t st = run(k, 0, in.S, (size_t)in.S * (size_t)k);
    if (st == PHM_ERR_ZERO_PROB && in.S > 1)               // some site of this model is impossible: one site at a time
      for (int64_t s = 0; s < in.S; ++s) {
        st = run(k, s, 1, (size_t)in.S * (size_t)k + (size_t)s);
        if (st) break;
      }
    if (st) return st;
  }
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Models are independent: with phm_options.n_devices > 1 device d computes a contiguous range of them (phm_plan_shards,
// run_shards); every output value is the one-device value bit for bit.
int32_t phm_expected_through_time_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                         int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const phm_options* opt,
                                         int32_t n_bounds, const double* bounds, double* occupancy, double* bin_stats,
                                         int64_t n_points, const int32_t* point_edge, const double* point_pos, double* point_post,
                                         double* loglik) {
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid)
    return fail(PHM_ERR_BAD_INPUT, TM_FN + "NULL argument (x, Q and pid are required)");
  if (!occupancy && !bin_stats && !point_post && !loglik)
    return fail(PHM_ERR_BAD_INPUT, TM_FN + "no output requested (occupancy, bin_stats, point_post and loglik are all NULL)");
  TmInput tmi;
  LlInput& in = tmi.ll;
  int32_t st = ll_validate(TM_FN, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, o, in);
  if (st) return st;
  std::string err;
  st = tm_check_counts(n_bounds, bounds, occupancy != nullptr, bin_stats != nullptr, n_points, point_edge, point_pos, point_post != nullptr, err);
  if (st) return fail(st, TM_FN + err);
  std::vector<double> mu;
  phm_br::br_model_mu(in.Qr.data(), in.n, in.K, mu);
  phm_br::BrSelection all;                               // every edge row carries the passes: all are held to the limit
  all.edges.resize((size_t)in.E);
  for (int b = 0; b < in.E; ++b) all.edges[b] = b;
  st = phm_br::br_check_jump_mean(mu, in.edge_length.data(), all, EX_MAX_JUMP_MEAN, err);
  if (st) return fail(st, TM_FN + err);
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
  if (st) return fail(st, TM_FN + err);
  const TmOut out = {occupancy, bin_stats, point_post, loglik};
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, in.K, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) {
    return in.n <= phm::LL_LANE_MAX ? tm_lanes_device(tmi, sh.device, sh.first, sh.count, out)
                                    : tm_wide_device(tmi, x, Q, pid, n_pid, observe, o, sh.device, sh.first, sh.count, bounds, point_edge,
                                                     point_pos, out);
  });
}

}  // extern "C"
