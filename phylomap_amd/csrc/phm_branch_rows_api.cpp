// phm_branch_rows_api.cpp -- C-ABI of the exact conditional expectations PER BRANCH for many rate matrices in one call
// (phm_expected_branch_stats_models), 2..64 states.  phm_loglik_models' validation (ll_validate), the edge
// selection and the labels (phm_branch_rows_host.h), then per device and per chunk of models P_k(t_b) once and, per chunk of
// sites, the passes of the totals entry points, launched unchanged: LlLanes with phm_scores.hip's model, root and down kernels at
// 2..8 states (models across the lanes), AwLanes with section 23's down pass and phm_scores_wide.hip's model kernel at 9..64 states
// (one state per lane).  The branch stage is this feature's (phm_branch_rows.hip, phm_branch_rows_wide.hip): it keeps each
// selected edge's finished row in a scratch of at most BR_SCRATCH bytes a launch; the rows are copied out, or first reduced to the
// labelled sums (br_label_kernel) so that a codon model moves a few doubles per branch, not 3 721.  An evaluation touches no other
// evaluation's buffers and an entry no other entry's, so neither the chunks nor the shards change an output bit.
#include "phm_ancestral_wide_host.h"
#include "phm_branch_rows.h"
#include "phm_branch_rows_host.h"
#include "phm_branch_rows_wide.h"

#include "../../include/phylomap_hip_ext4.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;
using namespace phm_br;

const std::string BR_FN = "phm_expected_branch_stats_models: ";

struct BrInput {
  LlInput ll;
  BrSelection sel;
  int64_t n_eval = 0;                                   // S * K (cross) or K (paired): values of loglik, fastest axis of branch
  std::vector<double> mu;                               // [K] max_i(-q_ii)
  std::vector<phm::ExDown> down;                        // grouped by the depth of the parent
  std::vector<int32_t> down_off, child_row;
};

// f(begin, end) over [0, n_items) on up to 8 threads when there are at least 4M values to move: the scatter of a large call is
// bound by the first touch of the caller's pages and by memory latency, and either spreads over threads
template <class F>
void br_parallel(int n_items, size_t values, F&& f) {
  const unsigned nt = values < (size_t(1) << 22) ? 1u : std::min<unsigned>({8u, std::max(1u, std::thread::hardware_concurrency()), (unsigned)n_items});
  if (nt <= 1) { f(0, n_items); return; }
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt; ++t) th.emplace_back([&f, n_items, nt, t] { f((int)((int64_t)n_items * t / nt), (int)((int64_t)n_items * (t + 1) / nt)); });
  f(0, (int)((int64_t)n_items / nt));
  for (std::thread& t : th) t.join();
}

// The branch stage of one chunk of evaluations, the same for both families: the selected edges in launches of ne_max, each
// followed by the label reduction when labels are asked for, one copy to the host and the scatter into the caller's layout
// [C][n_sel][evaluations].  launch(sel, count) runs the family's branch kernel into drows; at(k, s) is the chunk's evaluation of
// (model k, site s) and row_* the family's row layout (phm_branch_rows.h); possible(k, s) and eval(k, s) are the driver's.
template <class Launch, class At, class Possible, class Eval>
int32_t br_branch_stage(const BrInput& br, int ne_max, const DevBuf& dsel, const DevBuf& dw, DevBuf& drows, DevBuf& dlab, double* host,
                        size_t Ev, int64_t Kc, int64_t Sc, int64_t row_j, int64_t row_ev, int64_t row_col, KernelTimer& tm, double& kernel_ms,
                        Launch&& launch, At&& at, Possible&& possible, Eval&& eval, double* branch) {
  const int cols = br.ll.n * br.ll.n, L = br.sel.n_labels, C_out = br.sel.out_cols;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // labelled sums are [entry][label][ev]; full rows are in the family's own layout
  const int64_t h_j = L > 0 ? (int64_t)L * (int64_t)Ev : row_j, h_ev = L > 0 ? 1 : row_ev, h_col = L > 0 ? (int64_t)Ev : row_col;
  struct Live { int64_t src, ev; bool ok; };             // an evaluation of the chunk: where its values lie, where they go
  std::vector<Live> live;
  live.reserve((size_t)Kc * (size_t)Sc);
  for (int64_t k = 0; k < Kc; ++k)
    for (int64_t s = 0; s < Sc; ++s) live.push_back({(int64_t)at(k, s) * h_ev, eval(k, s), possible(k, s)});
  for (int e0 = 0; e0 < br.sel.n_sel; e0 += ne_max) {
    const int ne = std::min(ne_max, br.sel.n_sel - e0);
    HIPCHK(tm.start());
    HIPCHK(launch(dsel.as<int32_t>() + e0, ne));
    if (L > 0) {
      phm::BrLabelParams lp = {};
      lp.rows = drows.as<double>(); lp.w = dw.as<double>(); lp.out = dlab.as<double>();
      lp.cols = cols; lp.n_labels = L; lp.count = ne; lp.n_ev = (int64_t)Ev;
      lp.row_j = row_j; lp.row_ev = row_ev; lp.row_col = row_col;
      HIPCHK(phm::launch_br_labels(lp, nullptr));
    }
    HIPCHK(tm.stop());
    HIPCHK(hipMemcpy(host, L > 0 ? dlab.p : drows.p, sizeof(double) * (size_t)ne * (size_t)C_out * Ev, hipMemcpyDeviceToHost));
    HIPCHK(tm.add_to(kernel_ms));
    br_parallel(ne, (size_t)ne * (size_t)C_out * live.size(), [&](int j0, int j1) {
      for (int j = j0; j < j1; ++j)
        for (int c = 0; c < C_out; ++c) {
          const double* src = host + (int64_t)j * h_j + (int64_t)c * h_col;
          double* dst = branch + ((size_t)c * br.sel.n_sel + (size_t)(e0 + j)) * (size_t)br.n_eval;
          for (const Live& v : live) dst[v.ev] = v.ok ? src[v.src] : nan;   // an impossible evaluation: NaN in all of its rows
        }
    });
  }
  return PHM_OK;
}

// 2..8 states: models [first, first + count) on one device, models across the lanes
int32_t br_lanes_device(const BrInput& br, int32_t device, int64_t first, int64_t count, double* branch, double* loglik) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = br.ll;
  const int n = in.n, E = in.E, NT = in.NT, L = br.sel.n_labels;
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.sites_per_model();
  KernelTimer tm;
  double kernel_ms = 0.0;
  LlLanes ln(in);
  DevBuf ddown, dchild, dsel, dw;
  st = ln.upload_tree();
  if (st) return st;
  HIPCHK(upload(ddown, br.down)); HIPCHK(upload(dchild, br.child_row)); HIPCHK(upload(dsel, br.sel.edges));
  if (L > 0) HIPCHK(upload(dw, br.sel.w));

  // On top of section 17's footprint: per model mu and B; per evaluation O, F with their exponents and lam.  The rows of one
  // branch-stage launch, and their labelled sums, take a fixed share each.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const bool ws = n > phm::LL_REG_MAX;
  const int chunk = g_phm_debug.expect_chunk;
  const size_t cell = br_cell_doubles(n, br.sel);
  LlPlan pl = ll_plan(free_b, in, count, chunk, BR_SCRATCH * (L > 0 ? 2 : 1), sizeof(double) * (nn + 1),
                      sizeof(double) * ((size_t)NT * (n + 1) + (size_t)E * (n + 1) + 1));
  br_fit_chunk(cell, 64, pl.Kc_max, pl.Sc_max);
  const size_t Kpm = (size_t)pl.Kc_max, Evm = Kpm * (size_t)pl.Sc_max;
  // the rows hold a chunk's models without the lanes that pad them to 64: Eom evaluations at most
  const size_t Eom = (size_t)std::min<int64_t>(pl.Kc_max, count) * (size_t)pl.Sc_max;
  const int ne_max = br_edges_per_launch(br.sel.n_sel, cell, Eom, chunk, phm::BR_GRID_MAX);

  DevBuf dmu, dB, dO, dsO, dF, dsF, dlam, drows, dlab;
  st = ln.alloc(pl);
  if (st) return st;
  HIPCHK(dmu.alloc(sizeof(double) * Kpm));
  if (ws) HIPCHK(dB.alloc(sizeof(double) * nn * Kpm));
  HIPCHK(dO.alloc(sizeof(double) * (size_t)NT * n * Evm)); HIPCHK(dsO.alloc(sizeof(double) * (size_t)NT * Evm));
  HIPCHK(dF.alloc(sizeof(double) * (size_t)E * n * Evm)); HIPCHK(dsF.alloc(sizeof(double) * (size_t)E * Evm));
  HIPCHK(dlam.alloc(sizeof(double) * Evm));
  HIPCHK(drows.alloc(sizeof(double) * nn * (size_t)ne_max * Eom));
  if (L > 0) HIPCHK(dlab.alloc(sizeof(double) * (size_t)L * (size_t)ne_max * Eom));
  const std::unique_ptr<double[]> host(new double[(size_t)br.sel.out_cols * (size_t)ne_max * Eom]);   // left uninitialised: every value read was copied in

  for (int64_t c0 = 0; c0 < count; c0 += pl.Kc_max) {
    const int64_t Kc = std::min<int64_t>(pl.Kc_max, count - c0);
    st = ln.load_models(first + c0, Kc);
    if (st) return st;
    const int Kp = ln.Kp;
    const int64_t m0 = ln.m0;                            // global index of this chunk's first model
    phm::ScParams sp = {};
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
    HIPCHK(tm.add_to(kernel_ms));

    for (int64_t s0 = 0; s0 < S_eval; s0 += pl.Sc_max) {
      const int64_t Sc = std::min<int64_t>(pl.Sc_max, S_eval - s0);
      p.n_sites = (int)Sc;
      const size_t Eo = (size_t)Sc * (size_t)Kc;
      st = ln.stage_tips(s0, Sc);
      if (st) return st;
      HIPCHK(tm.start());
      st = ln.passes(p);
      if (st) return st;
      HIPCHK(phm::launch_sc_root(sp, nullptr));
      for (size_t l = 0; l + 1 < br.down_off.size(); ++l)
        HIPCHK(phm::launch_sc_down(sp, ddown.as<phm::ExDown>() + br.down_off[l], br.down_off[l + 1] - br.down_off[l], nullptr));
      HIPCHK(tm.stop());
      st = ln.fetch_ll(Sc);
      if (st) return st;
      HIPCHK(tm.add_to(kernel_ms));
      auto eval = [&](int64_t k, int64_t s) { return ll_eval_of(in, s0 + s, m0 + k); };
      auto lane = [&](int64_t k, int64_t s) { return (size_t)s * Kp + (size_t)k; };       // in the passes' padded buffers
      auto at = [&](int64_t k, int64_t s) { return (size_t)s * (size_t)Kc + (size_t)k; };  // in the rows
      auto possible = [&](int64_t k, int64_t s) { return std::isfinite(ln.llh[lane(k, s)]); };
      if (loglik)
        for (int64_t s = 0; s < Sc; ++s)
          for (int64_t k = 0; k < Kc; ++k) loglik[eval(k, s)] = ln.llh[lane(k, s)];
      // rows: [entry][col][Eo]
      st = br_branch_stage(br, ne_max, dsel, dw, drows, dlab, host.get(), Eo, Kc, Sc, (int64_t)nn * (int64_t)Eo, 1, (int64_t)Eo, tm, kernel_ms,
                           [&](const int32_t* sel, int ne) { return phm::launch_br_branch(sp, sel, ne, drows.as<double>(), nullptr); }, at,
                           possible, eval, branch);
      if (st) return st;
    }
  }
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

// 9..64 states: models [first, first + count) on one device, one state per lane
int32_t br_wide_device(const BrInput& br, int32_t device, int64_t first, int64_t count, double* branch, double* loglik) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = br.ll;
  const int n = in.n, E = in.E, NT = in.NT, NP = phm::aw_lanes(n), L = br.sel.n_labels;
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.sites_per_model();
  const double ninf = -std::numeric_limits<double>::infinity();
  KernelTimer tm;
  double kernel_ms = 0.0;
  AwLanes ln(in);
  DevBuf ddown, dchild, dsel, dw;
  st = ln.upload_tree();
  if (st) return st;
  HIPCHK(upload(ddown, br.down)); HIPCHK(upload(dchild, br.child_row)); HIPCHK(upload(dsel, br.sel.edges));
  if (L > 0) HIPCHK(upload(dw, br.sel.w));

  // On top of section 23's footprint: per model mu, B and the form words; per evaluation O, F with their exponents and lam.  The
  // rows of one branch-stage launch, and their labelled sums, take a fixed share each.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const int chunk = g_phm_debug.expect_chunk;
  const size_t vec_b = sizeof(double) * NP + sizeof(int32_t);
  const size_t cell = br_cell_doubles(n, br.sel);
  AwPlan pl = aw_plan(free_b, in, count, chunk, BR_SCRATCH * (L > 0 ? 2 : 1), sizeof(double) * (nn + 1) + sizeof(int32_t) * (size_t)E,
                      vec_b * (size_t)NT + vec_b * (size_t)E + sizeof(double));
  br_fit_chunk(cell, 1, pl.Kc_max, pl.Sc_max);
  const int step_max = pl.step_max;
  const size_t Km = (size_t)pl.Kc_max, Evm = Km * (size_t)pl.Sc_max;
  const int ne_max = br_edges_per_launch(br.sel.n_sel, cell, Evm, chunk, phm::BR_GRID_MAX);

  DevBuf dmu, dB, dform, dO, dsO, dF, dsF, dlam, drows, dlab;
  st = ln.alloc(pl);
  if (st) return st;
  HIPCHK(dmu.alloc(sizeof(double) * Km)); HIPCHK(dB.alloc(sizeof(double) * nn * Km)); HIPCHK(dform.alloc(sizeof(int32_t) * (size_t)E * Km));
  HIPCHK(dO.alloc(sizeof(double) * (size_t)NT * NP * Evm)); HIPCHK(dsO.alloc(sizeof(int32_t) * (size_t)NT * Evm));
  HIPCHK(dF.alloc(sizeof(double) * (size_t)E * NP * Evm)); HIPCHK(dsF.alloc(sizeof(int32_t) * (size_t)E * Evm));
  HIPCHK(dlam.alloc(sizeof(double) * Evm));
  HIPCHK(drows.alloc(sizeof(double) * nn * (size_t)ne_max * Evm));
  if (L > 0) HIPCHK(dlab.alloc(sizeof(double) * (size_t)L * (size_t)ne_max * Evm));
  const std::unique_ptr<double[]> host(new double[(size_t)br.sel.out_cols * (size_t)ne_max * Evm]);   // left uninitialised: every value read was copied in
  std::vector<int32_t> formh((size_t)E * Km);

  for (int64_t c0 = 0; c0 < count; c0 += pl.Kc_max) {
    const int64_t Kc = std::min<int64_t>(pl.Kc_max, count - c0);
    const int64_t m0 = first + c0;                       // global index of this chunk's first model
    st = ln.load_models(m0, Kc);
    if (st) return st;
    phm::ScwParams sp = {};
    phm::AwParams& p = sp.aw;
    p = ln.params();
    p.Sc = 1;
    for (int64_t k = 0; k < Kc; ++k)
      for (int b = 0; b < E; ++b) formh[(size_t)k * E + b] = phm::sw_form_terms(br.mu[m0 + k] * in.edge_length[b], phm::SW_M_CAP);
    HIPCHK(hipMemcpy(dform.p, formh.data(), sizeof(int32_t) * (size_t)E * Kc, hipMemcpyHostToDevice));
    p.O = dO.as<double>(); p.sO = dsO.as<int32_t>(); p.F = dF.as<double>(); p.sF = dsF.as<int32_t>(); p.lam = dlam.as<double>();
    sp.Q = ln.dQ.as<double>(); sp.t = ln.dt.as<double>(); sp.child = dchild.as<int32_t>(); sp.mu = dmu.as<double>();
    sp.B = dB.as<double>(); sp.form = dform.as<int32_t>();
    sp.runs = drows.as<double>(); sp.tot = drows.as<double>();   // the totals kernels' buffers: their launchers ask for them, no launch here touches them
    HIPCHK(tm.start());
    st = ln.expm();
    if (st) return st;
    HIPCHK(phm::launch_scw_model(sp, nullptr));
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
      const phm::ExDown* down = ddown.as<phm::ExDown>();
      HIPCHK(tm.start());
      st = ln.passes(p);
      if (st) return st;
      st = aw_level_steps(br.down_off, step_max, [&](int k0, int cnt) { return phm::launch_aw_down(p, down + k0, cnt, nullptr); });
      if (st) return st;
      HIPCHK(tm.stop());
      st = ln.fetch_ll(Sc);
      if (st) return st;
      HIPCHK(tm.add_to(kernel_ms));
      auto eval = [&](int64_t k, int64_t s) { return ll_eval_of(in, s0 + s, m0 + k); };
      auto at = [&](int64_t k, int64_t s) { return (size_t)k * Sc + (size_t)s; };
      // an impossible evaluation, or a model whose Pade met a zero pivot: -inf and NaN rows
      auto possible = [&](int64_t k, int64_t s) { return ln.possible(k, at(k, s)); };
      if (loglik)
        for (int64_t k = 0; k < Kc; ++k)
          for (int64_t s = 0; s < Sc; ++s) loglik[eval(k, s)] = possible(k, s) ? ln.llh[at(k, s)] : ninf;
      // rows: [entry][Ev][col]
      st = br_branch_stage(br, ne_max, dsel, dw, drows, dlab, host.get(), Ev, Kc, Sc, (int64_t)Ev * (int64_t)nn, (int64_t)nn, 1, tm, kernel_ms,
                           [&](const int32_t* sel, int ne) { return phm::launch_brw_branch(sp, sel, ne, drows.as<double>(), nullptr); }, at,
                           possible, eval, branch);
      if (st) return st;
    }
  }
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Models are independent: with phm_options.n_devices > 1 device d computes a contiguous range of them (phm_plan_shards,
// run_shards); every output value is the one-device value bit for bit.
int32_t phm_expected_branch_stats_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                         int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const phm_options* opt,
                                         int32_t n_edges, const int32_t* edges, int32_t n_labels, const double* labels,
                                         double* branch, double* loglik) {
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid || !branch)
    return fail(PHM_ERR_BAD_INPUT, BR_FN + "NULL argument (only observe, site_of_model, opt, edges, labels and loglik may be NULL)");
  BrInput br;
  LlInput& in = br.ll;
  int32_t st = ll_validate(BR_FN, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, o, in);
  if (st) return st;
  if (in.n > phm::LL_LANE_MAX && (int64_t)in.S * in.K > (int64_t)INT32_MAX) return fail(PHM_ERR_BAD_INPUT, BR_FN + "sites * models must fit in 31 bits");
  std::string err;
  st = br_select(in.n, in.E, n_edges, edges, n_labels, labels, br.sel, err);
  if (st) return fail(st, BR_FN + err);
  br_model_mu(in.Qr.data(), in.n, in.K, br.mu);
  st = br_check_jump_mean(br.mu, in.edge_length.data(), br.sel, EX_MAX_JUMP_MEAN, err);
  if (st) return fail(st, BR_FN + err);
  br.n_eval = in.paired ? in.K : (int64_t)in.S * in.K;
  ex_down_schedule(in.sched, in.T, br.down, br.down_off, &br.child_row);
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, in.K, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) {
    return in.n <= phm::LL_LANE_MAX ? br_lanes_device(br, sh.device, sh.first, sh.count, branch, loglik)
                                    : br_wide_device(br, sh.device, sh.first, sh.count, branch, loglik);
  });
}

}  // extern "C"
