// phm_gibbs_wide_api.cpp -- C-ABI of the batched posterior sampler of the rates of an index model at 9..64 states
// (phm_gibbs_rates_wide): phm_gibbs_rates' arguments, validation (gb_validate of phm_gibbs_host.h) and
// outputs.  Iteration i of chain k: Q_k = Q(theta_k) into section 23's buffers (AwLanes::set_models), P_k(t_b) by one Pade launch
// per chain, the table of mu_k, B_k and beta to the chain's own depth, the tips / up / root launches, one exact history per
// evaluation by phm_sample_wide.hip's kernels in their sites form (a tile is 64 consecutive sites of ONE chain, lane = site), and
// on the device the finish and the sum of every chain's columns over its sites; then, on the host, the conjugate Gamma draw of
// every rate from the chain's SUMMED row alone.  A chunk of chains runs all its iterations on buffers allocated once; per
// iteration there is one upload (Q, squaring counts, depths) and one download of Kc (cols + 1) + 1 doubles.
// Every random number is addressed by global indices only: histories by (site * C + chain, iteration + replica_offset) as
// phm_sample_histories_models_wide with draws = 1 addresses them, rates by (ENT_RATE | parameter, chain, iteration + replica_offset).
#include "phm_ancestral_wide_host.h"
#include "phm_gibbs_host.h"
#include "phm_sample_wide.h"

namespace {

using namespace phm_ex;
using namespace phm_ll;

const std::string GW_FN = "phm_gibbs_rates_wide: ";

int32_t gw_device(const GbInput& g, int32_t device, int64_t first, int64_t count) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = g.ll;
  const int n = in.n, E = in.E, NT = in.NT, cols = g.cols, np = g.p;
  const size_t nn = (size_t)n * n;
  const int64_t C = in.K;
  const int64_t S_eval = in.sites_per_model();           // sites per chain
  const int tpc = (int)((S_eval + 63) / 64);             // tiles per chain: 64 consecutive sites each
  const double nan = std::numeric_limits<double>::quiet_NaN();
  KernelTimer tm;
  double kernel_ms = 0.0, pade_ms = 0.0;
  const bool q_timing = g_phm_debug.q_timing != 0;      // host clock of the phases of an iteration, printed to stderr
  double up_ms = 0.0, run_ms = 0.0, host_ms = 0.0;
  int launches = 0, threads_used = 1;
  AwLanes ln(in);
  DevBuf ddown, dorder, derr;
  st = ln.upload_tree();
  if (st) return st;
  HIPCHK(upload(ddown, in.sched.down)); HIPCHK(upload(dorder, g.order));
  HIPCHK(derr.alloc(sizeof(uint32_t)));
  HIPCHK(hipMemset(derr.p, 0, sizeof(uint32_t)));

  // Chunks of chains by free HBM, on top of section 23's footprint.  Per chain: mu, B, the depth, the table (to the depth theta_max
  // allows) and the reduced row; per evaluation its share of the chain's tiles (node states and accumulators of 64 lanes each).
  // Every site of a chain sits in the chunk: the reduction sums over them every iteration.
  const size_t tab_stride = phm::sw_table_doubles(n, g.depth), tab_b = sizeof(double) * tab_stride;
  const size_t tile_b = (size_t)NT * 64 + 64 * (sizeof(unsigned long long) * n + sizeof(uint32_t) * n * (n - 1)) + sizeof(phm::SmTile);
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  AwPlan pl = aw_plan(free_b, in, count, 0, sizeof(double), sizeof(double) * (nn + 1 + cols + 1) + sizeof(int32_t) + tab_b,
                      (tile_b * tpc + (size_t)S_eval - 1) / (size_t)S_eval);
  if (pl.budget < pl.per_model + pl.per_eval)            // before anything of the plan is used: not one evaluation fits
    return fail(PHM_ERR_CAPACITY, GW_FN + "a chain's table of " + std::to_string(tab_b) + " bytes (" + std::to_string(g.depth + 1) +
                                      " rows of " + std::to_string(nn) + " doubles, the depth theta_max allows) does not fit in the " +
                                      std::to_string(pl.budget) + " bytes of HBM this call may use; lower theta_max");
  if (pl.Sc_max < S_eval) return fail(PHM_ERR_OOM, GW_FN + "one chain with all its sites does not fit the device; run fewer sites per call");
  pl.Kc_max = std::min<int64_t>({pl.Kc_max, phm::SW_ITEMS_MAX / E / tpc, ((int64_t)1 << 24) / S_eval});   // grid of the branch launch; 32-bit offsets
  const int chunk = g_phm_debug.expect_chunk;
  if (chunk > 0) { pl.Kc_max = std::min<int64_t>(pl.Kc_max, chunk); pl.step_max = std::min(pl.step_max, chunk); }
  const size_t Km = (size_t)pl.Kc_max, Tm = Km * (size_t)tpc;

  SwModels md;
  DevBuf dtile, dnst, ddw, dcnt, dred;
  st = ln.alloc(pl);
  if (st) return st;
  st = md.alloc(n, Km, tab_stride);
  if (st) return st;
  HIPCHK(dtile.alloc(sizeof(phm::SmTile) * Tm)); HIPCHK(dnst.alloc((size_t)NT * 64 * Tm));
  HIPCHK(ddw.alloc(sizeof(unsigned long long) * n * 64 * Tm)); HIPCHK(dcnt.alloc(sizeof(uint32_t) * (size_t)n * (n - 1) * 64 * Tm));
  const size_t red_max = (size_t)(cols + 1) * Km + 1;
  HIPCHK(dred.alloc(sizeof(double) * red_max));
  PinnedBuf hQ, hsq, hdepth, hred;                       // the per-iteration copies go through page-locked memory
  HIPCHK(hQ.reserve(sizeof(double) * nn * Km)); HIPCHK(hsq.reserve(sizeof(int32_t) * (size_t)E * Km));
  HIPCHK(hdepth.reserve(sizeof(int32_t) * Km)); HIPCHK(hred.reserve(sizeof(double) * red_max));
  double* Qh = hQ.as<double>();
  int32_t* sqh = hsq.as<int32_t>();
  int32_t* depth_h = hdepth.as<int32_t>();
  const double* redh = hred.as<double>();
  std::vector<double> th((size_t)np * Km), nan_row((size_t)S_eval, nan);
  std::vector<phm::SmTile> tiles(Tm);

  phm::SwParams sp = {};
  phm::SmCore& sc = sp.core;
  sm_fill_core(sc, in, g.opt, g.fx_exp);                 // replica: the iteration's, below
  sc.tiles = dtile.as<phm::SmTile>(); sc.down = ddown.as<phm::DownStep>(); sc.order = dorder.as<int32_t>();
  sc.nstate = dnst.as<uint8_t>(); sc.dwfx = ddw.as<unsigned long long>(); sc.cnt = dcnt.as<uint32_t>();
  sc.out = nullptr; sc.nodes = nullptr; sc.err = derr.as<uint32_t>();
  md.fill(sp, ln);
  sp.ll = ln.dll.as<double>(); sp.lane_stride = (uint32_t)C;

  for (int64_t c0 = 0; c0 < count; c0 += pl.Kc_max) {
    const int64_t Kc = std::min<int64_t>(pl.Kc_max, count - c0);
    const int64_t m0 = first + c0;                       // global index of this chunk's first chain
    st = ln.load_models(m0, Kc);                         // pid; Q is this driver's own: Qh, uploaded every iteration
    if (st) return st;
    // what the device needs of chain k's rates: Q(theta_k), its squaring counts and the depth of its table.  mu_k <= (most rates
    // in a row) * theta_max up to rounding, so the depth is at most g.depth; the kernels raise DERR_CAPACITY beyond a table's end
    auto stage = [&](int64_t k) {
      double* Qk = Qh + (size_t)k * nn;
      fill_q(g, &th[(size_t)k * np], Qk, 1);
      double mu = 0.0;
      for (int i = 0; i < n; ++i) mu = std::max(mu, -Qk[(size_t)i * n + i]);
      depth_h[k] = std::min(phm::sm_stop_index(mu * g.t_max), g.depth);
      for (int b = 0; b < E; ++b) sqh[(size_t)k * E + b] = ex_squarings(Qk, n, in.edge_length[b]);
    };
    for (int64_t k = 0; k < Kc; ++k) {
      std::copy_n(g.theta0 + (size_t)(m0 + k) * np, np, th.begin() + (size_t)k * np);
      stage(k);
    }
    const int nt = (int)(Kc * tpc);
    for (int64_t k = 0; k < Kc; ++k)
      for (int j = 0; j < tpc; ++j) {                    // sites 64 j .. of chain k: evaluations k * S_eval + 64 j ..
        const int64_t site0 = in.paired ? in.site_of_model[m0 + k] : (int64_t)64 * j;
        phm::SmTile tl = {};
        tl.ev = (int32_t)(k * S_eval + 64 * j); tl.k = (int32_t)k; tl.eval_id = (uint32_t)(site0 * C + (m0 + k));
        tl.n_valid = (int32_t)std::min<int64_t>(64, S_eval - (int64_t)64 * j);
        tiles[(size_t)k * tpc + j] = tl;
      }
    st = ln.stage_tips(0, S_eval);
    if (st) return st;
    HIPCHK(hipMemcpy(dtile.p, tiles.data(), sizeof(phm::SmTile) * nt, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(ddw.p, 0, sizeof(unsigned long long) * n * 64 * nt));
    HIPCHK(hipMemset(dcnt.p, 0, sizeof(uint32_t) * (size_t)n * (n - 1) * 64 * nt));
    phm::AwParams p = ln.params();
    p.Sc = (int)S_eval;
    sp.Kc = (int)Kc; sp.Ev = (size_t)S_eval * Kc;
    sc.n_tiles = nt;
    const size_t red_n = (size_t)(cols + 1) * Kc + 1;

    // The update of chains [k_lo, k_hi) of the chunk from the iteration's download, row T of chain k at redh + k (cols + 1): one
    // pass over the off-diagonal entries in row-major order, N_c += T[n + i (n - 1) + (j > i ? j - 1 : j)] and W_c += T[i] for
    // c = index[i, j], then the draws for c ascending.
    auto update = [&](int iter, int64_t k_lo, int64_t k_hi) {
      std::vector<double> Nc(np), Wc(np);
      for (int64_t k = k_lo; k < k_hi; ++k) {
        const int64_t ch = m0 + k;
        double* thk = &th[(size_t)k * np];
        const double* T = redh + (size_t)k * (cols + 1);
        const double ll = T[cols];
        if (!g.status[ch] && (ln.badh[k] || !std::isfinite(ll))) g.status[ch] = 1;
        if (!gb_record(g, iter, ch, thk, ll, [&](int c) { return T[c]; })) continue;   // an impossible chain: its rates stay as they are
        std::fill(Nc.begin(), Nc.end(), 0.0); std::fill(Wc.begin(), Wc.end(), 0.0);
        for (int i = 0; i < n; ++i)
          for (int j = 0; j < n; ++j) {
            const int c = g.index[(size_t)i * n + j];    // 0 on the diagonal and for a structural zero
            if (c < 1) continue;
            Nc[c - 1] += T[n + i * (n - 1) + (j > i ? j - 1 : j)];
            Wc[c - 1] += T[i];
          }
        for (int c = 0; c < np; ++c) gb_draw(g, iter, ch, c, Nc[c], Wc[c], thk);
        stage(k);
      }
    };
    // a chain's update is O(n^2) and its squaring counts O(n^2 E)
    const int n_threads = (int)std::max<int64_t>(1, std::min<int64_t>({16, Kc, (int64_t)(Kc * nn * E >> 18)}));
    threads_used = std::max(threads_used, n_threads);

    for (int iter = 0; iter < g.iters; ++iter) {
      sc.replica = (uint32_t)iter + (uint32_t)g.opt.replica_offset;
      GbLap lap;
      st = ln.set_models(Qh, sqh);
      if (st) return st;
      HIPCHK(hipMemcpy(md.ddepth.p, depth_h, sizeof(int32_t) * Kc, hipMemcpyHostToDevice));
      lap(up_ms);
      HIPCHK(tm.start());
      st = ln.expm();
      if (st) return st;
      HIPCHK(tm.stop());
      st = ln.fetch_bad();
      if (st) return st;
      HIPCHK(tm.add_to(pade_ms));
      HIPCHK(tm.start());
      HIPCHK(phm::launch_sw_table(sp, nullptr));
      st = ln.passes(p);
      if (st) return st;
      for (int64_t k = 0; k < Kc; ++k)                   // a chain whose Pade met a zero pivot: its lanes idle, whatever P holds
        if (ln.badh[k]) HIPCHK(hipMemcpy(ln.dll.as<double>() + (size_t)k * S_eval, nan_row.data(), sizeof(double) * S_eval, hipMemcpyHostToDevice));
      HIPCHK(phm::launch_sw_sample_sites(sp, g.level_off, (int)S_eval, tpc, dred.as<double>(), nullptr));
      HIPCHK(tm.stop());
      HIPCHK(hipMemcpy(hred.p, dred.p, sizeof(double) * red_n, hipMemcpyDeviceToHost));
      HIPCHK(tm.add_to(kernel_ms));
      lap(run_ms);
      const uint32_t derrh = (uint32_t)redh[red_n - 1];
      if (derrh & phm::DERR_CAPACITY) return fail(PHM_ERR_CAPACITY, GW_FN + "a chain's jump-count series outgrew the table theta_max allows");
      const int32_t ds = device_status(derrh);
      if (ds) return ds;
      deal_ranges(Kc, n_threads, [&](int64_t k_lo, int64_t k_hi) { update(iter, k_lo, k_hi); });
      lap(host_ms);
    }
    int levels = 0;
    for (size_t l = 0; l + 1 < g.level_off.size(); ++l) levels += g.level_off[l + 1] > g.level_off[l] ? 1 : 0;
    launches = (int)Kc + 3 + (int)in.up_off.size() - 1 + 3 + levels;   // P per chain, table, tips, up levels, root | root, node levels, branch, reduce
  }
  kernel_ms += pade_ms;
  if (q_timing)
    std::fprintf(stderr, "phm_gibbs_rates_wide: device %d, chains %lld, per iteration: upload of Q %.4f ms, launches + device + download %.4f ms "
                 "(device %.4f ms, of which Pade %.4f ms), host update %.4f ms on %d thread(s); %d launches per iteration\n", (int)device,
                 (long long)count, up_ms / g.iters, run_ms / g.iters, kernel_ms / g.iters, pade_ms / g.iters, host_ms / g.iters,
                 threads_used, launches);
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Chains are independent and every random number is addressed by global indices: with phm_options.n_devices > 1 device d runs a
// contiguous range of the chains (phm_plan_shards, run_shards), and every output is the one-device output bit for bit.
int32_t phm_gibbs_rates_wide(const phm_tree* x, int32_t n_states, const int32_t* index, int32_t n_params, int32_t n_chains,
                             const double* theta0, const double* prior, int32_t n_prior, double theta_max, const double* pid,
                             int32_t n_pid, const int32_t* observe, const int32_t* site_of_chain, int32_t iters, int32_t thin,
                             const phm_options* opt, double* theta, double* loglik, double* stats, int32_t* rejected,
                             int32_t* chain_status) {
  const phm_options o = resolve_options(opt);
  GbInput g;
  int32_t st = gb_validate(GW_FN, true, x, n_states, index, n_params, n_chains, theta0, prior, n_prior, theta_max, pid, n_pid, observe,
                           site_of_chain, iters, thin, o, theta, loglik, stats, rejected, chain_status, g);
  if (st) return st;
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, g.ll.K, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) { return gw_device(g, sh.device, sh.first, sh.count); });
}

}  // extern "C"
