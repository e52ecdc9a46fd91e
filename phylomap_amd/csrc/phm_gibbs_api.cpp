// phm_gibbs_api.cpp -- C-ABI of the batched posterior sampler of the rates of an index model by exact data augmentation
// (phm_gibbs_rates).  C chains run in lock-step, one chain per lane.  Iteration i of chain k: Q_k = Q(theta_k),
// section 17's P, tips, up and root launches, unchanged, on the chunk's buffers; one exact history per evaluation by section 19's
// kernels in their packed form (phm_sample.hip, lane = chain); then, on the host, the conjugate Gamma draw of every rate from the
// history's counts and dwell times (HostStream::gamma of phm_qupdate.h).  A chunk of chains runs ALL its iterations on buffers
// allocated once; per iteration there is one upload (Q) and one download (statistics, log-likelihoods and the error word).
// Every random number is addressed by global indices only: histories by (site * C + chain, iteration + replica_offset) as
// phm_sample_histories_models with draws = 1 addresses them, rates by (ENT_RATE | parameter, chain, iteration + replica_offset).
#include "phm_gibbs_host.h"

namespace {

using namespace phm_ex;
using namespace phm_ll;

const std::string GB_FN = "phm_gibbs_rates: ";

int32_t gb_device(const GbInput& g, int32_t device, int64_t first, int64_t count) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = g.ll;
  const int n = in.n, E = in.E, NT = in.NT, T = in.T, cols = g.cols, np = g.p;
  const size_t nn = (size_t)n * n;
  const int64_t C = in.K;
  const int64_t S_eval = in.sites_per_model();           // sites per chain
  KernelTimer tm;
  double kernel_ms = 0.0;
  const bool q_timing = g_phm_debug.q_timing != 0;      // host clock of the phases of an iteration, printed to stderr
  double up_ms = 0.0, run_ms = 0.0, host_ms = 0.0;
  int launches = 0;
  LlLanes ln(in);
  DevBuf ddown, dorder, derr;
  st = ln.upload_tree();
  if (st) return st;
  HIPCHK(upload(ddown, in.sched.down)); HIPCHK(upload(dorder, g.order));
  HIPCHK(derr.alloc(sizeof(uint32_t)));
  HIPCHK(hipMemset(derr.p, 0, sizeof(uint32_t)));

  // Chunks of chains by free HBM: section 17's buffers and the table (to the depth theta_max allows) per chain, and per evaluation
  // L, sL, ll and the sampler's lane.  Every site of a chain sits in the chunk (joint mode sums over them every iteration).
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const bool ws = n > phm::LL_REG_MAX;
  const size_t budget = free_b / 2 > (ws ? LL_WORK : 0) ? free_b / 2 - (ws ? LL_WORK : 0) : 0;
  const size_t per_model = sizeof(double) * ((size_t)E * nn + 2 * nn + n + 1 + ((size_t)g.depth + 1) * nn) + sizeof(uint32_t) + sizeof(int32_t);
  const size_t per_eval = sizeof(double) * ((size_t)NT * (n + 1) + 1) + (in.paired ? (size_t)T : 0) + (size_t)NT +
                          sizeof(double) * (cols + 1 + n) + sizeof(uint32_t) * ((size_t)n * (n - 1) + 1);
  int64_t Kc_max = (int64_t)(budget / (per_model + per_eval * (size_t)S_eval)) / 64 * 64;
  Kc_max = std::min<int64_t>(Kc_max, ((int64_t)1 << 22) / S_eval / 64 * 64);       // evaluations of a chunk: 32-bit offsets
  if (Kc_max < 64) return fail(PHM_ERR_OOM, GB_FN + "64 chains with all their sites do not fit the device; run fewer sites per call");
  const int chunk = g_phm_debug.expect_chunk;
  if (chunk > 0) Kc_max = std::min<int64_t>(Kc_max, ((int64_t)chunk + 63) / 64 * 64);
  Kc_max = std::min<int64_t>(Kc_max, (count + 63) / 64 * 64);
  const size_t Kpm = (size_t)Kc_max, Evm = Kpm * (size_t)S_eval;
  LlPlan pl;
  pl.Kc_max = Kc_max; pl.Sc_max = S_eval; pl.ne_max = ll_edges_per_launch(n, E, Kpm, chunk);

  DevBuf dmu, dB, dbeta, ddepth, dtile, dlane, dnst, ddw, dcnt, dout;
  st = ln.alloc(pl);
  if (st) return st;
  HIPCHK(dmu.alloc(sizeof(double) * Kpm)); HIPCHK(dB.alloc(sizeof(double) * nn * Kpm));
  HIPCHK(dbeta.alloc(sizeof(double) * ((size_t)g.depth + 1) * nn * Kpm)); HIPCHK(ddepth.alloc(sizeof(int32_t) * Kpm));
  HIPCHK(dtile.alloc(sizeof(phm::SmTile) * (Evm / 64))); HIPCHK(dlane.alloc(sizeof(uint32_t) * Evm));
  HIPCHK(dnst.alloc((size_t)NT * Evm));
  HIPCHK(ddw.alloc(sizeof(unsigned long long) * n * Evm)); HIPCHK(dcnt.alloc(sizeof(uint32_t) * (size_t)n * (n - 1) * Evm));
  const size_t out_max = (size_t)(cols + 1) * Evm + 1;
  HIPCHK(dout.alloc(sizeof(double) * out_max));
  PinnedBuf hQ, hout;                                    // the two per-iteration copies go through page-locked memory
  HIPCHK(hQ.reserve(sizeof(double) * nn * Kpm)); HIPCHK(hout.reserve(sizeof(double) * out_max));
  double* Qh = hQ.as<double>();
  const double* outh = hout.as<double>();
  std::vector<double> th((size_t)np * Kpm);
  std::vector<phm::SmTile> tiles(Evm / 64);
  std::vector<uint32_t> lane_id(Evm);

  phm::SmParams sp = {};
  phm::LlParams& p = sp.ll;
  phm::SmCore& sc = sp.core;
  sm_fill_core(sc, in, g.opt, g.fx_exp);                 // replica: the iteration's, below
  sc.tiles = dtile.as<phm::SmTile>(); sc.down = ddown.as<phm::DownStep>(); sc.order = dorder.as<int32_t>();
  sc.nstate = dnst.as<uint8_t>(); sc.dwfx = ddw.as<unsigned long long>(); sc.cnt = dcnt.as<uint32_t>();
  sc.out = dout.as<double>(); sc.nodes = nullptr; sc.err = derr.as<uint32_t>();
  sp.mu = dmu.as<double>(); sp.B = dB.as<double>(); sp.beta = dbeta.as<double>(); sp.depth_of = ddepth.as<int32_t>();
  sp.packed = 1; sp.t_max = g.t_max; sp.depth = g.depth; sp.lane_id = dlane.as<uint32_t>();

  for (int64_t c0 = 0; c0 < count; c0 += Kc_max) {
    const int64_t Kc = std::min<int64_t>(Kc_max, count - c0);
    st = ln.load_priors(first + c0, Kc);                 // Q is this driver's own: filled into Qh, uploaded every iteration
    if (st) return st;
    const int Kp = ln.Kp;
    const int64_t m0 = ln.m0;                            // global index of this chunk's first chain
    const size_t npad = (size_t)S_eval * Kp;             // lanes of the chunk: evaluation s * Kp + k is lane s * Kp + k
    const int nt = (int)(npad / 64);
    std::fill(Qh, Qh + nn * Kp, 0.0);
    for (int64_t k = 0; k < Kc; ++k) {
      std::copy_n(g.theta0 + (size_t)(m0 + k) * np, np, th.begin() + (size_t)k * np);
      fill_q(g, &th[(size_t)k * np], Qh + k, (size_t)Kp);
    }
    for (int64_t s = 0; s < S_eval; ++s)
      for (int k0 = 0; k0 < Kp; k0 += 64) {
        phm::SmTile tl = {};
        tl.ev = (int32_t)(s * Kp + k0); tl.k = k0; tl.n_valid = 64;
        tiles[(size_t)(s * Kp + k0) / 64] = tl;
        for (int l = 0; l < 64; ++l) {
          const int64_t k = k0 + l;
          const int64_t site = k < Kc ? (in.paired ? in.site_of_model[m0 + k] : s) : 0;
          lane_id[(size_t)(s * Kp + k)] = k < Kc ? (uint32_t)(site * C + (m0 + k)) : phm::SM_LANE_IDLE;
        }
      }
    st = ln.stage_tips(0, S_eval);
    if (st) return st;
    HIPCHK(hipMemcpy(dtile.p, tiles.data(), sizeof(phm::SmTile) * nt, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dlane.p, lane_id.data(), sizeof(uint32_t) * npad, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(ddw.p, 0, sizeof(unsigned long long) * n * npad));
    HIPCHK(hipMemset(dcnt.p, 0, sizeof(uint32_t) * (size_t)n * (n - 1) * npad));
    p = ln.params();
    sc.n_tiles = nt;
    const int branch_blocks = (int)std::min<int64_t>(((int64_t)E * nt + 3) / 4, 2048);
    const size_t out_n = (size_t)(cols + 1) * npad + 1;

    // the update of chains [k_lo, k_hi) of the chunk from the iteration's download
    auto update = [&](int iter, int64_t k_lo, int64_t k_hi) {
      for (int64_t k = k_lo; k < k_hi; ++k) {
        const int64_t ch = m0 + k;
        double* thk = &th[(size_t)k * np];
        auto over_sites = [&](int c) {                   // column c of the download summed over the chain's sites, ascending
          double v = 0.0;
          for (int64_t s = 0; s < S_eval; ++s) v += outh[(size_t)c * npad + (size_t)(s * Kp + k)];
          return v;
        };
        const double ll = over_sites(cols);
        if (!g.status[ch] && !std::isfinite(ll)) g.status[ch] = 1;
        if (!gb_record(g, iter, ch, thk, ll, over_sites)) continue;   // an impossible chain: its lanes idle on the device
        for (int c = 0; c < np; ++c) {
          double Nc = 0.0, Wc = 0.0;                     // W_c: sites ascending, within a site the entries in row-major order
          for (int64_t s = 0; s < S_eval; ++s) {
            const size_t ln = (size_t)(s * Kp + k);
            for (int i = 0; i < n; ++i)
              for (int j = 0; j < n; ++j) {
                if (g.index[(size_t)i * n + j] != c + 1) continue;
                Nc += outh[(size_t)(n + i * (n - 1) + (j > i ? j - 1 : j)) * npad + ln];
                Wc += outh[(size_t)i * npad + ln];
              }
          }
          gb_draw(g, iter, ch, c, Nc, Wc, thk);
        }
        fill_q(g, thk, Qh + k, (size_t)Kp);
      }
    };
    const int n_threads = (int)std::max<int64_t>(1, std::min<int64_t>(16, Kc * np / 4096));

    for (int iter = 0; iter < g.iters; ++iter) {
      sc.replica = (uint32_t)iter + (uint32_t)g.opt.replica_offset;
      GbLap lap;
      HIPCHK(hipMemcpy(ln.dQ.p, Qh, sizeof(double) * nn * Kp, hipMemcpyHostToDevice));
      lap(up_ms);
      HIPCHK(tm.start());
      p.n_sites = 1;
      st = ln.expm(p);
      if (st) return st;
      HIPCHK(phm::launch_sm_table(sp, nullptr));
      p.n_sites = (int)S_eval;
      st = ln.passes(p);
      if (st) return st;
      HIPCHK(phm::launch_sm_sample(sp, g.level_off, branch_blocks, phm::MAPS_OFF, nullptr));
      HIPCHK(tm.stop());
      HIPCHK(hipMemcpy(hout.p, dout.p, sizeof(double) * out_n, hipMemcpyDeviceToHost));
      HIPCHK(tm.add_to(kernel_ms));
      lap(run_ms);
      const uint32_t derrh = (uint32_t)outh[out_n - 1];
      if (derrh & phm::DERR_CAPACITY) return fail(PHM_ERR_CAPACITY, GB_FN + "a chain's jump-count series outgrew the table theta_max allows");
      const int32_t ds = device_status(derrh);
      if (ds) return ds;
      deal_ranges(Kc, n_threads, [&](int64_t k_lo, int64_t k_hi) { update(iter, k_lo, k_hi); });
      lap(host_ms);
    }
    int levels = 0;
    for (size_t l = 0; l + 1 < g.level_off.size(); ++l) levels += g.level_off[l + 1] > g.level_off[l] ? 1 : 0;
    launches = (E + pl.ne_max - 1) / pl.ne_max + 3 + (int)in.up_off.size() - 1 + 3 + levels;   // P, table, tips, up levels, root | root, node levels, branch, finish
  }
  if (q_timing)
    std::fprintf(stderr, "phm_gibbs_rates: device %d, chains %lld, per iteration: upload of Q %.4f ms, launches + device + download %.4f ms "
                 "(device %.4f ms), host update %.4f ms on %d thread(s); %d launches per iteration\n", (int)device, (long long)count,
                 up_ms / g.iters, run_ms / g.iters, kernel_ms / g.iters, host_ms / g.iters,
                 (int)std::max<int64_t>(1, std::min<int64_t>(16, std::min<int64_t>(Kc_max, count) * np / 4096)), launches);
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Chains are independent and every random number is addressed by global indices: with phm_options.n_devices > 1 device d runs a
// contiguous range of the chains (phm_plan_shards, run_shards), and every output is the one-device output bit for bit.
int32_t phm_gibbs_rates(const phm_tree* x, int32_t n_states, const int32_t* index, int32_t n_params, int32_t n_chains,
                        const double* theta0, const double* prior, int32_t n_prior, double theta_max, const double* pid,
                        int32_t n_pid, const int32_t* observe, const int32_t* site_of_chain, int32_t iters, int32_t thin,
                        const phm_options* opt, double* theta, double* loglik, double* stats, int32_t* rejected,
                        int32_t* chain_status) {
  const phm_options o = resolve_options(opt);
  GbInput g;
  int32_t st = gb_validate(GB_FN, false, x, n_states, index, n_params, n_chains, theta0, prior, n_prior, theta_max, pid, n_pid, observe,
                           site_of_chain, iters, thin, o, theta, loglik, stats, rejected, chain_status, g);
  if (st) return st;
  const LlInput& in = g.ll;

  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, in.K, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) { return gb_device(g, sh.device, sh.first, sh.count); });
}

}  // extern "C"
