// phm_sample_wide_api.cpp -- C-ABI of the exact sampler of histories over many rate matrices and sites at 9..64 states
// (phm_sample_histories_models_wide): phm_sample_histories_models' arguments, validation (ll_validate and
// sm_prepare of phm_sample_host.h) and outputs.  Per device and per chunk of models P_k(t_b) by one launch_expm_pade per model and
// the table of mu_k, B_k and beta (a workgroup per model); per chunk of sites section 23's tips / up / root launches; and per
// batch of tiles the root, node-level, branch and finish launches of phm_sample_wide.hip, which read P, L and pid in place.
// Histories are addressed by their global index h = e D + d, so a shard of models is a contiguous range of histories and section
// 14's per-shard map buffers (phm_maps_host.h) serve unchanged.  Every draw is addressed by its global evaluation and draw index
// and every evaluation is independent of every other one, so neither the chunks nor the shards change an output bit.
#include "../../include/phylomap_hip_ext.h"
#include "phm_exp.h"
#include "phm_maps_host.h"
#include "phm_sample_host.h"
#include "phm_sample_wide.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;

const std::string SW_FN = "phm_sample_histories_models_wide: ";
const char* const SW_NAME = "phm_sample_histories_models_wide";

// models [first, first + count) on one device
int32_t sw_device(const SmInput& sm, int32_t device, int64_t first, int64_t count, double* stats, double* loglik,
                  phm_maps::Host* mh, size_t si) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = sm.ll;
  const int n = in.n, E = in.E, NT = in.NT, T = in.T, cols = sm.cols, D = sm.D, NP = phm::aw_lanes(in.n);
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.sites_per_model();
  const int64_t H = sm.H;
  const int tiles_per_eval = (D + 63) / 64;
  const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  const int64_t h_first = ll_eval_of(in, 0, first) * D, h_count = count * S_eval * D;      // the shard's histories
  KernelTimer tm;
  double t_pade = 0.0, t_table = 0.0, t_pass = 0.0, t_sample = 0.0, t_off = 0.0, ms = 0.0;   // device time of the phases
  DevBuf dt, dobs, dup, ddown, dorder, derr;
  HIPCHK(upload(dt, in.edge_length)); HIPCHK(upload(dobs, in.obs)); HIPCHK(upload(dup, in.up));
  HIPCHK(upload(ddown, in.sched.down)); HIPCHK(upload(dorder, sm.order));
  HIPCHK(derr.alloc(sizeof(uint32_t)));
  HIPCHK(hipMemset(derr.p, 0, sizeof(uint32_t)));

  phm::MapsDev maps_dev;
  phm_maps::Shard ms_buf;
  const int64_t map_pad = (h_count + 63) / 64 * 64;
  if (mh) {
    if (h_count > (int64_t)INT32_MAX) return fail(PHM_ERR_UNSUPPORTED, SW_FN + "maps of more than 2^31 - 1 histories on one device");
    st = ms_buf.setup(*mh, h_first, h_count, map_pad, maps_dev);
    if (st) return st;
  }

  int depth_max = 0;
  int64_t k_deep = first;
  for (int64_t k = first; k < first + count; ++k)
    if (sm.depth[k] > depth_max) { depth_max = sm.depth[k]; k_deep = k; }
  const size_t tab_stride = phm::sw_table_doubles(n, depth_max), tab_b = sizeof(double) * tab_stride;

  // Chunks by free HBM.  Once: the Pade workspace of one model and a share of an eighth for the tiles (up to n + n (n - 1)
  // columns of accumulators and output per history: 3.3 MB a tile at 64 states).  Per model: Q, pid, the squaring counts, the
  // error word, P, mu, B, the depth, the table and, when paired, its tips.  Per evaluation: L, sL and ll.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const size_t work_b = sizeof(double) * 5 * nn * (size_t)E;
  const size_t per_tile = (size_t)NT * 64 + 64 * (sizeof(double) * (cols + n) + sizeof(uint32_t) * n * (n - 1)) +
                          (sm.nodes ? sizeof(int32_t) * 64 * (size_t)NT : 0) + sizeof(phm::SmTile);
  const int chunk = g_phm_debug.expect_chunk;
  const int64_t tiles_total = count * S_eval * tiles_per_eval;
  int64_t Tc_max = std::max<int64_t>(1, std::min<int64_t>({tiles_total, (int64_t)(free_b / 8 / per_tile), (int64_t)1 << 20,
                                                            phm::SW_ITEMS_MAX / E}));
  if (chunk > 0) Tc_max = std::min<int64_t>(Tc_max, chunk);
  const size_t fixed_b = work_b + per_tile * (size_t)Tc_max;
  const size_t budget = free_b / 2 > fixed_b ? free_b / 2 - fixed_b : 0;
  const size_t per_model = sizeof(double) * ((size_t)E * nn + 2 * nn + n + 1) + sizeof(int32_t) * ((size_t)E + 1) + sizeof(uint32_t) +
                           (in.paired ? (size_t)T : 0) + tab_b;
  const size_t per_eval = (sizeof(double) * NP + sizeof(int32_t)) * (size_t)NT + sizeof(double);
  if (budget < per_model + per_eval)
    return fail(PHM_ERR_CAPACITY, SW_FN + "model " + std::to_string(k_deep) + ": its table of " + std::to_string(tab_b) + " bytes (" +
                                      std::to_string(depth_max + 1) + " rows of " + std::to_string(nn) + " doubles) does not fit in the " +
                                      std::to_string(budget) + " bytes of HBM this call may use");
  int64_t Sc_max = std::min<int64_t>(S_eval, phm::AW_GRID_MAX);
  int64_t Kc_max = (int64_t)(budget / (per_model + per_eval * (size_t)Sc_max));
  if (Kc_max < 1) {
    Kc_max = 1;
    Sc_max = std::max<int64_t>(1, std::min<int64_t>(Sc_max, (int64_t)((budget - per_model) / per_eval)));
  }
  int step_max = phm::AW_GRID_MAX;                       // level steps of one launch
  if (chunk > 0) {
    Kc_max = std::min<int64_t>(Kc_max, chunk);
    Sc_max = std::min<int64_t>(Sc_max, chunk);
    step_max = std::min(step_max, chunk);
  }
  Kc_max = std::min<int64_t>({Kc_max, count, (int64_t)phm::AW_GRID_MAX});
  const size_t Km = (size_t)Kc_max, Evm = Km * (size_t)Sc_max;

  DevBuf dQ, dpid, dsq, dP, dwork, dbad, dL, dsL, dll, dtips, dmu, dB, dbeta, ddepth, dtile, dnst, ddw, dcnt, dout, dnodes;
  HIPCHK(dQ.alloc(sizeof(double) * nn * Km)); HIPCHK(dpid.alloc(sizeof(double) * n * Km));
  HIPCHK(dsq.alloc(sizeof(int32_t) * (size_t)E * Km)); HIPCHK(dbad.alloc(sizeof(uint32_t) * Km));
  HIPCHK(dP.alloc(sizeof(double) * (size_t)E * nn * Km)); HIPCHK(dwork.alloc(work_b));
  HIPCHK(dL.alloc(sizeof(double) * (size_t)NT * NP * Evm)); HIPCHK(dsL.alloc(sizeof(int32_t) * (size_t)NT * Evm));
  HIPCHK(dll.alloc(sizeof(double) * Evm));
  HIPCHK(dtips.alloc(in.paired ? (size_t)T * Km : (size_t)T * (size_t)Sc_max));
  HIPCHK(dmu.alloc(sizeof(double) * Km)); HIPCHK(dB.alloc(sizeof(double) * nn * Km));
  HIPCHK(dbeta.alloc(tab_b * Km)); HIPCHK(ddepth.alloc(sizeof(int32_t) * Km));
  const size_t npad_max = (size_t)Tc_max * 64;
  HIPCHK(dtile.alloc(sizeof(phm::SmTile) * (size_t)Tc_max)); HIPCHK(dnst.alloc((size_t)NT * npad_max));
  HIPCHK(ddw.alloc(sizeof(unsigned long long) * n * npad_max)); HIPCHK(dcnt.alloc(sizeof(uint32_t) * (size_t)n * (n - 1) * npad_max));
  HIPCHK(dout.alloc(sizeof(double) * cols * npad_max));
  if (sm.nodes) HIPCHK(dnodes.alloc(sizeof(int32_t) * (size_t)NT * npad_max));
  std::vector<double> llh(Evm), outh((size_t)cols * npad_max);
  std::vector<uint8_t> tips_h(in.paired ? (size_t)T * Km : (size_t)T * (size_t)Sc_max);
  std::vector<int32_t> sqh((size_t)E * Km), nodes_h(sm.nodes ? (size_t)NT * npad_max : 0);
  std::vector<uint32_t> badh(Km);
  std::vector<phm::SmTile> tiles;
  tiles.reserve((size_t)Tc_max);

  phm::SwParams sp = {};
  sp.n = n; sp.NP = NP; sp.n_tips = T; sp.n_node = in.Nn; sp.n_edge = E; sp.root_row = T + in.sched.root;
  sp.seed_lo = (uint32_t)(sm.opt.seed & 0xFFFFFFFFull); sp.seed_hi = (uint32_t)(sm.opt.seed >> 32);
  sp.replica = (uint32_t)sm.opt.replica_offset;
  sp.fx_scale = std::ldexp(1.0, 61 - sm.fx_exp); sp.fx_inv = std::ldexp(1.0, sm.fx_exp - 61);
  sp.Q = dQ.as<double>(); sp.P = dP.as<double>(); sp.pid = dpid.as<double>(); sp.L = dL.as<double>(); sp.t = dt.as<double>();
  sp.tiles = dtile.as<phm::SmTile>(); sp.down = ddown.as<phm::DownStep>(); sp.order = dorder.as<int32_t>();
  sp.mu = dmu.as<double>(); sp.B = dB.as<double>(); sp.depth_of = ddepth.as<int32_t>(); sp.tab_stride = tab_stride;
  sp.beta = dbeta.as<double>();
  sp.nstate = dnst.as<uint8_t>(); sp.dwfx = ddw.as<unsigned long long>(); sp.cnt = dcnt.as<uint32_t>();
  sp.out = dout.as<double>(); sp.nodes = sm.nodes ? dnodes.as<int32_t>() : nullptr; sp.err = derr.as<uint32_t>();
  sp.maps = maps_dev; sp.map_pad = map_pad;
  const int maps_mode = mh ? mh->mode : phm::MAPS_OFF;

  // the tiles collected so far: sampled, copied home and scattered into the caller's arrays
  auto flush = [&]() -> int32_t {
    if (tiles.empty()) return PHM_OK;
    const int nt = (int)tiles.size();
    const size_t npad = (size_t)nt * 64;
    sp.n_tiles = nt;
    HIPCHK(hipMemcpy(dtile.p, tiles.data(), sizeof(phm::SmTile) * nt, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(ddw.p, 0, sizeof(unsigned long long) * n * npad));
    HIPCHK(hipMemset(dcnt.p, 0, sizeof(uint32_t) * (size_t)n * (n - 1) * npad));
    HIPCHK(tm.start());
    HIPCHK(phm::launch_sw_sample(sp, sm.level_off, maps_mode, nullptr));
    HIPCHK(tm.stop());
    HIPCHK(hipMemcpy(outh.data(), dout.p, sizeof(double) * cols * npad, hipMemcpyDeviceToHost));
    if (sm.nodes) HIPCHK(hipMemcpy(nodes_h.data(), dnodes.p, sizeof(int32_t) * (size_t)NT * npad, hipMemcpyDeviceToHost));
    uint32_t derrh = 0;
    HIPCHK(hipMemcpy(&derrh, derr.p, sizeof derrh, hipMemcpyDeviceToHost));
    HIPCHK(tm.elapsed(ms));
    t_sample += ms;
    if (derrh & phm::DERR_CAPACITY) return fail(PHM_ERR_CAPACITY, SW_FN + "a branch's jump-count series outgrew the table of its model");
    const int32_t ds = device_status(derrh);
    if (ds) return ds;
    for (int i = 0; i < nt; ++i) {
      const int64_t h0 = h_first + tiles[i].row0;
      const int nv = tiles[i].n_valid;
      for (int c = 0; c < cols; ++c)
        std::copy_n(outh.data() + (size_t)c * npad + (size_t)i * 64, nv, stats + h0 + H * c);
      if (sm.nodes) std::copy_n(nodes_h.data() + (size_t)i * 64 * NT, (size_t)nv * NT, sm.nodes + h0 * NT);
    }
    tiles.clear();
    return PHM_OK;
  };

  for (int64_t c0 = 0; c0 < count; c0 += Kc_max) {
    const int64_t Kc = std::min<int64_t>(Kc_max, count - c0);
    const int64_t m0 = first + c0;                       // global index of this chunk's first model
    for (int64_t k = 0; k < Kc; ++k)
      for (int b = 0; b < E; ++b) sqh[(size_t)k * E + b] = ex_squarings(in.Qr.data() + (size_t)(m0 + k) * nn, n, in.edge_length[b]);
    HIPCHK(hipMemcpy(dQ.p, in.Qr.data() + (size_t)m0 * nn, sizeof(double) * nn * Kc, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dpid.p, in.pid.data() + (size_t)m0 * n, sizeof(double) * n * Kc, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsq.p, sqh.data(), sizeof(int32_t) * (size_t)E * Kc, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ddepth.p, sm.depth.data() + m0, sizeof(int32_t) * Kc, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dbad.p, 0, sizeof(uint32_t) * Kc));
    sp.Kc = (int)Kc;
    HIPCHK(tm.start());
    for (int64_t k = 0; k < Kc; ++k)
      HIPCHK(phm::launch_expm_pade(n, dQ.as<double>() + (size_t)k * nn, dt.as<double>(), dsq.as<int32_t>() + (size_t)k * E, E,
                                   dwork.as<double>(), dP.as<double>() + (size_t)k * E * nn, dbad.as<uint32_t>() + k, nullptr));
    HIPCHK(tm.stop());
    HIPCHK(hipMemcpy(badh.data(), dbad.p, sizeof(uint32_t) * Kc, hipMemcpyDeviceToHost));
    HIPCHK(tm.elapsed(ms));
    t_pade += ms;
    HIPCHK(tm.start());
    HIPCHK(phm::launch_sw_table(sp, nullptr));
    HIPCHK(tm.stop());
    HIPCHK(tm.elapsed(ms));
    t_table += ms;

    phm::AwParams p = {};
    p.n = n; p.NP = NP; p.n_tips = T; p.n_edge = E; p.root = sp.root_row; p.Kc = (int)Kc;
    p.tip_model = in.paired ? 1 : 0; p.tip_site = in.paired ? 0 : 1;
    p.P = dP.as<double>(); p.pid = dpid.as<double>(); p.tips = dtips.as<uint8_t>(); p.obs = dobs.as<int32_t>();
    p.L = dL.as<double>(); p.sL = dsL.as<int32_t>(); p.ll = dll.as<double>();

    for (int64_t s0 = 0; s0 < S_eval; s0 += Sc_max) {
      const int64_t Sc = std::min<int64_t>(Sc_max, S_eval - s0);
      p.Sc = (int)Sc;
      const size_t Ev = (size_t)Sc * Kc;
      sp.Ev = Ev;
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
      HIPCHK(tm.start());
      HIPCHK(phm::launch_aw_tips(p, nullptr));
      for (size_t l = 0; l + 1 < in.up_off.size(); ++l)
        for (int k0 = in.up_off[l]; k0 < in.up_off[l + 1]; k0 += step_max)
          HIPCHK(phm::launch_aw_up(p, up + k0, std::min(step_max, in.up_off[l + 1] - k0), false, nullptr));
      HIPCHK(phm::launch_aw_root(p, nullptr));
      HIPCHK(tm.stop());
      HIPCHK(hipMemcpy(llh.data(), dll.p, sizeof(double) * Ev, hipMemcpyDeviceToHost));
      HIPCHK(tm.elapsed(ms));
      t_pass += ms;
      for (int64_t k = 0; k < Kc; ++k)
        for (int64_t s = 0; s < Sc; ++s) {
          const size_t at = (size_t)k * Sc + s;
          const int64_t site = in.paired ? in.site_of_model[m0 + k] : s0 + s;
          const int64_t ev = ll_eval_of(in, s0 + s, m0 + k);
          // an impossible evaluation (or a model whose Pade met a zero pivot) is not drawn: -inf, NaN rows, zero nodes, empty map rows
          const bool possible = !badh[k] && std::isfinite(llh[at]);
          loglik[ev] = possible ? llh[at] : ninf;
          if (!possible) {
            for (int64_t h = ev * D; h < (ev + 1) * D; ++h) {
              for (int c = 0; c < cols; ++c) stats[h + H * c] = nan;
              if (sm.nodes) std::fill_n(sm.nodes + h * NT, NT, 0);
            }
            continue;
          }
          for (int d0 = 0; d0 < D; d0 += 64) {
            phm::SmTile tl = {};
            tl.ev = (int32_t)at; tl.k = (int32_t)k; tl.eval_id = (uint32_t)(site * in.K + (m0 + k));
            tl.d0 = d0; tl.n_valid = std::min(64, D - d0); tl.row0 = ev * D + d0 - h_first;
            tiles.push_back(tl);
            if ((int64_t)tiles.size() == Tc_max) { st = flush(); if (st) return st; }
          }
        }
      st = flush();                                      // L of this chunk of sites is overwritten by the next
      if (st) return st;
    }
  }
  if (mh) {
    HIPCHK(tm.start());
    HIPCHK(ms_buf.after_kernel(*mh, map_pad, nullptr));  // sizing: counts -> offsets
    HIPCHK(tm.stop());
    HIPCHK(tm.elapsed(ms));
    t_off += ms;
    st = ms_buf.copy_home(*mh, si, SW_NAME);
    if (st) return st;
  }
  if (g_phm_debug.phase_timing)
    std::fprintf(stderr, "phm_sample_histories_models_wide: Pade %.3f ms, table %.3f ms, passes %.3f ms, sampling %.3f ms, map offsets %.3f ms\n",
                 t_pade, t_table, t_pass, t_sample, t_off);
  g_phm_last_kernel_ms = t_pade + t_table + t_pass + t_sample + t_off;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Models are independent and every draw is addressed by its global evaluation and draw index: with phm_options.n_devices > 1
// device d samples a contiguous range of the models (phm_plan_shards, run_shards), and every output is the one-device output bit
// for bit.
int32_t phm_sample_histories_models_wide(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                         int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, int32_t draws,
                                         const phm_options* opt, double* stats, double* loglik, int32_t* nodes,
                                         int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state) {
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid || !stats || !loglik)
    return fail(PHM_ERR_BAD_INPUT, SW_FN + "NULL argument (only observe, site_of_model, opt, nodes and the map arrays may be NULL)");
  SmInput sm;
  int32_t st = ll_validate(SW_FN, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, o, sm.ll);
  if (st) return st;
  sm.opt = o; sm.nodes = nodes;
  st = sm_prepare(SW_FN, phm::AW_MIN_STATES, phm::EX_MAX_STATES, "9..64 states only: 2..8 states go to phm_sample_histories_models", sm, draws);
  if (st) return st;
  const bool want_maps = map_off || map_dwell || map_state;
  phm_maps::Host mh;
  if (want_maps) {
    st = phm_maps::validate(SW_NAME, sm.H, x->n_edge, map_off, map_cap, map_dwell, map_state, mh);
    if (st) return st;
  }
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, sm.ll.K, shards);
  if (st) return st;
  mh.shard_total.assign(shards.size(), 0);
  st = run_shards(shards, [&](const phm_shard& sh, size_t i) {
    return sw_device(sm, sh.device, sh.first, sh.count, stats, loglik, want_maps ? &mh : nullptr, i);
  });
  if (st) return st;
  if (want_maps) {
    // finish_sizing works in units of histories: a shard of models is histories [e(first) D, e(first + count) D)
    std::vector<phm_shard> hs = shards;
    const int64_t per_model = (sm.ll.paired ? 1 : (int64_t)sm.ll.S) * sm.D;
    for (phm_shard& s : hs) { s.first *= per_model; s.count *= per_model; }
    phm_maps::finish_sizing(mh, hs);
  }
  return PHM_OK;
}

}  // extern "C"
