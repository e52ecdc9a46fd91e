// phm_sample_api.cpp -- C-ABI of the exact sampler of histories over many rate matrices and sites
// (phm_sample_histories_models): phm_loglik_models' validation (ll_validate), then per device and per chunk
// of models P_k(t_b) (section 17) and the table of mu_k, B_k and beta; per chunk of sites section 17's tips / up / root launches;
// and per batch of tiles the root, node-level, branch and finish launches of phm_sample.hip, which read P, L and pid in place.
// Histories are addressed by their global index h = e D + d (e: the evaluation's index into loglik), so a shard of models is a
// contiguous range of histories and section 14's per-shard map buffers (phm_maps_host.h) serve unchanged.
#include "phm_maps_host.h"
#include "phm_sample_host.h"

#include <limits>

namespace {

using namespace phm_ex;
using namespace phm_ll;

const std::string SM_FN = "phm_sample_histories_models: ";

int32_t sm_device(const SmInput& sm, int32_t device, int64_t first, int64_t count, double* stats, double* loglik,
                  phm_maps::Host* mh, size_t si) {
  int32_t st = select_device(device);
  if (st) return st;
  const LlInput& in = sm.ll;
  const int n = in.n, E = in.E, NT = in.NT, T = in.T, cols = sm.cols, D = sm.D;
  const size_t nn = (size_t)n * n;
  const int64_t S_eval = in.sites_per_model();
  const int64_t H = sm.H;
  const int tiles_per_eval = (D + 63) / 64;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const int64_t h_first = ll_eval_of(in, 0, first) * D, h_count = count * S_eval * D;      // the shard's histories
  KernelTimer tm;
  double kernel_ms = 0.0, ms = 0.0;
  LlLanes ln(in);
  DevBuf ddown, dorder, derr;
  st = ln.upload_tree();
  if (st) return st;
  HIPCHK(upload(ddown, in.sched.down)); HIPCHK(upload(dorder, sm.order));
  HIPCHK(derr.alloc(sizeof(uint32_t)));
  HIPCHK(hipMemset(derr.p, 0, sizeof(uint32_t)));

  phm::MapsDev maps_dev;
  phm_maps::Shard ms_buf;
  const int64_t map_pad = (h_count + 63) / 64 * 64;
  if (mh) {
    if (h_count > (int64_t)INT32_MAX) return fail(PHM_ERR_UNSUPPORTED, SM_FN + "maps of more than 2^31 - 1 histories on one device");
    st = ms_buf.setup(*mh, h_first, h_count, map_pad, maps_dev);
    if (st) return st;
  }

  int depth_max = 0;
  for (int64_t k = first; k < first + count; ++k) depth_max = std::max(depth_max, sm.depth[k]);

  // On top of section 17's footprint: mu, B, the table and its depth per model, and a fixed share for the tiles.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const size_t per_tile = (size_t)NT * 64 + 64 * (sizeof(double) * (cols + n) + sizeof(uint32_t) * n * (n - 1)) +
                          (sm.nodes ? sizeof(int32_t) * 64 * (size_t)NT : 0) + sizeof(phm::SmTile);
  const int chunk = g_phm_debug.expect_chunk;
  const int64_t tiles_total = count * S_eval * tiles_per_eval;
  int64_t Tc_max = std::max<int64_t>(1, std::min<int64_t>({tiles_total, (int64_t)(free_b / 8 / per_tile), (int64_t)1 << 20}));
  if (chunk > 0) Tc_max = std::min<int64_t>(Tc_max, chunk);
  const LlPlan pl = ll_plan(free_b, in, count, chunk, per_tile * (size_t)Tc_max,
                            sizeof(double) * (nn + 1 + ((size_t)depth_max + 1) * nn) + sizeof(int32_t), 0);
  const size_t Kpm = (size_t)pl.Kc_max;

  DevBuf dmu, dB, dbeta, ddepth, dtile, dnst, ddw, dcnt, dout, dnodes;
  st = ln.alloc(pl);
  if (st) return st;
  HIPCHK(dmu.alloc(sizeof(double) * Kpm)); HIPCHK(dB.alloc(sizeof(double) * nn * Kpm));
  HIPCHK(dbeta.alloc(sizeof(double) * ((size_t)depth_max + 1) * nn * Kpm)); HIPCHK(ddepth.alloc(sizeof(int32_t) * Kpm));
  const size_t npad_max = (size_t)Tc_max * 64;
  HIPCHK(dtile.alloc(sizeof(phm::SmTile) * (size_t)Tc_max)); HIPCHK(dnst.alloc((size_t)NT * npad_max));
  HIPCHK(ddw.alloc(sizeof(unsigned long long) * n * npad_max)); HIPCHK(dcnt.alloc(sizeof(uint32_t) * (size_t)n * (n - 1) * npad_max));
  HIPCHK(dout.alloc(sizeof(double) * cols * npad_max));
  if (sm.nodes) HIPCHK(dnodes.alloc(sizeof(int32_t) * (size_t)NT * npad_max));
  std::vector<double> outh((size_t)cols * npad_max);
  std::vector<int32_t> depth_h(Kpm), nodes_h(sm.nodes ? (size_t)NT * npad_max : 0);
  std::vector<phm::SmTile> tiles;
  tiles.reserve((size_t)Tc_max);

  phm::SmParams sp = {};
  phm::LlParams& p = sp.ll;
  sp.n_node = in.Nn; sp.n_edge = E; sp.root_row = T + in.sched.root;
  sp.seed_lo = (uint32_t)(sm.opt.seed & 0xFFFFFFFFull); sp.seed_hi = (uint32_t)(sm.opt.seed >> 32);
  sp.replica = (uint32_t)sm.opt.replica_offset;
  sp.fx_scale = std::ldexp(1.0, 61 - sm.fx_exp); sp.fx_inv = std::ldexp(1.0, sm.fx_exp - 61);
  sp.tiles = dtile.as<phm::SmTile>(); sp.down = ddown.as<phm::DownStep>(); sp.order = dorder.as<int32_t>();
  sp.mu = dmu.as<double>(); sp.B = dB.as<double>(); sp.beta = dbeta.as<double>(); sp.depth_of = ddepth.as<int32_t>();
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
    const int branch_blocks = (int)std::min<int64_t>(((int64_t)E * nt + 3) / 4, 2048);
    HIPCHK(tm.start());
    HIPCHK(phm::launch_sm_sample(sp, sm.level_off, branch_blocks, maps_mode, nullptr));
    HIPCHK(tm.stop());
    HIPCHK(hipMemcpy(outh.data(), dout.p, sizeof(double) * cols * npad, hipMemcpyDeviceToHost));
    if (sm.nodes) HIPCHK(hipMemcpy(nodes_h.data(), dnodes.p, sizeof(int32_t) * (size_t)NT * npad, hipMemcpyDeviceToHost));
    uint32_t derrh = 0;
    HIPCHK(hipMemcpy(&derrh, derr.p, sizeof derrh, hipMemcpyDeviceToHost));
    HIPCHK(tm.elapsed(ms));
    kernel_ms += ms;
    if (derrh & phm::DERR_CAPACITY) return fail(PHM_ERR_CAPACITY, SM_FN + "a branch's jump-count series outgrew the table of its model");
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

  for (int64_t c0 = 0; c0 < count; c0 += pl.Kc_max) {
    const int64_t Kc = std::min<int64_t>(pl.Kc_max, count - c0);
    st = ln.load_models(first + c0, Kc);
    if (st) return st;
    const int Kp = ln.Kp;
    const int64_t m0 = ln.m0;                            // global index of this chunk's first model
    std::fill(depth_h.begin(), depth_h.end(), 0);
    int depth_c = 0;
    for (int64_t k = 0; k < Kc; ++k) {
      depth_h[k] = sm.depth[m0 + k];
      depth_c = std::max(depth_c, depth_h[k]);
    }
    HIPCHK(hipMemcpy(ddepth.p, depth_h.data(), sizeof(int32_t) * Kp, hipMemcpyHostToDevice));
    p = ln.params();
    sp.depth = depth_c;
    HIPCHK(tm.start());
    st = ln.expm(p);
    if (st) return st;
    HIPCHK(phm::launch_sm_table(sp, nullptr));
    HIPCHK(tm.stop());
    HIPCHK(tm.elapsed(ms));
    kernel_ms += ms;

    for (int64_t s0 = 0; s0 < S_eval; s0 += pl.Sc_max) {
      const int64_t Sc = std::min<int64_t>(pl.Sc_max, S_eval - s0);
      p.n_sites = (int)Sc;
      st = ln.stage_tips(s0, Sc);
      if (st) return st;
      HIPCHK(tm.start());
      st = ln.passes(p);
      if (st) return st;
      HIPCHK(tm.stop());
      st = ln.fetch_ll(Sc);
      if (st) return st;
      HIPCHK(tm.elapsed(ms));
      kernel_ms += ms;
      for (int64_t s = 0; s < Sc; ++s)
        for (int64_t k = 0; k < Kc; ++k) {
          const int64_t site = in.paired ? in.site_of_model[m0 + k] : s0 + s;
          const int64_t ev = ll_eval_of(in, s0 + s, m0 + k);
          const double ll = ln.llh[(size_t)s * Kp + k];
          loglik[ev] = ll;
          if (!std::isfinite(ll)) {                      // an impossible evaluation is not drawn: NaN rows, zero nodes, empty map rows
            for (int64_t h = ev * D; h < (ev + 1) * D; ++h) {
              for (int c = 0; c < cols; ++c) stats[h + H * c] = nan;
              if (sm.nodes) std::fill_n(sm.nodes + h * NT, NT, 0);
            }
            continue;
          }
          for (int d0 = 0; d0 < D; d0 += 64) {
            phm::SmTile tl = {};
            tl.ev = (int32_t)(s * Kp + k); tl.k = (int32_t)k; tl.eval_id = (uint32_t)(site * in.K + (m0 + k));
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
    kernel_ms += ms;
    st = ms_buf.copy_home(*mh, si, "phm_sample_histories_models");
    if (st) return st;
  }
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Models are independent and every draw is addressed by its global evaluation and draw index: with phm_options.n_devices > 1
// device d samples a contiguous range of the models (phm_plan_shards, run_shards), and every output is the one-device output bit
// for bit.
int32_t phm_sample_histories_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                    int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, int32_t draws,
                                    const phm_options* opt, double* stats, double* loglik, int32_t* nodes,
                                    int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state) {
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid || !stats || !loglik)
    return fail(PHM_ERR_BAD_INPUT, SM_FN + "NULL argument (only observe, site_of_model, opt, nodes and the map arrays may be NULL)");
  SmInput sm;
  int32_t st = ll_validate(SM_FN, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, o, sm.ll);
  if (st) return st;
  sm.opt = o; sm.nodes = nodes;
  st = sm_prepare(SM_FN, 2, phm::LL_LANE_MAX, "more than 8 states are not supported", sm, draws);
  if (st) return st;
  const bool want_maps = map_off || map_dwell || map_state;
  phm_maps::Host mh;
  if (want_maps) {
    st = phm_maps::validate("phm_sample_histories_models", sm.H, x->n_edge, map_off, map_cap, map_dwell, map_state, mh);
    if (st) return st;
  }
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, sm.ll.K, shards);
  if (st) return st;
  mh.shard_total.assign(shards.size(), 0);
  st = run_shards(shards, [&](const phm_shard& sh, size_t i) {
    return sm_device(sm, sh.device, sh.first, sh.count, stats, loglik, want_maps ? &mh : nullptr, i);
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
