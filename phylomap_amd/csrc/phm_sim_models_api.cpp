// phm_sim_models_api.cpp -- C-ABI of the forward simulation under many rate matrices (phm_simulate_histories_models, DESIGN.md
// section 22): K models (Q_k, pid_k), R histories each, history h = k R + r being what phm_simulate_histories returns for global
// replica replica_offset + h under (Q_k, pid_k).  Validation and the model tables on the host by the front end it shares with
// phm_sim_api.cpp (phm_sim_host.h: check_generator's row-major Q, IEEE 1 / (-q_ii), totals summed left to right); per device and per chunk of histories the model
// tables of the chunk (model-fastest), then the root, depth-level and finish launches of phm_simm.hip and phm_sim.hip's
// transposing epilogue.  A shard of models is a contiguous range of histories, so section 14's per-shard map buffers
// (phm_maps_host.h) serve unchanged.
#include "phm_internal.h"
#include "phm_maps_host.h"
#include "phm_sim_host.h"
#include "phm_simm.h"

namespace {

const std::string SMM_FN = "phm_simulate_histories_models: ";

// What every device of a call shares, checked and derived once on the host.
struct SimmInput {
  int n = 0, T = 0, Nn = 0, E = 0, n_pid = 1, fx_exp = 0;
  int64_t K = 0, R = 0, H = 0;
  phm::Schedule sched;
  std::vector<int32_t> order, level_off;        // s.down positions by the depth of the parent
  std::vector<double> qoff, qtot, inv_rate;     // [K][n n] jump weights (diagonal 0), [K][n] their row totals, [K][n] 1 / (-q_ss)
  std::vector<double> pid, ptot;                // [n_pid][n] as given, [n_pid] summed left to right
  std::vector<double> edge_length;
  std::vector<int32_t> state_map;               // 0-based state -> reported 1-based state: n for the tips, then n for the nodes
  phm_options opt;
};

int32_t simm_validate(const phm_tree* x, int32_t n, int32_t K, const double* Q, const double* pid, int32_t n_pid,
                      const int32_t* observe, int32_t replicates, const phm_options& o, const int32_t* tips, const double* stats,
                      SimmInput& in) {
  int32_t st = phm_sim::check_head(SMM_FN, "only observe, opt, nodes and the map arrays may be NULL", x, n, Q, pid, tips, stats);
  if (st) return st;
  if (K < 1) return fail(PHM_ERR_BAD_INPUT, SMM_FN + "n_models must be >= 1");
  if (n_pid != 1 && n_pid != K) return fail(PHM_ERR_BAD_INPUT, SMM_FN + "n_pid must be 1 (shared) or n_models");
  if (replicates < 1) return fail(PHM_ERR_BAD_INPUT, SMM_FN + "replicates must be >= 1");
  if (o.reduce != 0) return fail(PHM_ERR_BAD_INPUT, SMM_FN + "reduce must be 0 (statistics are per history)");
  in.K = K; in.R = replicates; in.H = (int64_t)K * replicates;
  if (o.replica_offset < 0 || (int64_t)o.replica_offset + in.H > ((int64_t)1 << 32))
    return fail(PHM_ERR_BAD_INPUT, SMM_FN + "replica_offset + n_models * replicates = " + std::to_string((int64_t)o.replica_offset + in.H) +
                                       " does not fit in the 32-bit replica word");
  st = phm_sim::check_tree(SMM_FN, x, in.sched, in.edge_length);
  if (st) return st;
  in.n = n; in.T = x->n_tips; in.Nn = x->n_node; in.E = x->n_edge; in.n_pid = n_pid; in.opt = o;
  double tree_len = 0.0;
  for (int b = 0; b < in.E; ++b) tree_len += in.edge_length[b];
  (void)std::frexp(std::max(tree_len, 1.0), &in.fx_exp);
  const size_t nn = (size_t)n * n;
  in.qoff.resize((size_t)K * nn); in.qtot.resize((size_t)K * n); in.inv_rate.resize((size_t)K * n);
  for (int k = 0; k < K; ++k) {
    st = phm_sim::model_tables(Q + (size_t)k * nn, n, "model " + std::to_string(k) + ": ", &in.qoff[(size_t)k * nn], &in.qtot[(size_t)k * n],
                               &in.inv_rate[(size_t)k * n]);
    if (st) return st;
  }
  st = phm_sim::root_priors(pid, n_pid, n, true, in.pid, in.ptot);
  if (st) return st;
  st = phm_sim::state_maps(observe, n, in.state_map);
  if (st) return st;
  phm::depth_levels(in.sched, in.order, in.level_off);
  return PHM_OK;
}

// Models [first, first + count) of the call on one device: histories [first R, (first + count) R).  tips / nodes / stats point at
// the caller's full matrices.  mh: the maps (NULL: none), shard index `si`.
int32_t simm_device(const SimmInput& in, int32_t device, int64_t first, int64_t count, int32_t* tips, int32_t* nodes, double* stats,
                    phm_maps::Host* mh, size_t si) {
  int32_t st = select_device(device);
  if (st) return st;
  const int n = in.n, T = in.T, E = in.E, rows = in.T + in.Nn, cols = n + n * n + 1;
  const size_t nn = (size_t)n * n;
  const int64_t R = in.R, H = in.H;
  const int64_t h_first = first * R, h_count = count * R;            // the shard's histories
  KernelTimer tm;
  double kernel_ms = 0.0;
  const uint32_t err_init = 0u;
  const unsigned long long cap_init = ~0ull;
  DevBuf ddown, dorder, dlen, dmap, derr, dcap;
  HIPCHK(upload(ddown, in.sched.down)); HIPCHK(upload(dorder, in.order)); HIPCHK(upload(dlen, in.edge_length));
  HIPCHK(upload(dmap, in.state_map)); HIPCHK(upload(derr, &err_init, 1)); HIPCHK(upload(dcap, &cap_init, 1));

  phm::MapsDev maps_dev;
  phm_maps::Shard msh;
  const int64_t map_pad = (h_count + 63) / 64 * 64;
  if (mh) {
    if (h_count > (int64_t)INT32_MAX) return fail(PHM_ERR_UNSUPPORTED, SMM_FN + "maps of more than 2^31 - 1 histories on one device");
    st = msh.setup(*mh, h_first, h_count, map_pad, maps_dev);
    if (st) return st;
  }

  // Chunks of histories by free HBM: per history the state bytes, the accumulators, the columns and the transposed states; per
  // model (one per history at R = 1) its tables.
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const size_t table_b = sizeof(double) * (nn + 3 * (size_t)n + 1);
  const size_t per_hist = (size_t)rows + sizeof(unsigned long long) * n + sizeof(uint32_t) * nn + sizeof(double) * cols +
                          sizeof(int32_t) * (size_t)(nodes ? rows : T) + table_b / (size_t)R + 1;
  const size_t fixed = 130 * table_b;
  const int chunk = g_phm_debug.expect_chunk;
  int64_t Hc_max = (int64_t)((free_b / 2 > fixed ? free_b / 2 - fixed : 0) / per_hist) / 64 * 64;
  Hc_max = std::max<int64_t>(64, std::min<int64_t>({Hc_max, (h_count + 63) / 64 * 64, (int64_t)1 << 22}));
  if (chunk > 0) Hc_max = std::min<int64_t>(Hc_max, ((int64_t)chunk + 63) / 64 * 64);
  const size_t Kp_max = (size_t)((std::min<int64_t>(count, Hc_max / R + 2) + 63) / 64 * 64);
  const size_t pad_max = (size_t)Hc_max;

  DevBuf dq, dtot, dinv, dpid, dptot, dns, ddw, dcnt, dout, dtr;
  HIPCHK(dq.alloc(sizeof(double) * nn * Kp_max)); HIPCHK(dtot.alloc(sizeof(double) * n * Kp_max));
  HIPCHK(dinv.alloc(sizeof(double) * n * Kp_max)); HIPCHK(dpid.alloc(sizeof(double) * n * Kp_max));
  HIPCHK(dptot.alloc(sizeof(double) * Kp_max));
  HIPCHK(dns.alloc((size_t)rows * pad_max)); HIPCHK(ddw.alloc(sizeof(unsigned long long) * n * pad_max));
  HIPCHK(dcnt.alloc(sizeof(uint32_t) * nn * pad_max)); HIPCHK(dout.alloc(sizeof(double) * cols * pad_max));
  HIPCHK(dtr.alloc(sizeof(int32_t) * pad_max * (size_t)(nodes ? rows : T)));
  std::vector<double> qh(nn * Kp_max), toth((size_t)n * Kp_max), invh((size_t)n * Kp_max), pidh((size_t)n * Kp_max), ptoth(Kp_max);

  phm::SimmParams p = {};
  p.n_states = n; p.n_tips = T; p.n_node = in.Nn; p.n_edge = E; p.root = in.sched.root;
  p.n_rep_model = (uint32_t)R; p.replica_offset = (uint32_t)in.opt.replica_offset;
  p.seed_lo = (uint32_t)(in.opt.seed & 0xFFFFFFFFull); p.seed_hi = (uint32_t)(in.opt.seed >> 32);
  p.map_pad = map_pad;
  p.fx_scale = std::ldexp(1.0, 61 - in.fx_exp); p.fx_inv = std::ldexp(1.0, in.fx_exp - 61);
  p.down = ddown.as<phm::DownStep>(); p.order = dorder.as<int32_t>(); p.edge_length = dlen.as<double>();
  p.qoff = dq.as<double>(); p.qtot = dtot.as<double>(); p.inv_rate = dinv.as<double>(); p.pid = dpid.as<double>();
  p.ptot = dptot.as<double>(); p.nstate = dns.as<uint8_t>(); p.dwfx = ddw.as<unsigned long long>(); p.cnt = dcnt.as<uint32_t>();
  p.out = dout.as<double>(); p.err = derr.as<uint32_t>(); p.cap = dcap.as<unsigned long long>();
  p.maps = maps_dev;
  const int maps_mode = mh ? mh->mode : phm::MAPS_OFF;

  for (int64_t c0 = 0; c0 < h_count; c0 += Hc_max) {
    const int64_t Hc = std::min<int64_t>(Hc_max, h_count - c0);
    const size_t pad = (size_t)((Hc + 63) / 64 * 64);
    const int64_t h0 = h_first + c0;                                  // global index of the chunk's first history
    const int64_t k0 = h0 / R, Kc = (h0 + Hc - 1) / R - k0 + 1;       // the chunk's models
    const size_t Kp = (size_t)((Kc + 63) / 64 * 64);
    std::fill(qh.begin(), qh.end(), 0.0); std::fill(toth.begin(), toth.end(), 0.0); std::fill(invh.begin(), invh.end(), 0.0);
    std::fill(pidh.begin(), pidh.end(), 0.0); std::fill(ptoth.begin(), ptoth.end(), 0.0);
    for (int64_t k = 0; k < Kc; ++k) {                                // model-fastest: lane k of row e
      const size_t m = (size_t)(k0 + k), mp = in.n_pid == 1 ? 0 : m;
      for (size_t e = 0; e < nn; ++e) qh[e * Kp + k] = in.qoff[m * nn + e];
      for (int i = 0; i < n; ++i) {
        toth[(size_t)i * Kp + k] = in.qtot[m * n + i];
        invh[(size_t)i * Kp + k] = in.inv_rate[m * n + i];
        pidh[(size_t)i * Kp + k] = in.pid[mp * n + i];
      }
      ptoth[k] = in.ptot[mp];
    }
    HIPCHK(hipMemcpy(dq.p, qh.data(), sizeof(double) * nn * Kp, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dtot.p, toth.data(), sizeof(double) * n * Kp, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dinv.p, invh.data(), sizeof(double) * n * Kp, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dpid.p, pidh.data(), sizeof(double) * n * Kp, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dptot.p, ptoth.data(), sizeof(double) * Kp, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(ddw.p, 0, sizeof(unsigned long long) * n * pad));
    HIPCHK(hipMemset(dcnt.p, 0, sizeof(uint32_t) * nn * pad));
    p.n_hist = (int32_t)Hc; p.n_hist_pad = (int32_t)pad; p.h0 = (uint32_t)h0; p.k0 = (uint32_t)k0; p.Kp = (int32_t)Kp;
    p.map_row0 = c0;
    HIPCHK(tm.start());
    HIPCHK(phm::launch_simulate_models(p, in.level_off, chunk, maps_mode, nullptr));
    HIPCHK(tm.stop());
    uint32_t errh = 0;
    HIPCHK(hipMemcpy(&errh, derr.p, sizeof errh, hipMemcpyDeviceToHost));
    HIPCHK(tm.add_to(kernel_ms));
    if (errh & phm::DERR_CAPACITY) {
      unsigned long long caph = 0;
      HIPCHK(hipMemcpy(&caph, dcap.p, sizeof caph, hipMemcpyDeviceToHost));
      return phm_sim::capacity_refusal("model " + std::to_string(caph >> 32) + ": ", caph & 0xFFFFFFFFull);
    }
    st = device_status(errh);
    if (st) return st;
    st = phm_sim::send_home(dout.as<double>(), dns.as<uint8_t>(), dmap.as<int32_t>(), dtr.as<int32_t>(), n, T, rows, (int)pad, h0, Hc,
                            stats, H, tips, nodes);
    if (st) return st;
  }
  if (mh) {
    HIPCHK(tm.start());
    HIPCHK(msh.after_kernel(*mh, map_pad, nullptr));                 // sizing: counts -> offsets
    HIPCHK(tm.stop());
    HIPCHK(tm.add_to(kernel_ms));
    st = msh.copy_home(*mh, si, "phm_simulate_histories_models");
    if (st) return st;
  }
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Models are independent and every draw is addressed by the global history index: with phm_options.n_devices > 1 device d
// simulates a contiguous range of the models (phm_plan_shards, run_shards), and every output is the one-device output bit for bit.
int32_t phm_simulate_histories_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                      int32_t n_pid, const int32_t* observe, int32_t replicates, const phm_options* opt,
                                      int32_t* tips, int32_t* nodes, double* stats,
                                      int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state) {
  const phm_options o = resolve_options(opt);
  SimmInput in;
  int32_t st = simm_validate(x, n_states, n_models, Q, pid, n_pid, observe, replicates, o, tips, stats, in);
  if (st) return st;
  const bool want_maps = map_off || map_dwell || map_state;
  phm_maps::Host mh;
  if (want_maps) {
    st = phm_maps::validate("phm_simulate_histories_models", in.H, in.E, map_off, map_cap, map_dwell, map_state, mh);
    if (st) return st;
  }
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, in.K, shards);
  if (st) return st;
  mh.shard_total.assign(shards.size(), 0);
  st = run_shards(shards, [&](const phm_shard& sh, size_t i) {
    return simm_device(in, sh.device, sh.first, sh.count, tips, nodes, stats, want_maps ? &mh : nullptr, i);
  });
  if (st) return st;
  if (want_maps) {
    // finish_sizing works in units of histories: a shard of models is histories [first R, (first + count) R)
    std::vector<phm_shard> hs = shards;
    for (phm_shard& s : hs) { s.first *= in.R; s.count *= in.R; }
    phm_maps::finish_sizing(mh, hs);
  }
  return PHM_OK;
}

}  // extern "C"
