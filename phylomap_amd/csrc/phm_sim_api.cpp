// phm_sim_api.cpp -- C-ABI of the forward simulation of character histories (phm_simulate_histories): sample2statehistory /
// samplethebranch (R/sourceme.R:346-414), simulate_2_state_tree / simulate_4_state_tree (R/simulate_*_state_tree.R) for many
// replicas in one call.  Validation on the host, one kernel launch per device, a transposing epilogue for the state matrices.
#include "phm_internal.h"
#include "phm_maps_host.h"
#include "phm_sim.h"

namespace {

// What every device of a call shares, checked and derived once on the host.
struct SimInput {
  int n = 0, T = 0, Nn = 0, E = 0;
  phm::Schedule sched;
  std::vector<double> qoff, inv_rate, pid, edge_length;
  std::vector<int32_t> tip_map, node_map;      // 0-based state -> reported 1-based state
};

int32_t sim_validate(const phm_tree* x, int32_t n, const double* Q, const double* pid, const int32_t* observe, const phm_options& o,
                     const int32_t* tips, const double* stats, SimInput& in) {
  if (!x || !Q || !pid || !tips || !stats) return fail(PHM_ERR_BAD_INPUT, "phm_simulate_histories: NULL argument (only `nodes` may be NULL)");
  if (n < 2 || n > phm::SIM_MAX_STATES) return fail(PHM_ERR_BAD_INPUT, "phm_simulate_histories: n_states must be in 2..64");
  if (o.reduce != 0) return fail(PHM_ERR_BAD_INPUT, "phm_simulate_histories: reduce must be 0 (statistics are per replica)");
  if (o.n_replicas < 0 || o.n_replicas > (1 << 22)) return fail(PHM_ERR_BAD_INPUT, "phm_simulate_histories: n_replicas must be in 0..4194304");
  if (!x->edge || !x->edge_length) return fail(PHM_ERR_BAD_INPUT, "phm_simulate_histories: x$edge and x$edge.length are required");
  std::string serr;
  if (!phm::build_schedule(x->n_tips, x->n_node, x->n_edge, x->edge, in.sched, serr)) return fail(PHM_ERR_BAD_INPUT, "tree: " + serr);
  in.n = n; in.T = x->n_tips; in.Nn = x->n_node; in.E = x->n_edge;
  int32_t st = check_edge_lengths(x);
  if (st) return st;
  in.edge_length.assign(x->edge_length, x->edge_length + in.E);
  st = check_generator(Q, n, in.qoff);
  if (st) return st;
  in.inv_rate.assign(n, 0.0);
  for (int i = 0; i < n; ++i) {
    double* row = &in.qoff[(size_t)i * n];
    const double qii = row[i];
    row[i] = 0.0;
    double off = 0.0;
    for (int j = 0; j < n; ++j) off += row[j];
    if (qii < 0.0 && !(off > 0.0)) return fail(PHM_ERR_BAD_INPUT, "Q: row " + std::to_string(i + 1) + " leaves its state but has no target");
    in.inv_rate[i] = qii < 0.0 ? 1.0 / (-qii) : 0.0;                  // 0: absorbing (q_ss = 0)
  }
  double psum = 0.0;
  st = check_root_prior(pid, n, psum);
  if (st) return st;
  in.pid.assign(pid, pid + n);
  st = check_observe(observe, n, in.tip_map);
  if (st) return st;
  in.node_map.resize(n);
  for (int i = 0; i < n; ++i) in.node_map[i] = i + 1;
  return PHM_OK;
}

// Replicas [first, first + R) of the call on one device.  tips / nodes / stats point at the caller's full matrices; stats has
// ld_stats rows (the call's replica count).  mh: the maps of phm_simulate_histories_maps (NULL: none), shard index `si`.
int32_t sim_one_device(const SimInput& in, const phm_options& o, int32_t device, int64_t first, int32_t R, int32_t* tips, int32_t* nodes,
                       double* stats, int64_t ld_stats, phm_maps::Host* mh = nullptr, size_t si = 0) {
  int32_t st = select_device(device);
  if (st) return st;
  const int n = in.n, T = in.T, E = in.E, rows = in.T + in.Nn, cols = n + n * n + 1;
  const int pad = (R + 63) / 64 * 64;
  std::vector<int32_t> maps(in.tip_map);
  maps.insert(maps.end(), in.node_map.begin(), in.node_map.end());
  const uint32_t err_init[2] = {0u, 0xFFFFFFFFu};
  DevBuf ddown, dq, dinv, dpid, dlen, dns, dstats, derr, dmap, dout;
  HIPCHK(upload(ddown, in.sched.down)); HIPCHK(upload(dq, in.qoff)); HIPCHK(upload(dinv, in.inv_rate)); HIPCHK(upload(dpid, in.pid));
  HIPCHK(upload(dlen, in.edge_length)); HIPCHK(upload(derr, err_init, 2)); HIPCHK(upload(dmap, maps));
  HIPCHK(dns.alloc((size_t)rows * pad)); HIPCHK(dstats.alloc(sizeof(double) * cols * (size_t)pad));
  HIPCHK(dout.alloc(sizeof(int32_t) * (size_t)R * (nodes ? rows : T)));
  HIPCHK(hipMemset(dstats.p, 0, dstats.bytes));
  phm::SimParams p;
  p.n_states = n; p.n_tips = T; p.n_node = in.Nn; p.n_edge = E; p.root = in.sched.root;
  p.n_rep = R; p.n_rep_pad = pad; p.replica_offset = (uint32_t)((int64_t)o.replica_offset + first);
  p.seed_lo = (uint32_t)(o.seed & 0xFFFFFFFFull); p.seed_hi = (uint32_t)(o.seed >> 32);
  p.down = ddown.as<phm::DownStep>(); p.qoff = dq.as<double>(); p.inv_rate = dinv.as<double>(); p.pid = dpid.as<double>();
  p.edge_length = dlen.as<double>(); p.nstate = dns.as<uint8_t>(); p.stats = dstats.as<double>(); p.err = derr.as<uint32_t>();
  const int maps_mode = mh ? mh->mode : phm::MAPS_OFF;
  phm_maps::Shard msh;
  if (mh) {
    st = msh.setup(*mh, first, R, pad, p.maps);
    if (st) return st;
  }
  KernelTimer tm;
  HIPCHK(tm.start());
  HIPCHK(phm::launch_simulate(p, nullptr, maps_mode));
  if (mh) HIPCHK(msh.after_kernel(*mh, pad, nullptr));      // sizing: counts -> offsets
  HIPCHK(tm.stop());
  HIPCHK(tm.elapsed(g_phm_last_kernel_ms));
  uint32_t errh[2];
  HIPCHK(hipMemcpy(errh, derr.p, sizeof errh, hipMemcpyDeviceToHost));
  if (errh[0] & phm::DERR_CAPACITY)
    return fail(PHM_ERR_CAPACITY, "more than " + std::to_string(phm::SIM_MAX_JUMPS) + " jumps on edge row " + std::to_string(errh[1] + 1) +
                                      " (samplethebranch stops there, R/sourceme.R:356)");
  st = device_status(errh[0]);
  if (st) return st;
  if (mh) {
    st = msh.copy_home(*mh, si, "phm_simulate_histories_maps");
    if (st) return st;
  }
  // statistics: [col][pad] -> the caller's column-major ld_stats x cols matrix, rows first .. first + R - 1
  HIPCHK(hipMemcpy2D(stats + first, sizeof(double) * ld_stats, dstats.p, sizeof(double) * pad, sizeof(double) * R, cols,
                     hipMemcpyDeviceToHost));
  HIPCHK(phm::launch_sim_transpose(dns.as<uint8_t>(), T, R, pad, dmap.as<int32_t>(), dout.as<int32_t>(), nullptr));
  HIPCHK(hipMemcpy(tips + first * T, dout.p, sizeof(int32_t) * (size_t)R * T, hipMemcpyDeviceToHost));
  if (nodes) {
    HIPCHK(phm::launch_sim_transpose(dns.as<uint8_t>(), rows, R, pad, dmap.as<int32_t>() + n, dout.as<int32_t>(), nullptr));
    HIPCHK(hipMemcpy(nodes + first * rows, dout.p, sizeof(int32_t) * (size_t)R * rows, hipMemcpyDeviceToHost));
  }
  return PHM_OK;
}

}  // namespace

extern "C" {

// Replicas are independent given (seed, global replica id): with phm_options.n_devices > 1 device d simulates a contiguous range
// of them (phm_plan_shards, run_shards); every output row is the one-device row bit for bit.
int32_t phm_simulate_histories(const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const int32_t* observe,
                               const phm_options* opt, int32_t* tips, int32_t* nodes, double* stats) {
  const phm_options o = resolve_options(opt);
  SimInput in;
  int32_t st = sim_validate(x, n_states, Q, pid, observe, o, tips, stats, in);
  if (st) return st;
  const int32_t R = std::max(1, (int)o.n_replicas);
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, R, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) {
    return sim_one_device(in, o, sh.device, sh.first, (int32_t)sh.count, tips, nodes, stats, R);
  });
}

// The same call, plus the stochastic maps of the histories: a sizing call (map_dwell and map_state NULL)
// writes map_off, a filling call reads it and writes the segments.  Every check runs before any device call.
int32_t phm_simulate_histories_maps(const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const int32_t* observe,
                                    const phm_options* opt, int32_t* tips, int32_t* nodes, double* stats,
                                    int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state) {
  const phm_options o = resolve_options(opt);
  SimInput in;
  int32_t st = sim_validate(x, n_states, Q, pid, observe, o, tips, stats, in);
  if (st) return st;
  const int32_t R = std::max(1, (int)o.n_replicas);
  phm_maps::Host mh;
  st = phm_maps::validate("phm_simulate_histories_maps", R, in.E, map_off, map_cap, map_dwell, map_state, mh);
  if (st) return st;
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, R, shards);
  if (st) return st;
  mh.shard_total.assign(shards.size(), 0);
  st = run_shards(shards, [&](const phm_shard& sh, size_t i) {
    return sim_one_device(in, o, sh.device, sh.first, (int32_t)sh.count, tips, nodes, stats, R, &mh, i);
  });
  if (st) return st;
  phm_maps::finish_sizing(mh, shards);
  return PHM_OK;
}

}  // extern "C"
