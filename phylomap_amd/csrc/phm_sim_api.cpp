// phm_sim_api.cpp -- C-ABI of the forward simulation of character histories (phm_simulate_histories): sample2statehistory /
// samplethebranch (R/sourceme.R:346-414), simulate_2_state_tree / simulate_4_state_tree (R/simulate_*_state_tree.R) for many
// replicas in one call.  Validation on the host (phm_sim_host.h, shared with phm_sim_models_api.cpp), one kernel launch per device,
// a transposing epilogue for the state matrices.
#include "phm_internal.h"
#include "phm_maps_host.h"
#include "phm_sim_host.h"

namespace {

const std::string SIM_FN = "phm_simulate_histories: ";

// What every device of a call shares, checked and derived once on the host.
struct SimInput {
  int n = 0, T = 0, Nn = 0, E = 0;
  phm::Schedule sched;
  std::vector<double> qoff, inv_rate, pid, edge_length;
  std::vector<int32_t> state_map;              // 0-based state -> reported 1-based state: n for the tips, then n for the nodes
};

int32_t sim_validate(const phm_tree* x, int32_t n, const double* Q, const double* pid, const int32_t* observe, const phm_options& o,
                     const int32_t* tips, const double* stats, SimInput& in) {
  int32_t st = phm_sim::check_head(SIM_FN, "only `nodes` may be NULL", x, n, Q, pid, tips, stats);
  if (st) return st;
  if (o.reduce != 0) return fail(PHM_ERR_BAD_INPUT, SIM_FN + "reduce must be 0 (statistics are per replica)");
  if (o.n_replicas < 0 || o.n_replicas > (1 << 22)) return fail(PHM_ERR_BAD_INPUT, SIM_FN + "n_replicas must be in 0..4194304");
  st = phm_sim::check_tree(SIM_FN, x, in.sched, in.edge_length);
  if (st) return st;
  in.n = n; in.T = x->n_tips; in.Nn = x->n_node; in.E = x->n_edge;
  in.qoff.resize((size_t)n * n); in.inv_rate.resize(n);
  std::vector<double> qtot(n), ptot;               // the kernel sums both totals itself, in the same order
  st = phm_sim::model_tables(Q, n, "", in.qoff.data(), qtot.data(), in.inv_rate.data());
  if (st) return st;
  st = phm_sim::root_priors(pid, 1, n, false, in.pid, ptot);
  if (st) return st;
  return phm_sim::state_maps(observe, n, in.state_map);
}

// Replicas [first, first + R) of the call on one device.  tips / nodes / stats point at the caller's full matrices; stats has
// ld_stats rows (the call's replica count).  mh: the maps of phm_simulate_histories_maps (NULL: none), shard index `si`.
int32_t sim_one_device(const SimInput& in, const phm_options& o, int32_t device, int64_t first, int32_t R, int32_t* tips, int32_t* nodes,
                       double* stats, int64_t ld_stats, phm_maps::Host* mh, size_t si) {
  int32_t st = select_device(device);
  if (st) return st;
  const int n = in.n, T = in.T, E = in.E, rows = in.T + in.Nn, cols = n + n * n + 1;
  const int pad = (R + 63) / 64 * 64;
  const uint32_t err_init[2] = {0u, 0xFFFFFFFFu};
  DevBuf ddown, dq, dinv, dpid, dlen, dns, dstats, derr, dmap, dout;
  HIPCHK(upload(ddown, in.sched.down)); HIPCHK(upload(dq, in.qoff)); HIPCHK(upload(dinv, in.inv_rate)); HIPCHK(upload(dpid, in.pid));
  HIPCHK(upload(dlen, in.edge_length)); HIPCHK(upload(derr, err_init, 2)); HIPCHK(upload(dmap, in.state_map));
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
  if (errh[0] & phm::DERR_CAPACITY) return phm_sim::capacity_refusal("", errh[1]);
  st = device_status(errh[0]);
  if (st) return st;
  if (mh) {
    st = msh.copy_home(*mh, si, "phm_simulate_histories_maps");
    if (st) return st;
  }
  return phm_sim::send_home(dstats.as<double>(), dns.as<uint8_t>(), dmap.as<int32_t>(), dout.as<int32_t>(), n, T, rows, pad, first, R,
                            stats, ld_stats, tips, nodes);
}

// Both entry points.  Replicas are independent given (seed, global replica id): with several devices each simulates a contiguous
// range of them (run_shards) and every output row is the one-device row bit for bit.  Maps: a sizing call
// (map_dwell and map_state NULL) writes map_off, a filling call reads it; every check runs before any device call.
int32_t simulate(const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const int32_t* observe, const phm_options* opt,
                 int32_t* tips, int32_t* nodes, double* stats, bool want_maps, int64_t* map_off, int64_t map_cap, double* map_dwell,
                 int32_t* map_state) {
  const phm_options o = resolve_options(opt);
  SimInput in;
  int32_t st = sim_validate(x, n_states, Q, pid, observe, o, tips, stats, in);
  if (st) return st;
  const int32_t R = std::max(1, (int)o.n_replicas);
  phm_maps::Host mh;
  if (want_maps) st = phm_maps::validate("phm_simulate_histories_maps", R, in.E, map_off, map_cap, map_dwell, map_state, mh);
  if (st) return st;
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, R, shards);
  if (st) return st;
  mh.shard_total.assign(shards.size(), 0);
  st = run_shards(shards, [&](const phm_shard& sh, size_t i) {
    return sim_one_device(in, o, sh.device, sh.first, (int32_t)sh.count, tips, nodes, stats, R, want_maps ? &mh : nullptr, i);
  });
  if (!st && want_maps) phm_maps::finish_sizing(mh, shards);
  return st;
}

}  // namespace

extern "C" {

int32_t phm_simulate_histories(const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const int32_t* observe,
                               const phm_options* opt, int32_t* tips, int32_t* nodes, double* stats) {
  return simulate(x, n_states, Q, pid, observe, opt, tips, nodes, stats, false, nullptr, 0, nullptr, nullptr);
}

int32_t phm_simulate_histories_maps(const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const int32_t* observe,
                                    const phm_options* opt, int32_t* tips, int32_t* nodes, double* stats,
                                    int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state) {
  return simulate(x, n_states, Q, pid, observe, opt, tips, nodes, stats, true, map_off, map_cap, map_dwell, map_state);
}

}  // extern "C"
