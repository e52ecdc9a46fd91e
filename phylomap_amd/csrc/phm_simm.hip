// phm_simm.hip -- forward simulation of the chain along the tree under MANY rate matrices in one call:
// K models (Q_k, pid_k), R histories each; history h = k R + r is, draw for draw, what phm_sim.hip's sim_kernel computes for global
// replica replica_offset + h under (Q_k, pid_k) -- section 12's streams and arithmetic, with only the replica word carrying h.
//
// Mapping: one LANE owns one history, a tile is 64 consecutive histories, and the MODEL is per lane (k = h / R): a wave holds 64
// models at R = 1, one at R >= 64, and crosses a model boundary at any lane otherwise.  The model tables (jump weights, row
// totals, 1 / (-q_ss), root prior) are model-fastest [..][Kp], so lanes that agree on the current state load coalesced rows; no
// Q in LDS.  Branch-parallel over depth levels, not a walk: a root launch, then one launch per depth level in which a wave takes
// (tile, group of consecutive edges of the level), reads the parent's state byte, walks the branch on its own stream and writes
// the child's byte -- [node id - 1][history] bytes, launch_sim_transpose's layout.  Several waves work on one history at once, so
// dwell goes to 64-bit fixed point (exact in any order: the sums are the same bits under any chunking) and counts to uint32, by
// atomics: one per segment for 5..64 states, one per touched column and item for 2..4 states (register accumulators, selects).
// A finish launch converts them to the simulator's columns.  Every loop has a hard end: SIM_MAX_JUMPS per branch, the item count
// for the persistent waves.
#include "phm_simm.h"

#include <algorithm>

#include "phm_history.h"
#include "phm_sim_walk.h"

namespace phm {

namespace {

// what a lane works on: history i of the chunk
struct SimmLane {
  bool valid;
  int k;                 // model, as a lane of the tables
  uint32_t rep;          // Philox replica word
};
__device__ __forceinline__ SimmLane simm_lane(const SimmParams& p, int i) {
  SimmLane l;
  const uint32_t h = p.h0 + (uint32_t)i;
  l.valid = i < p.n_hist;
  l.k = l.valid ? (int)(h / p.n_rep_model - p.k0) : 0;
  l.rep = p.replica_offset + h;
  return l;
}

// root: draw 0 of the stream (root node id, iteration SIM_ITER), categorical over the lane's pid
__global__ __launch_bounds__(SIMM_BLOCK) void simm_root_kernel(SimmParams p) {
  const int i = blockIdx.x * SIMM_BLOCK + threadIdx.x;
  if (i >= p.n_hist_pad) return;
  const SimmLane l = simm_lane(p, i);
  const uint32_t root_id = (uint32_t)(p.n_tips + 1 + p.root);
  uint32_t err = 0;
  int s = 0;
  if (l.valid)
    s = sim_categorical<0>(p.pid + l.k, (size_t)p.Kp, p.ptot[l.k], p.n_states,
                           stream_u(p.seed_lo, p.seed_hi, l.rep, SIM_ITER, ENT_NODE | root_id, 0), err);
  p.nstate[(size_t)(root_id - 1) * p.n_hist_pad + i] = (uint8_t)s;
  if (err) atomicOr(p.err, err);
}

// one depth level, positions [begin, end) of p.order: persistent waves over (tile, group of `group` consecutive edges of the level).
// MODE (phm_maps.h) as in sim_kernel: the draws are the same in all three.
template <int NS, int MODE>
__global__ __launch_bounds__(SIMM_BLOCK) void simm_level_kernel(SimmParams p, int begin, int end, int group) {
  __shared__ __align__(16) double s_ltab[2 * PHM_LOGTAB_N];        // (1/c_j, log c_j) of the exponential variates (neglog_u32)
  for (int i = threadIdx.x; i < 2 * PHM_LOGTAB_N; i += SIMM_BLOCK) s_ltab[i] = logtab_entry(i);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wslot = blockIdx.x * (SIMM_BLOCK / 64) + (threadIdx.x >> 6);
  const int n = NS > 0 ? NS : p.n_states;
  const size_t Kp = (size_t)p.Kp, pad = (size_t)p.n_hist_pad;
  const int T = p.n_tips;
  const int n_tiles = p.n_hist_pad / 64;
  const int n_groups = (end - begin + group - 1) / group;
  const int64_t items = (int64_t)n_groups * n_tiles;
  uint32_t err = 0;
  for (int64_t item = wslot; item < items; item += (int64_t)gridDim.x * (SIMM_BLOCK / 64)) {
    const int tile = (int)(item % n_tiles);
    const int q0 = begin + (int)(item / n_tiles) * group, q1 = min(q0 + group, end);
    const int i = tile * 64 + lane;
    const SimmLane l = simm_lane(p, i);
    if (!l.valid) continue;                                        // a lane past the last history of the chunk
    StatLanes<NS, NS * NS> st;                                     // counts by from * n + to
    st.begin(p.dwfx, p.cnt, pad, (size_t)i, p.fx_scale);
    const SimModel model = {p.qoff, p.qtot, p.inv_rate, Kp, l.k, n};   // model-fastest tables, the lane's model
    for (int qi = q0; qi < q1; ++qi) {
      const DownStep d = p.down[p.order[qi]];                      // wave-uniform
      const size_t parent_row = (size_t)(T + d.parent), child_row = (size_t)(d.child >= 0 ? T + d.child : ~d.child);
      const double t = p.edge_length[d.edge];
      const int s0 = p.nstate[parent_row * pad + i];
      MapRow<MODE> mr;                                             // maps: the history's row of this edge
      mr.begin(p.maps, (p.map_row0 + i) * p.n_edge + d.edge);
      Stream rs;
      rs.open(ENT_BSTATE | (uint32_t)d.edge, SIM_ITER, l.rep, p.seed_lo, p.seed_hi);
      const int s = sim_walk_branch<NS>(
          s0, t, rs, s_ltab, model,
          [&](int state, double x) { st.dwell(state, x); mr.emit(x, state); },
          [&](int from, int to) { st.count(from * n + to); },
          [&]() { atomicMin(p.cap, ((unsigned long long)(p.k0 + (uint32_t)l.k) << 32) | (unsigned long long)(uint32_t)d.edge); }, err);
      p.nstate[child_row * pad + i] = (uint8_t)s;
      mr.end((size_t)d.edge * p.map_pad + (size_t)(p.map_row0 + i));
    }
    st.flush();
  }
  if (err) atomicOr(p.err, err);
}

// accumulators -> the simulator's columns: dwell (n), counts (n x n, row-major from,to), root state
__global__ __launch_bounds__(256) void simm_finish_kernel(SimmParams p) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = p.n_states, nn = n * n;
  const int64_t pad = p.n_hist_pad;
  if (gid >= (int64_t)(n + nn + 1) * pad) return;
  const int c = (int)(gid / pad);
  const int64_t i = gid % pad;
  double v;
  if (c < n + nn) v = stat_cell_value(p.dwfx, p.cnt, n, c, (size_t)pad, (size_t)i, p.fx_inv);
  else v = (double)p.nstate[(size_t)(p.n_tips + p.root) * pad + i];
  p.out[gid] = v;
}

}  // namespace

hipError_t launch_simulate_models(const SimmParams& p, const std::vector<int32_t>& level_off, int max_group, int maps_mode,
                                  hipStream_t stream, int* launches) {
  if (p.n_states < 2 || p.n_states > SIM_MAX_STATES || p.n_hist <= 0 || p.n_hist_pad < p.n_hist || p.n_hist_pad % 64 || p.Kp <= 0 ||
      p.Kp % 64 || p.n_rep_model == 0)
    return hipErrorInvalidValue;
  constexpr int W = SIMM_BLOCK / 64;
  const int64_t n_tiles = p.n_hist_pad / 64;
#ifdef PHM_EXPERIMENT_SIMM_GENERIC        // measurement builds only: 2..4 states through the 5..64-state form
  const int n_form = 0;
#else
  const int n_form = p.n_states;
#endif
  int n_launch = 0;
  hipLaunchKernelGGL(simm_root_kernel, dim3((p.n_hist_pad + SIMM_BLOCK - 1) / SIMM_BLOCK), dim3(SIMM_BLOCK), 0, stream, p);
  ++n_launch;
  for (size_t l = 0; l + 1 < level_off.size(); ++l) {
    const int begin = level_off[l], end = level_off[l + 1];
    const int64_t cnt = end - begin;
    if (cnt <= 0) continue;
    // edges per wave item: as many as still leave every SIMD a few waves
    int group = (int)std::max<int64_t>(1, std::min<int64_t>(16, cnt * n_tiles / 8192));
    if (max_group > 0) group = std::min(group, max_group);
    const int64_t items = (cnt + group - 1) / group * n_tiles;
    const int blocks = (int)std::min<int64_t>((items + W - 1) / W, 65536);
    with_producer_form(maps_mode, n_form, [&](auto mode, auto ns) {
      hipLaunchKernelGGL((simm_level_kernel<decltype(ns)::value, decltype(mode)::value>), dim3(blocks), dim3(SIMM_BLOCK), 0, stream, p,
                         begin, end, group);
    });
    ++n_launch;
  }
  const int64_t cells = (int64_t)(p.n_states + p.n_states * p.n_states + 1) * p.n_hist_pad;
  hipLaunchKernelGGL(simm_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, p);
  ++n_launch;
  if (launches) *launches = n_launch;
  return hipGetLastError();
}

}  // namespace phm
