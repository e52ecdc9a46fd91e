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

// first j with u * total <= w_0 + .. + w_j, w_j at w[j st], `total` summed left to right beforehand
template <int NS>
__device__ __forceinline__ int simm_categorical(const double* __restrict__ w, size_t st, double total, int n_rt, double u,
                                                uint32_t& err) {
  const int n = NS > 0 ? NS : n_rt;
  if (!(total > 0.0) || isinf(total)) err |= DERR_ZERO_PROB;
  const double thr = u * total;
  double cum = w[0];
  int idx = (thr <= cum) ? 0 : 1;
#pragma unroll
  for (int j = 1; j < n - 1; ++j) { cum += w[(size_t)j * st]; idx += (thr <= cum) ? 0 : 1; }
  return idx;
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
    s = simm_categorical<0>(p.pid + l.k, (size_t)p.Kp, p.ptot[l.k], p.n_states,
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
  constexpr int NA = NS > 0 ? NS : 1, NC = NS > 0 ? NS * NS : 1;
  uint32_t err = 0;
  for (int64_t item = wslot; item < items; item += (int64_t)gridDim.x * (SIMM_BLOCK / 64)) {
    const int tile = (int)(item % n_tiles);
    const int q0 = begin + (int)(item / n_tiles) * group, q1 = min(q0 + group, end);
    const int i = tile * 64 + lane;
    const SimmLane l = simm_lane(p, i);
    if (!l.valid) continue;                                        // a lane past the last history of the chunk
    unsigned long long acc_dw[NA];
    uint32_t acc_ct[NC];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc_dw[c] = 0ull;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc_ct[c] = 0u;
    auto add_dwell = [&](int s, double x) {                        // fixed point: exact in any order
      const unsigned long long fx = (unsigned long long)__double2ll_rn(x * p.fx_scale);
      if constexpr (NS > 0) {
#pragma unroll
        for (int c = 0; c < NA; ++c) acc_dw[c] += (s == c) ? fx : 0ull;
      } else {
        atomicAdd(p.dwfx + (size_t)s * pad + i, fx);
      }
    };
    auto count = [&](int from, int to) {
      const int col = from * n + to;
      if constexpr (NS > 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) acc_ct[c] += (col == c) ? 1u : 0u;
      } else {
        atomicAdd(p.cnt + (size_t)col * pad + i, 1u);
      }
    };
    for (int qi = q0; qi < q1; ++qi) {
      const DownStep d = p.down[p.order[qi]];                      // wave-uniform
      const size_t parent_row = (size_t)(T + d.parent), child_row = (size_t)(d.child >= 0 ? T + d.child : ~d.child);
      const double t = p.edge_length[d.edge];
      int s = p.nstate[parent_row * pad + i];
      // maps: segments of this branch so far (count) / the write cursor and the end of the history's row of this edge (write)
      const int64_t mrow = (p.map_row0 + i) * p.n_edge + d.edge;
      int64_t cur = 0, stop = 0;
      if constexpr (MODE == MAPS_WRITE) { cur = p.maps.off[mrow] - p.maps.base; stop = p.maps.off[mrow + 1] - p.maps.base; }
      auto segment = [&](int st, double x) {
        add_dwell(st, x);
        if constexpr (MODE == MAPS_WRITE) {
          if (cur < stop) { p.maps.dwell[cur] = x; p.maps.state[cur] = st + 1; }
        }
        if constexpr (MODE != MAPS_OFF) ++cur;
      };
      Stream rs;
      rs.open(ENT_BSTATE | (uint32_t)d.edge, SIM_ITER, l.rep, p.seed_lo, p.seed_hi);
      double pos = 0.0;
      for (uint32_t j = 0;; ++j) {
        const double ir = p.inv_rate[(size_t)s * Kp + l.k];
        if (ir == 0.0) { segment(s, t - pos); break; }             // absorbing: the rest of the branch, no draw
        const double gap = ir * neglog_u32(rs.draw_word(2u * j), s_ltab);
        const double dab = pos + gap;
        if (!(dab < t)) { segment(s, gap - (dab - t)); break; }    // seg_len - (dab - branchlength)
        segment(s, gap);
        if (j == (uint32_t)SIM_MAX_JUMPS) {
          err |= DERR_CAPACITY;
          atomicMin(p.cap, ((unsigned long long)(p.k0 + (uint32_t)l.k) << 32) | (unsigned long long)(uint32_t)d.edge);
          break;
        }
        const int nx = simm_categorical<NS>(p.qoff + (size_t)(s * n) * Kp + l.k, Kp, p.qtot[(size_t)s * Kp + l.k], n,
                                            rs.draw(2u * j + 1u), err);
        count(s, nx);
        s = nx;
        pos = dab;
      }
      p.nstate[child_row * pad + i] = (uint8_t)s;
      if constexpr (MODE == MAPS_COUNT) p.maps.seg_cnt[(size_t)d.edge * p.map_pad + (size_t)(p.map_row0 + i)] = (uint16_t)cur;
      if constexpr (MODE == MAPS_WRITE) {
        if (cur != stop) atomicMin(p.maps.bad_row, (unsigned long long)mrow);
      }
    }
    if constexpr (NS > 0) {
#pragma unroll
      for (int c = 0; c < NA; ++c) if (acc_dw[c]) atomicAdd(p.dwfx + (size_t)c * pad + i, acc_dw[c]);
#pragma unroll
      for (int c = 0; c < NC; ++c) if (acc_ct[c]) atomicAdd(p.cnt + (size_t)c * pad + i, acc_ct[c]);
    }
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
  if (c < n) v = (double)(long long)p.dwfx[(size_t)c * pad + i] * p.fx_inv;
  else if (c < n + nn) v = (double)p.cnt[(size_t)(c - n) * pad + i];
  else v = (double)p.nstate[(size_t)(p.n_tips + p.root) * pad + i];
  p.out[gid] = v;
}

template <int MODE>
void launch_level(const SimmParams& p, int blocks, int begin, int end, int group, hipStream_t stream) {
#ifdef PHM_EXPERIMENT_SIMM_GENERIC        // measurement builds only: 2..4 states through the 5..64-state form
  hipLaunchKernelGGL((simm_level_kernel<0, MODE>), dim3(blocks), dim3(SIMM_BLOCK), 0, stream, p, begin, end, group);
  return;
#endif
  switch (p.n_states) {
    case 2: hipLaunchKernelGGL((simm_level_kernel<2, MODE>), dim3(blocks), dim3(SIMM_BLOCK), 0, stream, p, begin, end, group); break;
    case 3: hipLaunchKernelGGL((simm_level_kernel<3, MODE>), dim3(blocks), dim3(SIMM_BLOCK), 0, stream, p, begin, end, group); break;
    case 4: hipLaunchKernelGGL((simm_level_kernel<4, MODE>), dim3(blocks), dim3(SIMM_BLOCK), 0, stream, p, begin, end, group); break;
    default: hipLaunchKernelGGL((simm_level_kernel<0, MODE>), dim3(blocks), dim3(SIMM_BLOCK), 0, stream, p, begin, end, group); break;
  }
}

}  // namespace

hipError_t launch_simulate_models(const SimmParams& p, const std::vector<int32_t>& level_off, int max_group, int maps_mode,
                                  hipStream_t stream, int* launches) {
  if (p.n_states < 2 || p.n_states > SIM_MAX_STATES || p.n_hist <= 0 || p.n_hist_pad < p.n_hist || p.n_hist_pad % 64 || p.Kp <= 0 ||
      p.Kp % 64 || p.n_rep_model == 0)
    return hipErrorInvalidValue;
  constexpr int W = SIMM_BLOCK / 64;
  const int64_t n_tiles = p.n_hist_pad / 64;
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
    if (maps_mode == MAPS_COUNT) launch_level<MAPS_COUNT>(p, blocks, begin, end, group, stream);
    else if (maps_mode == MAPS_WRITE) launch_level<MAPS_WRITE>(p, blocks, begin, end, group, stream);
    else launch_level<MAPS_OFF>(p, blocks, begin, end, group, stream);
    ++n_launch;
  }
  const int64_t cells = (int64_t)(p.n_states + p.n_states * p.n_states + 1) * p.n_hist_pad;
  hipLaunchKernelGGL(simm_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, p);
  ++n_launch;
  if (launches) *launches = n_launch;
  return hipGetLastError();
}

}  // namespace phm
