// phm_sim.hip -- forward simulation of the chain along the tree: sample2statehistory / samplethebranch (R/sourceme.R:346-414)
// for many independent replicas at once.
//
// Mapping: one LANE owns one replica; the 64 lanes of a wavefront walk the same pre-order of the branches in lock step, so the
// branch records (edge row, parent, child, length) are wave-uniform scalar loads.  Along a branch every lane draws its own
// Gillespie path (lanes diverge only in the number of jumps).  Node states go to a [node][replica] byte buffer (one coalesced
// 64-byte row per wave); the replica-major tip / node matrices the caller wants come out of a transposing epilogue.
// Q's jump weights (diagonal 0), their row totals and 1/(-q_ss) are staged in LDS once per workgroup (32 KB at 64 states).
// Accumulators: n <= 4 in registers (selects, no dynamic register indexing); 5..64 states in the [col][replica] statistics
// buffer itself -- a replica belongs to one lane, so plain read-modify-write, no atomics.
#include "phm_sim_walk.h"

namespace phm {

namespace {

// MODE (phm_maps.h): MAPS_OFF = the plain simulation; MAPS_COUNT also stores every branch's segment count; MAPS_WRITE also
// stores every segment (dwell, 1-based true state) at the lane's cursor in its row of p.maps.  The draws are the same in all three.
template <int NS, int MODE>
__global__ __launch_bounds__(SIM_BLOCK) void sim_kernel(SimParams p) {
  constexpr int QN = NS > 0 ? NS : SIM_MAX_STATES;
  constexpr int AN = NS > 0 ? NS : 1;
  __shared__ __align__(16) double s_ltab[2 * PHM_LOGTAB_N];      // (1/c_j, log c_j) of the exponential variates (neglog_u32)
  __shared__ double s_q[QN * QN];
  __shared__ double s_inv[QN], s_tot[QN], s_pid[QN];
  const int n = NS > 0 ? NS : p.n_states;
  for (int i = threadIdx.x; i < 2 * PHM_LOGTAB_N; i += SIM_BLOCK) s_ltab[i] = logtab_entry(i);
  for (int i = threadIdx.x; i < n * n; i += SIM_BLOCK) s_q[i] = p.qoff[i];
  for (int i = threadIdx.x; i < n; i += SIM_BLOCK) { s_inv[i] = p.inv_rate[i]; s_pid[i] = p.pid[i]; }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += SIM_BLOCK) {              // row totals, left to right (what the categorical rule sums)
    double t = s_q[i * n];
    for (int j = 1; j < n; ++j) t += s_q[i * n + j];
    s_tot[i] = t;
  }
  __syncthreads();

  const int r = blockIdx.x * SIM_BLOCK + threadIdx.x;             // replica of this launch
  if (r >= p.n_rep) return;
  const uint32_t rep = p.replica_offset + (uint32_t)r;
  const size_t pad = (size_t)p.n_rep_pad;
  const int T = p.n_tips;
  double* __restrict__ col = p.stats + r;                          // column c of this replica: col[c * pad]
  uint32_t err = 0;
  double dw[AN];
  uint32_t cnt[AN][AN];
#pragma unroll
  for (int i = 0; i < AN; ++i) {
    dw[i] = 0.0;
#pragma unroll
    for (int j = 0; j < AN; ++j) cnt[i][j] = 0u;
  }
  const SimModel model = {s_q, s_tot, s_inv, 1, 0, n};              // the workgroup's LDS copy
  auto add_dwell = [&](int s, double x) {
    if constexpr (NS > 0) {
#pragma unroll
      for (int i = 0; i < NS; ++i) dw[i] += (s == i) ? x : 0.0;   // + 0.0 leaves a sum unchanged: the bits of dw[s] += x
    } else {
      col[(size_t)s * pad] += x;
    }
  };

  // root: draw 0 of the stream (root node id, iteration SIM_ITER), categorical over pid
  const uint32_t root_id = (uint32_t)(T + 1 + p.root);
  int root_state;
  {
    double total = s_pid[0];
    for (int j = 1; j < n; ++j) total += s_pid[j];
    root_state = sim_categorical<NS>(s_pid, 1, total, n, stream_u(p.seed_lo, p.seed_hi, rep, SIM_ITER, ENT_NODE | root_id, 0), err);
  }
  p.nstate[(size_t)(root_id - 1) * pad + r] = (uint8_t)root_state;

  for (int k = 0; k < p.n_edge; ++k) {
    const DownStep d = p.down[k];                                  // wave-uniform
    const size_t parent_row = (size_t)(T + d.parent), child_row = (size_t)(d.child >= 0 ? T + d.child : ~d.child);
    const double t = p.edge_length[d.edge];
    const int s0 = p.nstate[parent_row * pad + r];
    const size_t mrow = (size_t)r * p.n_edge + d.edge;            // maps: row r * E + edge
    MapRow<MODE> mr;
    mr.begin(p.maps, (int64_t)mrow);
    Stream rs;
    rs.open(ENT_BSTATE | (uint32_t)d.edge, SIM_ITER, rep, p.seed_lo, p.seed_hi);
    const int s = sim_walk_branch<NS>(
        s0, t, rs, s_ltab, model,
        [&](int st, double x) { add_dwell(st, x); mr.emit(x, st); },
        [&](int from, int to) {
          if constexpr (NS > 0) {
#pragma unroll
            for (int a = 0; a < NS; ++a)
#pragma unroll
              for (int b = 0; b < NS; ++b) cnt[a][b] += (from == a && to == b) ? 1u : 0u;
          } else {
            col[(size_t)(n + from * n + to) * pad] += 1.0;
          }
        },
        [&]() { atomicMin(&p.err[1], (uint32_t)d.edge); }, err);
    p.nstate[child_row * pad + r] = (uint8_t)s;
    mr.end((size_t)d.edge * pad + r);                              // one 128-byte row of counts per wave
  }

  if constexpr (NS > 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      col[(size_t)i * pad] = dw[i];
#pragma unroll
      for (int j = 0; j < NS; ++j) col[(size_t)(NS + i * NS + j) * pad] = (double)cnt[i][j];
    }
  }
  col[(size_t)(n + n * n) * pad] = (double)root_state;
  if (err) atomicOr(&p.err[0], err);
}

constexpr int TR_TILE = 64;

// [row][replica] bytes -> [replica][row] int32 through a 64 x 64 LDS tile, mapped through `map`
__global__ __launch_bounds__(256) void sim_transpose_kernel(const uint8_t* __restrict__ nstate, int rows, int n_rep, int pad,
                                                            const int32_t* __restrict__ map, int32_t* __restrict__ out) {
  __shared__ uint8_t tile[TR_TILE][TR_TILE + 4];
  const int row0 = blockIdx.x * TR_TILE, rep0 = blockIdx.y * TR_TILE;
  for (int i = threadIdx.x; i < TR_TILE * TR_TILE; i += 256) {
    const int rr = i / TR_TILE, c = i % TR_TILE;                   // coalesced read along the replicas
    tile[rr][c] = (row0 + rr < rows && rep0 + c < n_rep) ? nstate[(size_t)(row0 + rr) * pad + rep0 + c] : 0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TR_TILE * TR_TILE; i += 256) {
    const int c = i / TR_TILE, rr = i % TR_TILE;                   // contiguous write along the rows of one replica
    const int rep = rep0 + c, row = row0 + rr;
    if (rep < n_rep && row < rows) out[(size_t)rep * rows + row] = map[tile[rr][c]];
  }
}

}  // namespace

hipError_t launch_simulate(const SimParams& p, hipStream_t stream, int maps_mode) {
  const dim3 grid((p.n_rep + SIM_BLOCK - 1) / SIM_BLOCK);
  with_producer_form(maps_mode, p.n_states, [&](auto mode, auto ns) {
    hipLaunchKernelGGL((sim_kernel<decltype(ns)::value, decltype(mode)::value>), grid, dim3(SIM_BLOCK), 0, stream, p);
  });
  return hipGetLastError();
}

hipError_t launch_sim_transpose(const uint8_t* nstate, int rows, int n_rep, int n_rep_pad, const int32_t* map, int32_t* out,
                                hipStream_t stream) {
  if (rows <= 0 || n_rep <= 0) return hipSuccess;
  const dim3 grid((rows + TR_TILE - 1) / TR_TILE, (n_rep + TR_TILE - 1) / TR_TILE);
  hipLaunchKernelGGL(sim_transpose_kernel, grid, dim3(256), 0, stream, nstate, rows, n_rep, n_rep_pad, map, out);
  return hipGetLastError();
}

}  // namespace phm
