// phm_mcmc_maps.hip -- the replay kernels of the MCMC stochastic maps (see phm_mcmc_maps.h).
//
// One lane per replica, one wave per (tile of 64 replicas, group of branches), the branch kernel's own (tile, group) items.  A lane
// walks its m_b old segments one after the other (no limit of 64 merged segments: the same loop serves the LONG form and the
// general path of the branch kernels) and draws state i exactly as the branch kernel does:
//   s_i ~ B[s_{i-1}, :] (.) B^(m-i-1) e_end,  u = word i - 1 of the ENT_BSTATE | b stream,  s_{m-1} = the child's end state,
// the first segment in the parent's state unless m = 1 (child wins, updatenodestates :469-472).  Merging adds the old dwells left
// to right, as pass A of the branch kernels does.
#include "phm_mcmc_maps.h"

#include <algorithm>

namespace phm {

namespace {

constexpr int MM_BLOCK = 256;

// The walk of one (branch, lane): emit(dwell, state) per merged segment, parent end first.
template <class Draw, class Emit>
__device__ __forceinline__ void replay_branch(int m, int ps, int cs, const double* __restrict__ in, Stream& su, Draw draw, Emit emit) {
  int cur_s = (m == 1) ? cs : ps;
  double cur_len = in[0];
  for (int i = 1; i < m; ++i) {
    const int si = (i == m - 1) ? cs : draw(i, cur_s, su.draw_word((uint32_t)(i - 1)));
    const double di = in[(size_t)i * 64];
    if (si == cur_s) cur_len = cur_len + di;                                   // shortener :54
    else { emit(cur_len, cur_s); cur_s = si; cur_len = di; }
  }
  emit(cur_len, cur_s);
}

// n <= 4: the tables of phm_tiles.hip (TileParams: B2 by value, col[k][end][NS])
template <int NS, int MODE>
__global__ __launch_bounds__(MM_BLOCK) void mcmc_maps_tiles_kernel(TileParams<NS> p, McmcMapsLaunch mp, int it) {
  __shared__ double s_B2[NS * NS];               // indexed by a per-lane state: LDS, not the kernarg segment
  if (threadIdx.x < NS * NS) s_B2[threadIdx.x] = p.B2[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * (MM_BLOCK / 64) + (threadIdx.x >> 6);
  if (item >= p.n_groups * p.n_tiles) return;
  const int tile = item % p.n_tiles, grp = item / p.n_tiles;
  const int r = tile * 64 + lane;
  if (r >= p.n_rep) return;
  const uint32_t rep = (uint32_t)(p.replica_offset + r);
  const int E = p.n_edge;
  const int q1 = min((grp + 1) * p.group, E);
  for (int q = grp * p.group; q < q1; ++q) {
    const int b = p.branch_order[q];
    const size_t eb = ((size_t)tile * E + b) * 64 + lane;
    const int m = p.mcount[eb];
    const int es = p.estate[eb];
    const int ps = es & 15, cs = es >> 4;
    const double* __restrict__ in = p.dw[it & 1] + ((size_t)tile * p.rows + p.slot[b]) * 64 + lane;
    Stream su;
    su.open(ENT_BSTATE | (uint32_t)b, (uint32_t)it, rep, p.seed_lo, p.seed_hi);
    const int64_t k = ((int64_t)r * mp.J + mp.j) * E + b;
    MapRow<MODE> mr;
    mr.begin(mp.dev, k);
    uint32_t err = 0;                            // the branch kernel reports the sweep's errors
    auto draw = [&](int i, int sprev, uint32_t word) -> int {
      const int kk = min(m - i - 1, p.klong - 1);
      const double* beta = p.colL + ((size_t)kk * NS + cs) * NS;
      double pr[NS];
#pragma unroll
      for (int c = 0; c < NS; ++c) pr[c] = s_B2[sprev * NS + c] * beta[c];
      return sample_cat<NS>(pr, u01(word), err);
    };
    replay_branch(m, ps, cs, in, su, draw, [&](double len, int s) { mr.emit(len, s); });
    mr.end(((size_t)mp.j * E + b) * p.n_rep_pad + r);
  }
}

// 5..64 states: the tables of phm_wtiles.hip.  The draw finds the block of eight states its threshold falls into from the running
// sums blkL and walks that block, as wt_branch_kernel does (the same partial sums as sample_cat's full scan, hence the same state).
template <int MODE>
__global__ __launch_bounds__(MM_BLOCK) void mcmc_maps_wtiles_kernel(WtParams p, McmcMapsLaunch mp, int it) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * (MM_BLOCK / 64) + (threadIdx.x >> 6);
  if (item >= p.n_groups * p.n_tiles) return;
  const int tile = item % p.n_tiles, grp = item / p.n_tiles;
  const int r = tile * 64 + lane;
  if (r >= p.n_rep) return;
  const uint32_t rep = (uint32_t)(p.replica_offset + r);
  const int E = p.n_edge, n = p.n_states, ldt = p.ldt, nb = p.nblk;
  const int q1 = min((grp + 1) * p.group, E);
  for (int q = grp * p.group; q < q1; ++q) {
    const int b = p.branch_order[q];
    const size_t eb = ((size_t)tile * E + b) * 64 + lane;
    const int m = p.mcount[eb];
    const int es = p.estate[eb];
    const int ps = es & 255, cs = es >> 8;
    const double* __restrict__ in = p.dw[it & 1] + ((size_t)tile * p.rows + p.slot[b]) * 64 + lane;
    Stream su;
    su.open(ENT_BSTATE | (uint32_t)b, (uint32_t)it, rep, p.seed_lo, p.seed_hi);
    const int64_t k = ((int64_t)r * mp.J + mp.j) * E + b;
    MapRow<MODE> mr;
    mr.begin(mp.dev, k);
    auto draw = [&](int i, int sprev, uint32_t word) -> int {
      const int kk = min(m - i - 1, p.klong - 1);
      const double* __restrict__ blk = p.blkL + (((size_t)kk * n + sprev) * n + cs) * p.ldb;
      const double thr = u01(word) * blk[nb - 1];                             // the last kept sum is the total
      int b0 = 0;
      double cum = 0.0;
      for (int qq = 0; qq < nb - 1; ++qq) {                                    // running sums only grow: blocks wholly below thr
        const double e = blk[qq];
        const bool below = !(thr <= e);
        b0 += below ? 1 : 0;
        cum = below ? e : cum;
      }
      const int c0 = 8 * b0, c1 = min(c0 + 8, n - 1);                          // comparisons at states 0 .. n-2 decide (sample_cat)
      const double* __restrict__ beta = p.colL + ((size_t)kk * n + cs) * ldt;
      const double* __restrict__ brow = p.B2 + (size_t)sprev * ldt;
      int idx = c0;
      for (int c = c0; c < c1; ++c) {
        cum += brow[c] * beta[c];
        idx += !(thr <= cum) ? 1 : 0;
      }
      return idx;
    };
    replay_branch(m, ps, cs, in, su, draw, [&](double len, int s) { mr.emit(len, s); });
    mr.end(((size_t)mp.j * E + b) * p.n_rep_pad + r);
  }
}

// out[b][s*J + j] = cnt[j][b][s]: a thread per history, the edges of a chunk of rows per block row
__global__ __launch_bounds__(256) void mcmc_maps_transpose_kernel(const uint16_t* __restrict__ cnt, int S, int J, int E, int pad,
                                                                  uint16_t* __restrict__ out) {
  const int64_t H = (int64_t)S * J;
  const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (h >= H) return;
  const int s = (int)(h / J), j = (int)(h % J);
  for (int b = blockIdx.y; b < E; b += gridDim.y) out[(size_t)b * H + h] = cnt[((size_t)j * E + b) * pad + s];
}

}  // namespace

template <int NS>
hipError_t launch_mcmc_maps_tiles(const TileParams<NS>& p, const McmcMapsLaunch& m, int it, hipStream_t stream) {
  const dim3 g((unsigned)(((int64_t)p.n_groups * p.n_tiles + MM_BLOCK / 64 - 1) / (MM_BLOCK / 64)));
  if (m.mode != MAPS_COUNT && m.mode != MAPS_WRITE) return hipErrorInvalidValue;
  with_map_mode(m.mode, [&](auto mode) {
    if constexpr (mode != MAPS_OFF) hipLaunchKernelGGL((mcmc_maps_tiles_kernel<NS, mode>), g, dim3(MM_BLOCK), 0, stream, p, m, it);
  });
  return hipGetLastError();
}

template hipError_t launch_mcmc_maps_tiles<2>(const TileParams<2>&, const McmcMapsLaunch&, int, hipStream_t);
template hipError_t launch_mcmc_maps_tiles<3>(const TileParams<3>&, const McmcMapsLaunch&, int, hipStream_t);
template hipError_t launch_mcmc_maps_tiles<4>(const TileParams<4>&, const McmcMapsLaunch&, int, hipStream_t);

hipError_t launch_mcmc_maps_wtiles(const WtParams& p, const McmcMapsLaunch& m, int it, hipStream_t stream) {
  const dim3 g((unsigned)(((int64_t)p.n_groups * p.n_tiles + MM_BLOCK / 64 - 1) / (MM_BLOCK / 64)));
  if (m.mode != MAPS_COUNT && m.mode != MAPS_WRITE) return hipErrorInvalidValue;
  with_map_mode(m.mode, [&](auto mode) {
    if constexpr (mode != MAPS_OFF) hipLaunchKernelGGL((mcmc_maps_wtiles_kernel<mode>), g, dim3(MM_BLOCK), 0, stream, p, m, it);
  });
  return hipGetLastError();
}

hipError_t launch_mcmc_maps_transpose(const uint16_t* cnt, int S, int J, int E, int pad, uint16_t* out, hipStream_t stream) {
  const int64_t H = (int64_t)S * J;
  if (H <= 0 || E <= 0) return hipSuccess;
  const dim3 g((unsigned)((H + 255) / 256), (unsigned)std::min(E, 1024));
  hipLaunchKernelGGL(mcmc_maps_transpose_kernel, g, dim3(256), 0, stream, cnt, S, J, E, pad, out);
  return hipGetLastError();
}

}  // namespace phm
