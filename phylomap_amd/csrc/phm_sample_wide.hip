// phm_sample_wide.hip -- exact, independent draws of histories given the tips for many rate matrices and sites at 9..64 states
// (DESIGN.md section 24): section 19's sampler (phm_sample.hip) with the run-time state count, on section 23's buffers.  P_k(t_b)
// is [model][edge][n][n] row-major and L is [node row][Ev][NP] as phm_ancestral_wide.hip leaves them; both are read in place.
//
// The unit of work is section 19's: a tile is 64 consecutive draws of ONE evaluation and a lane is one history, so the model is
// wave-uniform and the serial per-history logic (the two-pass jump-count series, the time walk, the first-j categorical scan)
// needs no cross-lane step.  Every sum is left to right over explicit products (the library is built with -ffp-contract=off).
//
//   table    a workgroup owns a model: mu_k, B_k = I + Q_k / mu_k and beta_m = B^m for m = 0 .. M(mu_k max t_b).  Row m is stored
//            [e][c] = (B^m)[c, e], so the n weights beta_m[., e] of one state draw are a contiguous run.  beta_m and beta_{m+1}
//            ping-pong in LDS: step m + 1 reads what step m wrote there, never its own global stores.
//   root     a wave per tile; pid_k and L_root are wave-uniform.
//   nodes    one launch per depth level, a wave per (tile, edge of the level); L_child is wave-uniform, the lane gathers its
//            parent state's row of P.
//   branch   a one-wave workgroup per (tile, branch).  B_k is staged in LDS (row stride n | 1) only when a lane of the wave
//            drew two or more jumps, the one case in which a state is drawn; the neglog table sits in LDS.
//   finish   phm_sample.hip's kernel over the shared SmCore (launch_sm_finish).
// The categorical draw, the jump-count series and the walk are phm_sample_branch.h's (section 19a), shared with phm_sample.hip.
// Bounds: the series' loops end at the table depth (DERR_CAPACITY beyond it, nothing is read past the table), the walk at N <= M.
#include "phm_sample_wide.h"

#include <algorithm>

#include "phm_aw_device.h"
#include "phm_history.h"
#include "phm_sample_branch.h"

namespace phm {

namespace {

// grid: model.  LDS: B [n][n | 1], two rows of the table [e][c].
__global__ __launch_bounds__(SW_TABLE_BLOCK) void sw_table_kernel(SwParams p) {
  extern __shared__ __align__(16) double sw_lds[];
  __shared__ double s_mu;
  const int n = p.n, nn = n * n, LD = sw_row_stride(n);
  const int k = blockIdx.x;
  double* sB = sw_lds;
  double* prev = sB + n * LD;
  double* next = prev + nn;
  const double* __restrict__ Qk = p.Q + (size_t)k * nn;
  if (threadIdx.x == 0) {
    s_mu = model_mu(Qk, 1, n);
    p.mu[k] = s_mu;
  }
  __syncthreads();
  const double mu = s_mu;
  const int depth = p.depth_of[k];
  double* __restrict__ tab = p.beta + (size_t)k * p.tab_stride;
  for (int cell = threadIdx.x; cell < nn; cell += SW_TABLE_BLOCK) {
    const int i = cell / n, j = cell - i * n;
    const double d = i == j ? 1.0 : 0.0;
    const double b = model_b(Qk[cell], mu, d);
    p.B[(size_t)k * nn + cell] = b;
    sB[i * LD + j] = b;
    prev[cell] = d;                                                  // beta_0 = I (symmetric: [e][c] as well)
    tab[cell] = d;
  }
  __syncthreads();
  for (int m = 0; m < depth; ++m) {                                  // beta_{m+1} = B beta_m, unfused left-to-right sums
    double* __restrict__ row = tab + (size_t)(m + 1) * nn;
    for (int cell = threadIdx.x; cell < nn; cell += SW_TABLE_BLOCK) {
      const int e = cell / n, c = cell - e * n;
      const double* b = sB + c * LD;
      const double* v = prev + e * n;
      double acc = b[0] * v[0];
      for (int j = 1; j < n; ++j) acc += b[j] * v[j];
      next[cell] = acc;
      row[cell] = acc;
    }
    __syncthreads();                                                 // the hand-over: every cell of beta_{m+1} is in LDS
    double* s = prev; prev = next; next = s;
  }
}

// What a lane works on.  Draw-lanes form: the tile's one evaluation, the lane's draw.  Sites form (SITES = true, section 25, behind
// phm_gibbs_rates_wide): a tile is 64 consecutive sites of ONE chain and every lane has ONE draw, so the model stays
// wave-uniform while the evaluation (row tl.ev + lane of L and of ll) and its id (tl.eval_id + lane * lane_stride, site * C +
// chain) are the lane's.  A sites lane is live when it is below n_valid and its evaluation's log-likelihood is finite; one that is
// not loads no row of L or ll (the last chain's last tile would index past Ev) and keeps the fixed states a = e = 0, N = 0.
struct SwLane {
  size_t ev;
  uint32_t eval_id, rep;
  bool valid;
};
template <bool SITES>
__device__ __forceinline__ SwLane sw_lane(const SwParams& p, const SmTile& tl, int lane) {
  SwLane l;
  if constexpr (SITES) {
    l.valid = lane < tl.n_valid;
    l.ev = (size_t)tl.ev + (l.valid ? lane : 0);
    if (l.valid) l.valid = isfinite(p.ll[l.ev]);
    l.eval_id = tl.eval_id + (uint32_t)lane * p.lane_stride;
    l.rep = p.core.replica;
  } else {
    l.valid = lane < tl.n_valid;
    l.ev = (size_t)tl.ev;
    l.eval_id = tl.eval_id;
    l.rep = (uint32_t)(tl.d0 + lane) + p.core.replica;
  }
  return l;
}

template <bool SITES>
__global__ __launch_bounds__(SW_NODE_BLOCK) void sw_root_kernel(SwParams p) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * (SW_NODE_BLOCK / 64) + (threadIdx.x >> 6);
  if (tile >= p.core.n_tiles) return;
  const SmTile tl = p.core.tiles[tile];
  const int NT = p.n_tips + p.core.n_node;
  const SwLane l = sw_lane<SITES>(p, tl, lane);
  uint32_t err = 0;
  int s = 0;
  if (!SITES || l.valid) {
    const double u = stream_u(p.core.seed_lo, p.core.seed_hi, l.rep, l.eval_id, ENT_NODE | (uint32_t)p.core.root_row, 0);
    s = sm_draw<0>(p.pid + (size_t)tl.k * p.n, 1, p.L + ((size_t)p.core.root_row * p.Ev + l.ev) * p.NP, 1, p.n, u, err);
  }
  p.core.nstate[((size_t)tile * NT + p.core.root_row) * 64 + lane] = (uint8_t)s;
  if (err && l.valid) atomicOr(p.core.err, err);
}

// one depth level: a wave per (tile, edge of the level) draws the child's state, tips included
template <bool SITES>
__global__ __launch_bounds__(SW_NODE_BLOCK) void sw_node_kernel(SwParams p, int begin, int end) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * (SW_NODE_BLOCK / 64) + (threadIdx.x >> 6);
  const int n_lvl = end - begin;
  if (item >= (int64_t)n_lvl * p.core.n_tiles) return;
  const int n = p.n;
  const int tile = (int)(item / n_lvl);
  const DownStep ds = p.core.down[p.core.order[begin + (int)(item % n_lvl)]];
  const SmTile tl = p.core.tiles[tile];
  const int NT = p.n_tips + p.core.n_node;
  const int crow = ds.child >= 0 ? p.n_tips + ds.child : ~ds.child;
  uint8_t* __restrict__ nst = p.core.nstate + (size_t)tile * NT * 64;
  const int a = nst[(p.n_tips + ds.parent) * 64 + lane];
  const SwLane l = sw_lane<SITES>(p, tl, lane);
  uint32_t err = 0;
  int e = 0;
  if (!SITES || l.valid) {
    const double u = stream_u(p.core.seed_lo, p.core.seed_hi, l.rep, l.eval_id, ENT_NODE | (uint32_t)crow, 0);
    e = sm_draw<0>(p.P + (((size_t)tl.k * p.core.n_edge + ds.edge) * n + a) * n, 1, p.L + ((size_t)crow * p.Ev + l.ev) * p.NP, 1, n, u, err);
  }
  nst[crow * 64 + lane] = (uint8_t)e;
  if (err && l.valid) atomicOr(p.core.err, err);
}

// grid: (tile, branch) items, tile fastest; a workgroup is one wave; the branch draw is phm_sample_branch.h's
template <int MODE, bool SITES = false>
__global__ __launch_bounds__(SW_BRANCH_BLOCK) void sw_branch_kernel(SwParams p) {
  extern __shared__ __align__(16) double sw_lds[];                   // B of the item's model, rows n | 1 apart
  __shared__ __align__(16) double s_ltab[2 * PHM_LOGTAB_N];          // (1/c_j, log c_j) of the exponential variates (neglog_u32)
  const SmCore& sc = p.core;
  const int lane = threadIdx.x;
  for (int i = lane; i < 2 * PHM_LOGTAB_N; i += SW_BRANCH_BLOCK) s_ltab[i] = logtab_entry(i);
  const int n = p.n, nn = n * n, LD = sw_row_stride(n);
  const int NT = p.n_tips + sc.n_node;
  const int64_t item = blockIdx.x;
  const int tile = (int)(item % sc.n_tiles);
  const DownStep ds = sc.down[(int)(item / sc.n_tiles)];
  const SmTile tl = sc.tiles[tile];
  const size_t npad = (size_t)sc.n_tiles * 64;
  const SwLane l = sw_lane<SITES>(p, tl, lane);
  const bool valid = l.valid;
  const uint8_t* __restrict__ nst = sc.nstate + (size_t)tile * NT * 64;
  const double mu = p.mu[tl.k];
  const int depth = p.depth_of[tl.k];
  const double* __restrict__ Bk = p.B + (size_t)tl.k * nn;
  // B in LDS, rows LD apart; the model's table, row m [e][c]: (B^m)[c, e] at m nn + e n + c
  const SmTable<SmUnit> tab = {sw_lds, (size_t)LD, {}, p.beta + (size_t)tl.k * p.tab_stride, (size_t)nn, {}, (size_t)n};
  const int b = ds.edge;
  const int crow = ds.child >= 0 ? p.n_tips + ds.child : ~ds.child;
  const int a = nst[(p.n_tips + ds.parent) * 64 + lane];             // sites form: 0 in a lane that is not live
  const int e = nst[crow * 64 + lane];
  const double tb = p.t[b];
  const double x = mu * tb;                                          // wave-uniform
  uint32_t err = 0;
  StatLanes<0, 0> st;
  st.begin(sc.dwfx, sc.cnt, npad, (size_t)tile * 64 + lane, sc.fx_scale, valid);
  MapRow<MODE> mr;                                                   // a lane without a live history: an empty row, no count stored
  mr.begin(sc.maps, (tl.row0 + lane) * sc.n_edge + b, valid);
  auto segment = [&](int col, double v) { st.dwell(col, v); mr.emit(v, col); };
  auto count = [&](int from, int to) { st.count(from * (n - 1) + (to > from ? to - 1 : to)); };
  Stream sr;
  sr.open(ENT_BUNIF | (uint32_t)b, l.eval_id, l.rep, sc.seed_lo, sc.seed_hi);
  // mu = 0 or t = 0: no jump; a sites lane that is not live reads no table and walks nothing
  const int N = (x > 0.0 && (!SITES || valid)) ? sm_jump_count(tab, a, e, x, depth, sr, err) : 0;
  if (__any(N >= 2)) {                                               // only then is a state drawn from B
    for (int i = lane; i < nn; i += SW_BRANCH_BLOCK) {
      const int row = i / n;
      sw_lds[row * LD + (i - row * n)] = Bk[i];
    }
  }
  __syncthreads();                                                   // the neglog table and B are staged
  sm_walk<0>(tab, n, a, e, tb, N, sr, s_ltab, err, segment, count);
  if (valid) mr.end((size_t)b * sc.map_pad + (size_t)(tl.row0 + lane));
  if (err && valid) atomicOr(sc.err, err);
}

// Sites form: finish and reduction of one iteration.  A lane owns one (chain, column) and walks the chain's sites in ascending
// order: the cell's value as section 19's finish takes it (fixed point -> double, counter -> double) is added to the lane's
// double, one site after the other, and the cell is zeroed for the next iteration.  Column `cols` is the chain's
// log-likelihood, summed over its evaluations in the same order.  red [chain][cols + 1], then the error word.  A chain's tiles
// are consecutive (tiles_per_chain of them, lane = site & 63), so site s of chain k is cell (k tiles_per_chain) 64 + s.
__global__ __launch_bounds__(256) void sw_reduce_kernel(SwParams p, int sites, int tiles_per_chain, double* __restrict__ red) {
  const SmCore& sc = p.core;
  const int cols = p.n + p.n * (p.n - 1);
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid == 0) red[(size_t)p.Kc * (cols + 1)] = (double)*sc.err;
  if (gid >= (int64_t)p.Kc * (cols + 1)) return;
  const int k = (int)(gid / (cols + 1)), c = (int)(gid - (int64_t)k * (cols + 1));
  const size_t npad = (size_t)sc.n_tiles * 64;
  double v = 0.0;
  if (c == cols) {
    const double* __restrict__ ll = p.ll + (size_t)k * sites;
    for (int s = 0; s < sites; ++s) v += ll[s];
  } else if (c < p.n) {
    unsigned long long* __restrict__ dw = sc.dwfx + (size_t)c * npad + (size_t)k * tiles_per_chain * 64;
    for (int s = 0; s < sites; ++s) { v += (double)(long long)dw[s] * sc.fx_inv; dw[s] = 0ull; }
  } else {
    uint32_t* __restrict__ ct = sc.cnt + (size_t)(c - p.n) * npad + (size_t)k * tiles_per_chain * 64;
    for (int s = 0; s < sites; ++s) { v += (double)ct[s]; ct[s] = 0u; }
  }
  red[gid] = v;
}

inline bool sw_ok(const SwParams& p) {
  return p.n >= AW_MIN_STATES && p.n <= EX_MAX_STATES && p.NP == aw_lanes(p.n) && p.Kc >= 1 && p.Kc <= AW_GRID_MAX && p.core.n_edge >= 1;
}

// root and node levels of the tiles of p, one launch per depth level
template <bool SITES>
void sw_nodes(const SwParams& p, const std::vector<int32_t>& level_off, hipStream_t stream) {
  constexpr int W = SW_NODE_BLOCK / 64;
  hipLaunchKernelGGL(sw_root_kernel<SITES>, dim3((p.core.n_tiles + W - 1) / W), dim3(SW_NODE_BLOCK), 0, stream, p);
  for (size_t l = 0; l + 1 < level_off.size(); ++l) {
    const int64_t cnt = level_off[l + 1] - level_off[l];
    if (cnt <= 0) continue;
    const dim3 grid((unsigned)((cnt * p.core.n_tiles + W - 1) / W));
    hipLaunchKernelGGL(sw_node_kernel<SITES>, grid, dim3(SW_NODE_BLOCK), 0, stream, p, level_off[l], level_off[l + 1]);
  }
}

}  // namespace

hipError_t launch_sw_table(const SwParams& p, hipStream_t stream) {
  if (!sw_ok(p) || !p.Q || !p.mu || !p.B || !p.beta || !p.depth_of || p.tab_stride < sw_table_doubles(p.n, 0)) return hipErrorInvalidValue;
  const hipError_t e = aw_allow_lds(reinterpret_cast<const void*>(sw_table_kernel), (int)sw_table_lds_bytes(EX_MAX_STATES));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sw_table_kernel, dim3(p.Kc), dim3(SW_TABLE_BLOCK), sw_table_lds_bytes(p.n), stream, p);
  return hipGetLastError();
}

hipError_t launch_sw_sample(const SwParams& p, const std::vector<int32_t>& level_off, int maps_mode, hipStream_t stream) {
  if (!sw_ok(p) || p.core.n_tiles <= 0 || (int64_t)p.core.n_edge * p.core.n_tiles > SW_ITEMS_MAX) return hipErrorInvalidValue;
  sw_nodes<false>(p, level_off, stream);
  const dim3 items((unsigned)((int64_t)p.core.n_edge * p.core.n_tiles));
  with_map_mode(maps_mode, [&](auto mode) {
    constexpr int MODE = decltype(mode)::value;
    hipLaunchKernelGGL((sw_branch_kernel<MODE>), items, dim3(SW_BRANCH_BLOCK), sw_branch_lds_bytes(p.n), stream, p);
  });
  return launch_sm_finish(p.core, p.n, p.n_tips, nullptr, stream);
}

hipError_t launch_sw_sample_sites(const SwParams& p, const std::vector<int32_t>& level_off, int sites, int tiles_per_chain, double* red,
                                  hipStream_t stream) {
  if (!sw_ok(p) || p.core.n_tiles <= 0 || (int64_t)p.core.n_edge * p.core.n_tiles > SW_ITEMS_MAX) return hipErrorInvalidValue;
  if (!p.ll || !red || p.core.nodes || sites < 1 || (size_t)p.Kc * sites != p.Ev || tiles_per_chain != (sites + 63) / 64 ||
      (int64_t)p.Kc * tiles_per_chain != p.core.n_tiles)
    return hipErrorInvalidValue;
  sw_nodes<true>(p, level_off, stream);
  const dim3 items((unsigned)((int64_t)p.core.n_edge * p.core.n_tiles));
  hipLaunchKernelGGL((sw_branch_kernel<MAPS_OFF, true>), items, dim3(SW_BRANCH_BLOCK), sw_branch_lds_bytes(p.n), stream, p);
  const int64_t cells = (int64_t)p.Kc * (p.n + p.n * (p.n - 1) + 1);
  hipLaunchKernelGGL(sw_reduce_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, p, sites, tiles_per_chain, red);
  return hipGetLastError();
}

}  // namespace phm
