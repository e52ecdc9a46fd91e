// phm_sample.hip -- exact, independent draws of histories given the tips, for many rate matrices and sites in one call
// (DESIGN.md section 19): the top-down draw of every node's state (tips included) from section 17's P_k(t_b) and partial
// likelihoods L, read in place, and an end-point-conditioned uniformization sampler of every branch that has no jump cap, takes
// no exp(-mu t) and divides by no P[a, e], so that mu t in the thousands is sampled exactly.
//
// One lane is one history; a tile is 64 consecutive draws of ONE evaluation (model k, site s), so k and the evaluation are
// wave-uniform offsets into the model-fastest buffers and a lane's own states pick one of at most n^2 addresses per load.  Every
// random number is addressed by (seed, entity, GLOBAL evaluation id, draw index): nothing about tiles, chunks or devices enters.
//
// Branch (a, e, t), x = mu_k t, beta_m[c] = (B_k^m)[c, e] from the table:
//   jump count   N = first m with u S <= cum_m, cum_m = sum_{j <= m} r_j beta_j[a], S = cum_M the series' OWN total at the
//                stopping index M(x) (sm_stop_index, evaluated inline in the first pass); r, cum (and the Poisson sum of the rule)
//                are divided by 2^512 whenever r passes 2^512, and a partial sum taken before a later division is compared
//                after the divisions that followed it (exact powers of two);
//   jump times   T_i = t (c_i / G), c_i = E_1 + .. + E_i, G = c_{N+1}: normalised exponential spacings, taken twice from their
//                counter-addressed draws (G first, then the walk); no sort, no scratch;
//   states       x_i drawn with weights B[x_{i-1}, c] beta_{N-i}[c]; equal neighbours merge.
// Draw d of a branch stream: 0 the jump count, 1 .. N + 1 the exponentials, N + 1 + i the state x_i.
// Segments, counts and dwell sums are exp_tiles_branch_kernel's (64-bit fixed point; maps modes of phm_maps.h).
// The draw of a branch itself (sm_draw, sm_jump_count, sm_walk) is in phm_sample_branch.h (section 19a), shared with
// phm_sample_wide.hip; the finish kernel here serves both samplers.
//
// Packed form (PACKED = true, DESIGN.md section 20, behind phm_gibbs_rates): one draw per evaluation, so lane = chain.  A tile is 64
// consecutive chains of one site; the model, the evaluation, its id, mu, the table depth and the beta column are per lane
// (sm_lane); the buffers are model-fastest, so lanes that agree on (a, e) still load coalesced rows.  Same draws, same
// arithmetic: lane l of a packed tile computes what lane 0 of the unpacked tile of its evaluation computes.
#include "phm_sample.h"

#include <algorithm>

#include "phm_history.h"
#include "phm_ll_device.h"
#include "phm_sample_branch.h"

namespace phm {

namespace {

__global__ __launch_bounds__(SM_BLOCK) void sm_table_kernel(SmParams p) {
  const LlParams& q = p.ll;
  const int k = blockIdx.x * SM_BLOCK + threadIdx.x;
  if (k >= q.Kp) return;
  const int n = q.n, nn = n * n;
  const size_t Kp = q.Kp;
  const double mu = model_mu(q.Q + k, Kp, n);
  p.mu[k] = mu;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const double d = i == j ? 1.0 : 0.0;
      p.B[(size_t)(i * n + j) * Kp + k] = model_b(q.Q[(size_t)(i * n + j) * Kp + k], mu, d);
      p.beta[(size_t)(i * n + j) * Kp + k] = d;
    }
  int depth;
  if (p.packed) {                                                   // the chain's own depth, from the rates it has now
    depth = sm_stop_index(mu * p.t_max);
    if (depth > p.depth) { atomicOr(p.core.err, DERR_CAPACITY); depth = p.depth; }
    p.depth_of[k] = depth;
  } else {
    depth = min(p.depth_of[k], p.depth);
  }
  for (int m = 0; m < depth; ++m) {                                 // beta_{m+1} = B beta_m, unfused left-to-right sums
    const double* __restrict__ prev = p.beta + (size_t)m * nn * Kp + k;
    double* __restrict__ next = p.beta + (size_t)(m + 1) * nn * Kp + k;
    for (int c = 0; c < n; ++c)
      for (int e = 0; e < n; ++e) {
        double acc = p.B[(size_t)(c * n) * Kp + k] * prev[(size_t)e * Kp];
        for (int j = 1; j < n; ++j) acc += p.B[(size_t)(c * n + j) * Kp + k] * prev[(size_t)(j * n + e) * Kp];
        next[(size_t)(c * n + e) * Kp] = acc;
      }
  }
}

template <int NS>
__device__ __forceinline__ int sm_draw_n(const double* a, size_t sa, const double* b, size_t sb, int n, double u, uint32_t& err) {
  if constexpr (NS > 0) return sm_draw<NS>(a, sa, b, sb, n, u, err);
  switch (n) {                                                     // the node draws are launched with the run-time n
    case 2: return sm_draw<2>(a, sa, b, sb, n, u, err);
    case 3: return sm_draw<3>(a, sa, b, sb, n, u, err);
    case 4: return sm_draw<4>(a, sa, b, sb, n, u, err);
    default: return sm_draw<0>(a, sa, b, sb, n, u, err);
  }
}

// what a lane works on: wave-uniform in the tile form, its own chain in the packed form
struct SmLane {
  int k, ev;
  uint32_t eval_id, rep;
  bool valid;
};
template <bool PACKED>
__device__ __forceinline__ SmLane sm_lane(const SmParams& p, const SmTile& tl, int tile, int lane) {
  SmLane l;
  if constexpr (PACKED) {
    l.k = tl.k + lane;
    l.ev = tl.ev + lane;
    l.eval_id = p.lane_id[(size_t)tile * 64 + lane];
    l.rep = p.core.replica;
    l.valid = l.eval_id != SM_LANE_IDLE && isfinite(p.ll.ll[l.ev]);
  } else {
    l.k = tl.k;
    l.ev = tl.ev;
    l.eval_id = tl.eval_id;
    l.rep = (uint32_t)(tl.d0 + lane) + p.core.replica;
    l.valid = lane < tl.n_valid;
  }
  return l;
}

template <bool PACKED>
__global__ __launch_bounds__(SM_BLOCK) void sm_root_kernel(SmParams p) {
  const LlParams& q = p.ll;
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * (SM_BLOCK / 64) + (threadIdx.x >> 6);
  if (tile >= p.core.n_tiles) return;
  const SmTile tl = p.core.tiles[tile];
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp;
  const int NT = q.n_tips + p.core.n_node;
  const SmLane l = sm_lane<PACKED>(p, tl, tile, lane);
  uint32_t err = 0;
  int s = 0;
  if (!PACKED || l.valid) {
    const double u = stream_u(p.core.seed_lo, p.core.seed_hi, l.rep, l.eval_id, ENT_NODE | (uint32_t)p.core.root_row, 0);
    s = sm_draw_n<0>(q.pid + l.k, Kp, q.L + (size_t)p.core.root_row * q.n * Ev + l.ev, Ev, q.n, u, err);
  }
  p.core.nstate[((size_t)tile * NT + p.core.root_row) * 64 + lane] = (uint8_t)s;
  if (err && l.valid) atomicOr(p.core.err, err);
}

// one depth level: a wave per (tile, edge of the level) draws the child's state, tips included
template <bool PACKED>
__global__ __launch_bounds__(SM_BLOCK) void sm_node_kernel(SmParams p, int begin, int end) {
  const LlParams& q = p.ll;
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * (SM_BLOCK / 64) + (threadIdx.x >> 6);
  const int n_lvl = end - begin;
  if (item >= (int64_t)n_lvl * p.core.n_tiles) return;
  const int n = q.n;
  const int tile = (int)(item / n_lvl);
  const DownStep ds = p.core.down[p.core.order[begin + (int)(item % n_lvl)]];
  const SmTile tl = p.core.tiles[tile];
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp;
  const int NT = q.n_tips + p.core.n_node;
  const int crow = ds.child >= 0 ? q.n_tips + ds.child : ~ds.child;
  uint8_t* __restrict__ nst = p.core.nstate + (size_t)tile * NT * 64;
  const int a = nst[(q.n_tips + ds.parent) * 64 + lane];
  const SmLane l = sm_lane<PACKED>(p, tl, tile, lane);
  uint32_t err = 0;
  int e = 0;
  if (!PACKED || l.valid) {
    const double u = stream_u(p.core.seed_lo, p.core.seed_hi, l.rep, l.eval_id, ENT_NODE | (uint32_t)crow, 0);
    e = sm_draw_n<0>(q.P + ((size_t)ds.edge * n * n + (size_t)a * n) * Kp + l.k, Kp, q.L + (size_t)crow * n * Ev + l.ev, Ev, n, u, err);
  }
  nst[crow * 64 + lane] = (uint8_t)e;
  if (err && l.valid) atomicOr(p.core.err, err);
}

// persistent waves over (tile, group of `group` consecutive branches in pre-order); the branch draw is phm_sample_branch.h's
template <int NS, int MODE, bool PACKED = false>
__global__ __launch_bounds__(SM_BLOCK) void sm_branch_kernel(SmParams p, int group) {
  __shared__ __align__(16) double s_ltab[2 * PHM_LOGTAB_N];        // (1/c_j, log c_j) of the exponential variates (neglog_u32)
  for (int i = threadIdx.x; i < 2 * PHM_LOGTAB_N; i += SM_BLOCK) s_ltab[i] = logtab_entry(i);
  __syncthreads();
  const LlParams& q = p.ll;
  const SmCore& sc = p.core;
  const int lane = threadIdx.x & 63;
  const int wslot = blockIdx.x * (SM_BLOCK / 64) + (threadIdx.x >> 6);
  const int n = NS > 0 ? NS : q.n;
  const int nn = n * n;
  const size_t Kp = q.Kp;
  const int NT = q.n_tips + sc.n_node;
  const int n_groups = (sc.n_edge + group - 1) / group;
  const int64_t items = (int64_t)n_groups * sc.n_tiles;
  const size_t npad = (size_t)sc.n_tiles * 64;
  uint32_t err = 0;
  for (int64_t item = wslot; item < items; item += (int64_t)gridDim.x * (SM_BLOCK / 64)) {
    const int tile = (int)(item % sc.n_tiles);
    const int q0 = (int)(item / sc.n_tiles) * group, q1 = min(q0 + group, sc.n_edge);
    const SmTile tl = sc.tiles[tile];
    const size_t it = (size_t)tile * 64 + lane;
    const SmLane l = sm_lane<PACKED>(p, tl, tile, lane);
    const bool valid = l.valid;
    const uint8_t* __restrict__ nst = sc.nstate + (size_t)tile * NT * 64;
    const double mu = p.mu[l.k];
    const int depth = min(p.depth_of[l.k], p.depth);
    // model-fastest: B[c, j] at (c n + j) Kp + k, (B^m)[c, e] at (m nn + c n + e) Kp + k
    const SmTable<size_t> tab = {p.B + l.k, (size_t)n * Kp, Kp, p.beta + l.k, (size_t)nn * Kp, (size_t)n * Kp, Kp};
    StatLanes<NS, NS * (NS - 1)> st;
    st.begin(sc.dwfx, sc.cnt, npad, it, sc.fx_scale, valid);
    auto count = [&](int from, int to) { st.count(from * (n - 1) + (to > from ? to - 1 : to)); };
    for (int qi = q0; qi < q1; ++qi) {
      const DownStep ds = sc.down[qi];
      const int b = ds.edge;
      const int crow = ds.child >= 0 ? q.n_tips + ds.child : ~ds.child;
      const int a = nst[(q.n_tips + ds.parent) * 64 + lane];
      const int e = nst[crow * 64 + lane];
      const double tb = q.t[b];
      MapRow<MODE> mr;                                             // a lane without a live history: an empty row, no count stored
      mr.begin(sc.maps, (tl.row0 + lane) * sc.n_edge + b, valid);
      auto segment = [&](int col, double v) { st.dwell(col, v); mr.emit(v, col); };
      const double x = (!PACKED || valid) ? mu * tb : 0.0;         // packed: a lane without a live chain walks no series
      Stream sr;
      sr.open(ENT_BUNIF | (uint32_t)b, l.eval_id, l.rep, sc.seed_lo, sc.seed_hi);
      const int N = x > 0.0 ? sm_jump_count(tab, a, e, x, depth, sr, err) : 0;     // mu = 0 or t = 0: no jump
      sm_walk<NS>(tab, n, a, e, tb, N, sr, s_ltab, err, segment, count);
      if (valid) mr.end((size_t)b * sc.map_pad + (size_t)(tl.row0 + lane));
    }
    st.flush();
  }
  if (err) atomicOr(sc.err, err);
}

__global__ __launch_bounds__(256) void sm_finish_kernel(SmCore sc, int n, int n_tips, const double* packed_ll) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int cols = n + n * (n - 1);
  const int64_t npad = (int64_t)sc.n_tiles * 64;
  const int NT = n_tips + sc.n_node;
  if (gid < cols * npad) {
    const int c = (int)(gid / npad);
    const int64_t it = gid % npad;
    sc.out[gid] = stat_cell_value(sc.dwfx, sc.cnt, n, c, (size_t)npad, (size_t)it, sc.fx_inv);
    if (packed_ll) {                                                 // the next iteration accumulates from zero
      if (c < n) sc.dwfx[(size_t)c * npad + it] = 0ull;
      else sc.cnt[(size_t)(c - n) * npad + it] = 0u;
    }
  }
  if (packed_ll) {                                                   // one download per iteration: the lanes' ll and the error word ride along
    if (gid < npad) sc.out[(int64_t)cols * npad + gid] = packed_ll[sc.tiles[gid >> 6].ev + (int)(gid & 63)];
    if (gid == 0) sc.out[(int64_t)(cols + 1) * npad] = (double)*sc.err;
  }
  if (sc.nodes) {
    for (int64_t cell = gid; cell < npad * NT; cell += (int64_t)gridDim.x * blockDim.x) {
      const int64_t it = cell / NT;
      const int row = (int)(cell % NT);
      sc.nodes[cell] = (int32_t)sc.nstate[((size_t)(it >> 6) * NT + row) * 64 + (it & 63)] + 1;
    }
  }
}

}  // namespace

hipError_t launch_sm_finish(const SmCore& c, int n, int n_tips, const double* packed_ll, hipStream_t stream) {
  const int64_t cells = (int64_t)(n + n * (n - 1)) * c.n_tiles * 64;
  hipLaunchKernelGGL(sm_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, c, n, n_tips, packed_ll);
  return hipGetLastError();
}

hipError_t launch_sm_table(const SmParams& p, hipStream_t stream) {
  if (p.ll.n < 2 || p.ll.n > LL_LANE_MAX || p.ll.Kp <= 0 || p.ll.Kp % 64 || p.depth < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sm_table_kernel, dim3((p.ll.Kp + SM_BLOCK - 1) / SM_BLOCK), dim3(SM_BLOCK), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_sm_sample(const SmParams& p, const std::vector<int32_t>& level_off, int branch_blocks, int maps_mode,
                            hipStream_t stream) {
  if (p.ll.n < 2 || p.ll.n > LL_LANE_MAX || p.core.n_tiles <= 0 || branch_blocks <= 0) return hipErrorInvalidValue;
  if (p.packed && (maps_mode != MAPS_OFF || !p.lane_id || p.core.nodes)) return hipErrorInvalidValue;
  constexpr int W = SM_BLOCK / 64;
  const dim3 root_grid((p.core.n_tiles + W - 1) / W);
  if (p.packed) hipLaunchKernelGGL(sm_root_kernel<true>, root_grid, dim3(SM_BLOCK), 0, stream, p);
  else hipLaunchKernelGGL(sm_root_kernel<false>, root_grid, dim3(SM_BLOCK), 0, stream, p);
  for (size_t l = 0; l + 1 < level_off.size(); ++l) {
    const int64_t cnt = level_off[l + 1] - level_off[l];
    if (cnt <= 0) continue;
    const dim3 grid((unsigned)((cnt * p.core.n_tiles + W - 1) / W));
    if (p.packed) hipLaunchKernelGGL(sm_node_kernel<true>, grid, dim3(SM_BLOCK), 0, stream, p, level_off[l], level_off[l + 1]);
    else hipLaunchKernelGGL(sm_node_kernel<false>, grid, dim3(SM_BLOCK), 0, stream, p, level_off[l], level_off[l + 1]);
  }
  // branches per wave-item: as many as still leave every SIMD a few waves
  const int group = (int)std::max<int64_t>(1, std::min<int64_t>(16, (int64_t)p.core.n_edge * p.core.n_tiles / 8192));
  with_producer_form(maps_mode, p.ll.n, [&](auto mode, auto ns) {      // the packed form has no maps (checked above)
    constexpr int NS = decltype(ns)::value, MODE = decltype(mode)::value;
    if (p.packed) hipLaunchKernelGGL((sm_branch_kernel<NS, MAPS_OFF, true>), dim3(branch_blocks), dim3(SM_BLOCK), 0, stream, p, group);
    else hipLaunchKernelGGL((sm_branch_kernel<NS, MODE, false>), dim3(branch_blocks), dim3(SM_BLOCK), 0, stream, p, group);
  });
  return launch_sm_finish(p.core, p.ll.n, p.ll.n_tips, p.packed ? p.ll.ll : nullptr, stream);
}

}  // namespace phm
