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
//
// Packed form (PACKED = true, DESIGN.md section 20, behind phm_gibbs_rates): one draw per evaluation, so lane = chain.  A tile is 64
// consecutive chains of one site; the model, the evaluation, its id, mu, the table depth and the beta column are per lane
// (sm_lane); the buffers are model-fastest, so lanes that agree on (a, e) still load coalesced rows.  Same draws, same
// arithmetic: lane l of a packed tile computes what lane 0 of the unpacked tile of its evaluation computes.
#include "phm_sample.h"

#include <algorithm>

#include "phm_device.h"
#include "phm_history.h"

namespace phm {

namespace {

__global__ __launch_bounds__(SM_BLOCK) void sm_table_kernel(SmParams p) {
  const LlParams& q = p.ll;
  const int k = blockIdx.x * SM_BLOCK + threadIdx.x;
  if (k >= q.Kp) return;
  const int n = q.n, nn = n * n;
  const size_t Kp = q.Kp;
  double mu = 0.0;
  for (int i = 0; i < n; ++i) mu = fmax(mu, -q.Q[(size_t)(i * n + i) * Kp + k]);
  p.mu[k] = mu;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const double d = i == j ? 1.0 : 0.0;
      p.B[(size_t)(i * n + j) * Kp + k] = mu > 0.0 ? d + q.Q[(size_t)(i * n + j) * Kp + k] / mu : d;
      p.beta[(size_t)(i * n + j) * Kp + k] = d;
    }
  int depth;
  if (p.packed) {                                                   // the chain's own depth, from the rates it has now
    depth = sm_stop_index(mu * p.t_max);
    if (depth > p.depth) { atomicOr(p.err, DERR_CAPACITY); depth = p.depth; }
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

// first j with u * sum(w) <= w_0 + .. + w_j, w_c = a[c sa] * b[c sb], sums left to right (section 2's rule)
template <int NS>
__device__ __forceinline__ int sm_draw(const double* __restrict__ a, size_t sa, const double* __restrict__ b, size_t sb, int n,
                                       double u, uint32_t& err) {
  if constexpr (NS > 0) {
    double w[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) w[c] = a[c * sa] * b[c * sb];
    return sample_cat<NS>(w, u, err);
  } else {
    double total = a[0] * b[0];
    for (int c = 1; c < n; ++c) total += a[c * sa] * b[c * sb];
    if (!(total > 0.0) || isinf(total)) err |= DERR_ZERO_PROB;
    const double thr = u * total;
    double cum = a[0] * b[0];
    int idx = (thr <= cum) ? 0 : 1;
    for (int c = 1; c < n - 1; ++c) { cum += a[c * sa] * b[c * sb]; idx += (thr <= cum) ? 0 : 1; }
    return idx;
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
    l.rep = p.replica;
    l.valid = l.eval_id != SM_LANE_IDLE && isfinite(p.ll.ll[l.ev]);
  } else {
    l.k = tl.k;
    l.ev = tl.ev;
    l.eval_id = tl.eval_id;
    l.rep = (uint32_t)(tl.d0 + lane) + p.replica;
    l.valid = lane < tl.n_valid;
  }
  return l;
}

template <bool PACKED>
__global__ __launch_bounds__(SM_BLOCK) void sm_root_kernel(SmParams p) {
  const LlParams& q = p.ll;
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * (SM_BLOCK / 64) + (threadIdx.x >> 6);
  if (tile >= p.n_tiles) return;
  const SmTile tl = p.tiles[tile];
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp;
  const int NT = q.n_tips + p.n_node;
  const SmLane l = sm_lane<PACKED>(p, tl, tile, lane);
  uint32_t err = 0;
  int s = 0;
  if (!PACKED || l.valid) {
    const double u = stream_u(p.seed_lo, p.seed_hi, l.rep, l.eval_id, ENT_NODE | (uint32_t)p.root_row, 0);
    s = sm_draw_n<0>(q.pid + l.k, Kp, q.L + (size_t)p.root_row * q.n * Ev + l.ev, Ev, q.n, u, err);
  }
  p.nstate[((size_t)tile * NT + p.root_row) * 64 + lane] = (uint8_t)s;
  if (err && l.valid) atomicOr(p.err, err);
}

// one depth level: a wave per (tile, edge of the level) draws the child's state, tips included
template <bool PACKED>
__global__ __launch_bounds__(SM_BLOCK) void sm_node_kernel(SmParams p, int begin, int end) {
  const LlParams& q = p.ll;
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * (SM_BLOCK / 64) + (threadIdx.x >> 6);
  const int n_lvl = end - begin;
  if (item >= (int64_t)n_lvl * p.n_tiles) return;
  const int n = q.n;
  const int tile = (int)(item / n_lvl);
  const DownStep ds = p.down[p.order[begin + (int)(item % n_lvl)]];
  const SmTile tl = p.tiles[tile];
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp;
  const int NT = q.n_tips + p.n_node;
  const int crow = ds.child >= 0 ? q.n_tips + ds.child : ~ds.child;
  uint8_t* __restrict__ nst = p.nstate + (size_t)tile * NT * 64;
  const int a = nst[(q.n_tips + ds.parent) * 64 + lane];
  const SmLane l = sm_lane<PACKED>(p, tl, tile, lane);
  uint32_t err = 0;
  int e = 0;
  if (!PACKED || l.valid) {
    const double u = stream_u(p.seed_lo, p.seed_hi, l.rep, l.eval_id, ENT_NODE | (uint32_t)crow, 0);
    e = sm_draw_n<0>(q.P + ((size_t)ds.edge * n * n + (size_t)a * n) * Kp + l.k, Kp, q.L + (size_t)crow * n * Ev + l.ev, Ev, n, u, err);
  }
  nst[crow * 64 + lane] = (uint8_t)e;
  if (err && l.valid) atomicOr(p.err, err);
}

// persistent waves over (tile, group of `group` consecutive branches in pre-order)
template <int NS, int MODE, bool PACKED = false>
__global__ __launch_bounds__(SM_BLOCK) void sm_branch_kernel(SmParams p, int group) {
  __shared__ __align__(16) double s_ltab[2 * PHM_LOGTAB_N];        // (1/c_j, log c_j) of the exponential variates (neglog_u32)
  for (int i = threadIdx.x; i < 2 * PHM_LOGTAB_N; i += SM_BLOCK) s_ltab[i] = logtab_entry(i);
  __syncthreads();
  const LlParams& q = p.ll;
  const int lane = threadIdx.x & 63;
  const int wslot = blockIdx.x * (SM_BLOCK / 64) + (threadIdx.x >> 6);
  const int n = NS > 0 ? NS : q.n;
  const int nn = n * n;
  const size_t Kp = q.Kp;
  const int NT = q.n_tips + p.n_node;
  const int n_groups = (p.n_edge + group - 1) / group;
  const int64_t items = (int64_t)n_groups * p.n_tiles;
  const size_t npad = (size_t)p.n_tiles * 64;
  uint32_t err = 0;
  for (int64_t item = wslot; item < items; item += (int64_t)gridDim.x * (SM_BLOCK / 64)) {
    const int tile = (int)(item % p.n_tiles);
    const int q0 = (int)(item / p.n_tiles) * group, q1 = min(q0 + group, p.n_edge);
    const SmTile tl = p.tiles[tile];
    const size_t it = (size_t)tile * 64 + lane;
    const SmLane l = sm_lane<PACKED>(p, tl, tile, lane);
    const bool valid = l.valid;
    const uint8_t* __restrict__ nst = p.nstate + (size_t)tile * NT * 64;
    const double mu = p.mu[l.k];
    const int depth = min(p.depth_of[l.k], p.depth);
    const double* __restrict__ Bk = p.B + l.k;
    const double* __restrict__ bt = p.beta + l.k;
    const uint32_t rep = l.rep;
    StatLanes<NS, NS * (NS - 1)> st;
    st.begin(p.dwfx, p.cnt, npad, it, p.fx_scale, valid);
    auto count = [&](int from, int to) { st.count(from * (n - 1) + (to > from ? to - 1 : to)); };
    for (int qi = q0; qi < q1; ++qi) {
      const DownStep ds = p.down[qi];
      const int b = ds.edge;
      const int crow = ds.child >= 0 ? q.n_tips + ds.child : ~ds.child;
      const int a = nst[(q.n_tips + ds.parent) * 64 + lane];
      const int e = nst[crow * 64 + lane];
      const double tb = q.t[b];
      MapRow<MODE> mr;                                             // a lane without a live history: an empty row, no count stored
      mr.begin(p.maps, (tl.row0 + lane) * p.n_edge + b, valid);
      auto segment = [&](int col, double v) { st.dwell(col, v); mr.emit(v, col); };
      const double x = (!PACKED || valid) ? mu * tb : 0.0;         // packed: a lane without a live chain walks no series
      int N = 0;
      if (x > 0.0) {
        const double* __restrict__ ba = bt + (size_t)(a * n + e) * Kp;       // beta_m[a] at ba[m nn Kp]
        // first pass: the stopping index and the series' own total
        double r = 1.0, Sp = 1.0, Sa = ba[0];
        int R = 0, M = 0;
        for (int m = 1;; ++m) {
          const double rn = r * (x / (double)m);
          if (m >= 2 && x < (double)m && rn <= 0x1p-60 * Sp * (1.0 - x / (double)(m + 1))) break;
          if (m > depth) { err |= DERR_CAPACITY; break; }            // never with the host's depth: M is monotone in x
          r = rn;
          Sp += r;
          Sa += r * ba[(size_t)m * nn * Kp];
          M = m;
          if (r > 0x1p512) { r *= 0x1p-512; Sp *= 0x1p-512; Sa *= 0x1p-512; ++R; }
        }
        if (!(Sa > 0.0) || isinf(Sa)) err |= DERR_ZERO_PROB;
        Stream sr;
        sr.open(ENT_BUNIF | (uint32_t)b, l.eval_id, rep, p.seed_lo, p.seed_hi);
        const double thr = sr.draw(0) * Sa;
        // second pass: the first m whose partial sum reaches the threshold
        double cum = ba[0];
        int rho = 0;
        r = 1.0;
        if (!(thr <= ldexp(cum, -512 * R))) {
          N = M;
          for (int m = 1; m <= M; ++m) {
            r = r * (x / (double)m);
            cum += r * ba[(size_t)m * nn * Kp];
            if (r > 0x1p512) { r *= 0x1p-512; cum *= 0x1p-512; ++rho; }
            if (thr <= ldexp(cum, -512 * (R - rho))) { N = m; break; }
          }
        }
        if (N > 0) {
          // jump times: G = E_1 + .. + E_{N+1}, then the walk takes the same draws again
          double G = 0.0;
          for (int i = 1; i <= N + 1; ++i) G += neglog_u32(sr.draw_word((uint32_t)i), s_ltab);
          Stream su;
          su.open(ENT_BUNIF | (uint32_t)b, l.eval_id, rep, p.seed_lo, p.seed_hi);
          int prev = a, sprev = a;
          double tprev = 0.0, c = 0.0;
          for (int i = 1; i <= N; ++i) {
            c += neglog_u32(sr.draw_word((uint32_t)i), s_ltab);
            int di = e;
            if (i < N) {
              const double u = su.draw((uint32_t)(N + 1 + i));
              di = sm_draw<NS>(Bk + (size_t)(prev * n) * Kp, Kp, bt + ((size_t)(N - i) * nn + e) * Kp, (size_t)n * Kp, n, u, err);
            }
            if (prev != di) {
              const double ti = tb * (c / G);
              segment(sprev, ti - tprev);
              count(sprev, di);
              tprev = ti; sprev = di;
            }
            prev = di;
          }
          segment(sprev, tb - tprev);
        } else {
          segment(a, tb);
        }
      } else {
        segment(a, tb);                                              // mu = 0 or t = 0: the parent's state for the whole branch
      }
      if (valid) mr.end((size_t)b * p.map_pad + (size_t)(tl.row0 + lane));
    }
    st.flush();
  }
  if (err) atomicOr(p.err, err);
}

__global__ __launch_bounds__(256) void sm_finish_kernel(SmParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int n = p.ll.n, cols = n + n * (n - 1);
  const int64_t npad = (int64_t)p.n_tiles * 64;
  const int NT = p.ll.n_tips + p.n_node;
  if (gid < cols * npad) {
    const int c = (int)(gid / npad);
    const int64_t it = gid % npad;
    p.out[gid] = stat_cell_value(p.dwfx, p.cnt, n, c, (size_t)npad, (size_t)it, p.fx_inv);
    if (p.packed) {                                                  // the next iteration accumulates from zero
      if (c < n) p.dwfx[(size_t)c * npad + it] = 0ull;
      else p.cnt[(size_t)(c - n) * npad + it] = 0u;
    }
  }
  if (p.packed) {                                                    // one download per iteration: the lanes' ll and the error word ride along
    if (gid < npad) p.out[(int64_t)cols * npad + gid] = p.ll.ll[p.tiles[gid >> 6].ev + (int)(gid & 63)];
    if (gid == 0) p.out[(int64_t)(cols + 1) * npad] = (double)*p.err;
  }
  if (p.nodes) {
    for (int64_t cell = gid; cell < npad * NT; cell += (int64_t)gridDim.x * blockDim.x) {
      const int64_t it = cell / NT;
      const int row = (int)(cell % NT);
      p.nodes[cell] = (int32_t)p.nstate[((size_t)(it >> 6) * NT + row) * 64 + (it & 63)] + 1;
    }
  }
}

}  // namespace

hipError_t launch_sm_table(const SmParams& p, hipStream_t stream) {
  if (p.ll.n < 2 || p.ll.n > LL_LANE_MAX || p.ll.Kp <= 0 || p.ll.Kp % 64 || p.depth < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sm_table_kernel, dim3((p.ll.Kp + SM_BLOCK - 1) / SM_BLOCK), dim3(SM_BLOCK), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_sm_sample(const SmParams& p, const std::vector<int32_t>& level_off, int branch_blocks, int maps_mode,
                            hipStream_t stream) {
  if (p.ll.n < 2 || p.ll.n > LL_LANE_MAX || p.n_tiles <= 0 || branch_blocks <= 0) return hipErrorInvalidValue;
  if (p.packed && (maps_mode != MAPS_OFF || !p.lane_id || p.nodes)) return hipErrorInvalidValue;
  constexpr int W = SM_BLOCK / 64;
  const dim3 root_grid((p.n_tiles + W - 1) / W);
  if (p.packed) hipLaunchKernelGGL(sm_root_kernel<true>, root_grid, dim3(SM_BLOCK), 0, stream, p);
  else hipLaunchKernelGGL(sm_root_kernel<false>, root_grid, dim3(SM_BLOCK), 0, stream, p);
  for (size_t l = 0; l + 1 < level_off.size(); ++l) {
    const int64_t cnt = level_off[l + 1] - level_off[l];
    if (cnt <= 0) continue;
    const dim3 grid((unsigned)((cnt * p.n_tiles + W - 1) / W));
    if (p.packed) hipLaunchKernelGGL(sm_node_kernel<true>, grid, dim3(SM_BLOCK), 0, stream, p, level_off[l], level_off[l + 1]);
    else hipLaunchKernelGGL(sm_node_kernel<false>, grid, dim3(SM_BLOCK), 0, stream, p, level_off[l], level_off[l + 1]);
  }
  // branches per wave-item: as many as still leave every SIMD a few waves
  const int group = (int)std::max<int64_t>(1, std::min<int64_t>(16, (int64_t)p.n_edge * p.n_tiles / 8192));
  with_producer_form(maps_mode, p.ll.n, [&](auto mode, auto ns) {      // the packed form has no maps (checked above)
    constexpr int NS = decltype(ns)::value, MODE = decltype(mode)::value;
    if (p.packed) hipLaunchKernelGGL((sm_branch_kernel<NS, MAPS_OFF, true>), dim3(branch_blocks), dim3(SM_BLOCK), 0, stream, p, group);
    else hipLaunchKernelGGL((sm_branch_kernel<NS, MODE, false>), dim3(branch_blocks), dim3(SM_BLOCK), 0, stream, p, group);
  });
  const int n = p.ll.n;
  const int64_t cells = (int64_t)(n + n * (n - 1)) * p.n_tiles * 64;
  hipLaunchKernelGGL(sm_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace phm
