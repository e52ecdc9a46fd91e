// phm_time_models.hip -- the exact expectations through time for many rate matrices at 2..8 states:
// section 16's along-branch vectors, sub-branch integrals and fixed-order sums with the MODELS across the lanes, on top of section
// 17's P_k(t_b) and up pass and section 18's root and down pass, all launched unchanged.
//
// A lane owns one model k, as in phm_scores.hip and phm_branch_rows.hip; an item (a point pair on a branch, TmItem) is uniform over
// the wave, so its record, the branch length and the child row are scalar loads, and F, L, a, beta and the rows are coalesced
// along the models.
//
// tm_along_kernel: a = P_k(t1)^T F_b and beta = P_k(t2) L_c by uniformization with the lane's own B_k = I + Q_k / mu_k, which the
// branch stage needs anyway: no n x n matrix per (model, item) is formed or stored.  With x = mu_k t,
//   P(t) v = sum_m w_m B^m v / sum_m w_m,   w_0 = 1,  w_{m+1} = w_m x / (m + 1)     (Poisson(m; x) up to the factor e^-x)
// so there is no e^-x and no lgamma; whenever w passes 2^512, w, the sum and the accumulator are divided by 2^512, and the sum
// ends at the first m past the mode whose geometric tail bound w_{m+1} / (1 - x / (m + 2)) is at most 2^-60 of the sum.  B is
// non-negative, so every term is: nothing cancels.  The ends of a branch take no sum: t = 0 returns the vector unchanged, and
// t = t_b multiplies by the stored P_k(t_b) in the passes' own order (a as sc_down_kernel's O_c, beta as the up pass's P L), so a
// point at a node repeats the node's sums.  mu_k = 0 gives x = 0 and the vector unchanged at every t.
//
// tm_branch_kernel: br_branch_kernel's body (sc_branch_kernel's, operation for operation) on a sub-branch: (F_b, L_c, t_b) are
// (a(s1), beta(s2), h) with the factor 2^(e_a + e_beta - e_root) / lam.  RESTATED here for section 27's reason: those kernels'
// code stays as it is.  n <= 4: A, I, B, u_0 and v in registers.  5..8 states: B from global memory.
//
// tm_range_sum_kernel: lane (evaluation, column, range) adds its range's items in item order, continued across launches.
// Every loop is bounded by n, SC_M_CAP or the item / column count; no atomics.
#include "phm_time_models.h"

#include <algorithm>

#include "phm_ll_device.h"

namespace phm {

namespace {

constexpr int TM_BLOCK = 64;                   // along and branch stages: one wave per block, as SC_BRANCH_BLOCK
constexpr int TM_SUM_BLOCK = 256;

// v <- P(t) v (TR false) or P(t)^T v (TR true) for x = mu t by uniformization; Bat(e): entry e of the lane's row-major B
template <int N, bool TR, class BAT>
__device__ __forceinline__ void tm_apply(BAT&& Bat, double x, double (&v)[N]) {
  double acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = v[i];
  double w = 1.0, S = 1.0;
  for (int m = 0; m < SC_M_CAP; ++m) {
    const double wn = w * (x / (double)(m + 1));
    // past the mode (x < m + 1) the terms fall at least geometrically: sum_{j > m} w_j <= w_{m+1} / (1 - x / (m + 2))
    if (x < (double)(m + 1) && wn <= 0x1p-60 * S * (1.0 - x / (double)(m + 2))) break;
    double nv[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) s = fma(Bat(TR ? j * N + i : i * N + j), v[j], s);
      nv[i] = s;
    }
    w = wn;
    S += w;
#pragma unroll
    for (int i = 0; i < N; ++i) { acc[i] = fma(w, nv[i], acc[i]); v[i] = nv[i]; }
    if (w > 0x1p512) {
      w *= 0x1p-512;
      S *= 0x1p-512;
#pragma unroll
      for (int i = 0; i < N; ++i) acc[i] *= 0x1p-512;
    }
  }
  const double inv = 1.0 / S;
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = acc[i] * inv;
}

// grid: (models / 64, items of the launch, sites)
template <int N>
__global__ __launch_bounds__(TM_BLOCK) void tm_along_kernel(TmParams p) {
  constexpr bool REG = N <= LL_REG_MAX;
  constexpr int NN = N * N;
  const LlParams& q = p.sc.ll;
  const int k = blockIdx.x * TM_BLOCK + threadIdx.x;
  if (k >= q.Kc) return;
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp, ev = (size_t)blockIdx.z * Kp + k;
  const size_t Eo = (size_t)q.n_sites * q.Kc, eo = (size_t)blockIdx.z * q.Kc + k;
  const TmItem it = p.items[blockIdx.y];                           // uniform over the wave
  const int b = it.edge, c = p.sc.child[b];
  const double tb = q.t[b];
  const double mu = p.sc.mu[k];
  const bool still = !(mu > 0.0);                                  // the model leaves no state: P = I
  const double* __restrict__ Qk = q.Q + k;
  const double* __restrict__ Bg = REG ? nullptr : p.sc.B + k;
  const double* __restrict__ Pb = q.P + (size_t)b * NN * Kp + k;   // P_k(t_b), row-major entries
  double Breg[REG ? NN : 1];
  if constexpr (REG) {
#pragma unroll
    for (int e = 0; e < NN; ++e) Breg[e] = model_b(Qk[(size_t)e * Kp], mu, e / N == e % N ? 1.0 : 0.0);
  }
  auto Bat = [&](int e) -> double {
    if constexpr (REG) return Breg[e]; else return Bg[(size_t)e * Kp];
  };
  const bool posterior = p.post != nullptr;
  double* __restrict__ out = posterior ? p.post + (size_t)blockIdx.y * N * Eo + eo : nullptr;   // [state][Eo] of this item

  double v[N];
  // beta = P(t2) L_c
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = q.L[((size_t)c * N + i) * Ev + ev];
  if (it.t2 == tb && tb != 0.0) {                                  // the parent end: the up pass's P L
    double nv[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) s = fma(Pb[(size_t)(i * N + j) * Kp], v[j], s);
      nv[i] = s;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = nv[i];
  } else if (it.t2 != 0.0) {
    tm_apply<N, false>(Bat, still ? 0.0 : mu * it.t2, v);
  }
  if (posterior) {                                                 // beta, parked in the output
#pragma unroll
    for (int i = 0; i < N; ++i) out[(size_t)i * Eo] = v[i];
  } else {
    double mx = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) mx = fmax(mx, v[i]);
    const int e = ll_rescale<N>(v, mx);
    double* be = p.beta + (size_t)blockIdx.y * N * Eo + eo;
#pragma unroll
    for (int i = 0; i < N; ++i) be[(size_t)i * Eo] = v[i];
    p.sbeta[(size_t)blockIdx.y * Eo + eo] = q.sL[(size_t)c * Ev + ev] + (double)e;
  }

  // a = P(t1)^T F_b
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = p.sc.F[((size_t)b * N + i) * Ev + ev];
  if (it.t1 == tb && tb != 0.0) {                                  // the child end: sc_down_kernel's O_c = P(t_b)^T F_b
    double nv[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) s = fma(Pb[(size_t)(j * N + i) * Kp], v[j], s);
      nv[i] = s;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = nv[i];
  } else if (it.t1 != 0.0) {
    tm_apply<N, true>(Bat, still ? 0.0 : mu * it.t1, v);
  }
  if (posterior) {                                                 // ex_along_kernel's order on (a, beta)
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double be = out[(size_t)i * Eo];
      sum = fma(v[i], be, sum);
      v[i] = v[i] * be;
    }
    const double inv = 1.0 / sum;
#pragma unroll
    for (int i = 0; i < N; ++i) out[(size_t)i * Eo] = v[i] * inv;
    return;
  }
  double mx = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) mx = fmax(mx, v[i]);
  const int e = ll_rescale<N>(v, mx);
  double* a = p.a + (size_t)blockIdx.y * N * Eo + eo;
#pragma unroll
  for (int i = 0; i < N; ++i) a[(size_t)i * Eo] = v[i];
  p.sa[(size_t)blockIdx.y * Eo + eo] = p.sc.sF[(size_t)b * Ev + ev] + (double)e;
}

// grid: (models / 64, sub-branches of the launch, sites)
template <int N>
__global__ __launch_bounds__(TM_BLOCK) void tm_branch_kernel(TmParams p) {
  constexpr bool REG = N <= LL_REG_MAX;
  constexpr int NN = N * N;
  const LlParams& q = p.sc.ll;
  const int k = blockIdx.x * TM_BLOCK + threadIdx.x;
  if (k >= q.Kc) return;
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp, ev = (size_t)blockIdx.z * Kp + k;
  const size_t Eo = (size_t)q.n_sites * q.Kc, eo = (size_t)blockIdx.z * q.Kc + k;
  const double mu = p.sc.mu[k];
  const bool still = !(mu > 0.0);                                  // the model leaves no state: P = I
  const double* __restrict__ Qk = q.Q + k;
  const double* __restrict__ Bg = REG ? nullptr : p.sc.B + k;
  double Breg[REG ? NN : 1];
  if constexpr (REG) {
#pragma unroll
    for (int e = 0; e < NN; ++e) {
      const double d = e / N == e % N ? 1.0 : 0.0;
      Breg[e] = still ? d : d + Qk[(size_t)e * Kp] / mu;
    }
  }
  auto Bat = [&](int e) -> double {
    if constexpr (REG) return Breg[e]; else return Bg[(size_t)e * Kp];
  };
  const double lam = p.sc.lam[ev], e_root = q.sL[(size_t)p.sc.root * Ev + ev];
  double* out = p.rows + (size_t)blockIdx.y * NN * Eo + eo;        // [col][Eo] of this item
  const double t = p.items[blockIdx.y].h;                          // uniform over the wave
  const double* __restrict__ ai = p.a + (size_t)blockIdx.y * N * Eo + eo;
  const double* __restrict__ bi = p.beta + (size_t)blockIdx.y * N * Eo + eo;
  double u0[N], v[N], A[N][N], I[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    u0[i] = ai[(size_t)i * Eo];
    v[i] = bi[(size_t)i * Eo];
  }
  const double x = still ? 0.0 : mu * t;
  double r = still ? t : x;                                        // mu = 0: the one weight h, the sum 1 and no division by mu
  double S = still ? 1.0 : 1.0 + x;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) { A[i][j] = u0[i] * v[j]; I[i][j] = r * A[i][j]; }
  for (int m = 0; m < SC_M_CAP; ++m) {
    const double rn = r * (x / (double)(m + 2));
    // past the mode (x < m + 2) the terms fall at least geometrically: sum_{j > m} r_j <= r_{m+1} / (1 - x / (m + 3))
    if (x < (double)(m + 2) && rn <= 0x1p-60 * S * (1.0 - x / (double)(m + 3))) break;
    double nv[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) a = fma(Bat(i * N + j), v[j], a);
      nv[i] = a;
    }
    r = rn;
    S += r;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double tc[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        double a = u0[i] * nv[j];
#pragma unroll
        for (int kk = 0; kk < N; ++kk) a = fma(Bat(kk * N + i), A[kk][j], a);
        tc[i] = a;
      }
#pragma unroll
      for (int i = 0; i < N; ++i) { A[i][j] = tc[i]; I[i][j] = fma(r, tc[i], I[i][j]); }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = nv[i];
    if (r > 0x1p512) {
      r *= 0x1p-512;
      S *= 0x1p-512;
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) I[i][j] *= 0x1p-512;
    }
  }
  const double inv = 1.0 / (still ? S : S * mu);
  const double f = ldexp(1.0 / lam, (int)(p.sa[(size_t)blockIdx.y * Eo + eo] + p.sbeta[(size_t)blockIdx.y * Eo + eo] - e_root));
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int col = i == j ? i : count_col(N, i, j);
      out[(size_t)col * Eo] = i == j ? (I[i][i] * inv) * f : (Qk[(size_t)(i * N + j) * Kp] * (I[i][j] * inv)) * f;
    }
}

// grid: (evaluations / 256, columns, ranges of the launch).  A dependent chain over the range's items in order, continued from
// tot across launches, so the sum does not depend on how the items were chunked.
__global__ __launch_bounds__(TM_SUM_BLOCK) void tm_range_sum_kernel(const double* __restrict__ x, int cols, int count, int64_t q0,
                                                                    const int64_t* __restrict__ off, int r0, int n_ranges, int64_t Eo,
                                                                    double* __restrict__ tot) {
  const int64_t ev = (int64_t)blockIdx.x * TM_SUM_BLOCK + threadIdx.x;
  if (ev >= Eo) return;
  const int col = blockIdx.y, r = r0 + blockIdx.z;
  const int64_t lo = max(off[r], q0), hi = min(off[r + 1], q0 + (int64_t)count);
  if (lo >= hi) return;
  const double* xc = x + (int64_t)col * Eo + ev;
  double* t = tot + ((int64_t)col * n_ranges + r) * Eo + ev;
  double acc = *t;
  for (int64_t j = lo; j < hi; ++j) acc += xc[(j - q0) * cols * Eo];
  *t = acc;
}

inline bool tm_ok(const TmParams& p, int count) {
  return ll_ok(p.sc.ll) && count <= TM_GRID_MAX && p.items && (p.sc.ll.n <= LL_REG_MAX || p.sc.B);
}

}  // namespace

hipError_t launch_tm_along(const TmParams& p, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!tm_ok(p, count) || (!p.post && (!p.a || !p.sa || !p.beta || !p.sbeta))) return hipErrorInvalidValue;
  const dim3 g = model_grid(p.sc.ll, TM_BLOCK, count, p.sc.ll.n_sites);
  ll_with_states(p.sc.ll.n, [&](auto ns) { hipLaunchKernelGGL((tm_along_kernel<decltype(ns)::value>), g, dim3(TM_BLOCK), 0, stream, p); });
  return hipGetLastError();
}

hipError_t launch_tm_branch(const TmParams& p, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!tm_ok(p, count) || !p.a || !p.sa || !p.beta || !p.sbeta || !p.rows) return hipErrorInvalidValue;
  const dim3 g = model_grid(p.sc.ll, TM_BLOCK, count, p.sc.ll.n_sites);
  ll_with_states(p.sc.ll.n, [&](auto ns) { hipLaunchKernelGGL((tm_branch_kernel<decltype(ns)::value>), g, dim3(TM_BLOCK), 0, stream, p); });
  return hipGetLastError();
}

hipError_t launch_tm_range_sum(const double* x, int cols, int count, int64_t q0, const int64_t* off, int r_begin, int r_end,
                               int n_ranges, int64_t Eo, double* tot, hipStream_t stream) {
  if (count <= 0 || r_end <= r_begin) return hipSuccess;
  const int64_t gx = (Eo + TM_SUM_BLOCK - 1) / TM_SUM_BLOCK;
  if (!x || !off || !tot || cols < 1 || cols > LL_GRID_Y || Eo < 1 || gx > (int64_t)INT32_MAX || r_begin < 0 || r_end > n_ranges)
    return hipErrorInvalidValue;
  for (int r0 = r_begin; r0 < r_end; r0 += LL_GRID_Y)
    hipLaunchKernelGGL(tm_range_sum_kernel, dim3((unsigned)gx, cols, std::min(LL_GRID_Y, r_end - r0)), dim3(TM_SUM_BLOCK), 0, stream,
                       x, cols, count, q0, off, r0, n_ranges, Eo, tot);
  return hipGetLastError();
}

}  // namespace phm
