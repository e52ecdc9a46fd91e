// phm_loglik.hip -- log p(tips_s | Q_k, pid_k) for many rate matrices at once: section 13's up pass with the
// MODELS across the lanes.  A lane owns one model k: the tree records and branch lengths it reads are wave-uniform scalar loads,
// every load of Q, P and L is a coalesced row of the model-fastest buffers (phm_loglik.h).
//
// P_k(t_b) = expm(Q_k t_b) is computed once per (model, branch) and stored ([edge][n * n][model]): cross mode reuses it for every
// site.  The arithmetic is expm_pade_kernel's (phm_exp.hip): Pade(6) of (Q t) / 2^s, left-to-right products, partial pivoting,
// s squarings, with s from phm_ex::ex_squarings' rule evaluated by the lane itself (the largest row sum of |q_ij t| halved until
// <= 1/2: exact in IEEE arithmetic, so it is the host's count).
//   n <= 4: the five Pade matrices of a lane in registers, n a template parameter, every loop unrolled; the pivot row is exchanged
//           by selects over the unrolled rows, so no private array is indexed at run time and nothing spills.
//   5 .. 8: the same steps with the matrices in global memory, [matrix][entry][model], coalesced like everything else.
// 9 .. 64 states are not batched: phm_loglik_api.cpp loops the models through section 13's own launches.
//
// Tips, up and root are ex_tips_kernel / ex_up_kernel / ex_root_kernel with P per lane; an evaluation of probability 0 (or of a
// model one of whose P met a zero pivot) gets -inf and nothing fails.
#include "phm_loglik.h"

#include <algorithm>

#include "phm_ll_device.h"

namespace phm {

namespace {

constexpr int LL_BLOCK = 256;

// squarings of expm(Q t): phm_ex::ex_squarings on this lane's Q (stride st between entries)
__device__ __forceinline__ int ll_squarings(const double* __restrict__ q, size_t st, int n, double t) {
  double norm = 0.0;
  for (int i = 0; i < n; ++i) {
    double r = 0.0;
    for (int j = 0; j < n; ++j) r += fabs(q[(size_t)(i * n + j) * st] * t);
    norm = fmax(norm, r);
  }
  int s = 0;
  while (norm > 0.5 && s < 1000) { norm *= 0.5; ++s; }
  return s;
}

// C = A B, each sum left to right from its first product (block_gemm of phm_exp.hip)
template <int N>
__device__ __forceinline__ void ll_gemm(const double (&A)[N * N], const double (&B)[N * N], double (&C)[N * N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double acc = A[i * N] * B[j];
#pragma unroll
      for (int k = 1; k < N; ++k) acc += A[i * N + k] * B[k * N + j];
      C[i * N + j] = acc;
    }
}

// X = expm(q t) in registers; false on a zero pivot
template <int N>
__device__ __forceinline__ bool ll_expm_reg(const double (&q)[N * N], double tb, double (&X)[N * N]) {
  constexpr int NN = N * N;
  double norm = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) r += fabs(q[i * N + j] * tb);
    norm = fmax(norm, r);
  }
  int s = 0;
  while (norm > 0.5 && s < 1000) { norm *= 0.5; ++s; }
  const double sc = ldexp(1.0, s);
  double A[NN], Em[NN], Dm[NN], T2[NN];
  double c = 0.5;
#pragma unroll
  for (int e = 0; e < NN; ++e) {
    const double a = (q[e] * tb) / sc;
    A[e] = a; X[e] = a;
    const double ca = c * a;
    const bool diag = e / N == e % N;
    Em[e] = diag ? ca + 1.0 : ca;
    Dm[e] = diag ? -ca + 1.0 : -ca;
  }
#pragma unroll
  for (int i = 2; i <= 6; ++i) {
    c = c * (double)(6 - i + 1) / (double)(i * (2 * 6 - i + 1));
    ll_gemm<N>(A, X, T2);
#pragma unroll
    for (int e = 0; e < NN; ++e) {
      const double x = T2[e];
      X[e] = x;
      Em[e] += c * x;
      if (i % 2 == 0) Dm[e] += c * x; else Dm[e] -= c * x;
    }
  }
  bool ok = true;
#pragma unroll
  for (int col = 0; col < N; ++col) {
    int piv = col;
    double best = fabs(Dm[col * N + col]);
#pragma unroll
    for (int r = col + 1; r < N; ++r) {
      const double v = fabs(Dm[r * N + col]);
      if (v > best) { best = v; piv = r; }
    }
    if (!(best > 0.0)) ok = false;
#pragma unroll
    for (int r = col + 1; r < N; ++r) {                 // rows col and piv exchanged: a select per entry, no runtime row index
      const bool sw = piv == r;
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const double d0 = Dm[col * N + k], d1 = Dm[r * N + k], e0 = Em[col * N + k], e1 = Em[r * N + k];
        Dm[col * N + k] = sw ? d1 : d0; Dm[r * N + k] = sw ? d0 : d1;
        Em[col * N + k] = sw ? e1 : e0; Em[r * N + k] = sw ? e0 : e1;
      }
    }
#pragma unroll
    for (int r = col + 1; r < N; ++r) {
      const double f = Dm[r * N + col] / Dm[col * N + col];
#pragma unroll
      for (int k = 0; k < N; ++k) {
        if (k >= col) Dm[r * N + k] -= f * Dm[col * N + k];
        Em[r * N + k] -= f * Em[col * N + k];
      }
    }
  }
#pragma unroll
  for (int r = N - 1; r >= 0; --r)
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double acc = Em[r * N + k];
#pragma unroll
      for (int j = r + 1; j < N; ++j) acc -= Dm[r * N + j] * X[j * N + k];
      X[r * N + k] = acc / Dm[r * N + r];
    }
  for (int i = 0; i < s; ++i) {
    ll_gemm<N>(X, X, T2);
#pragma unroll
    for (int e = 0; e < NN; ++e) X[e] = T2[e];
  }
  return ok;
}

template <int N>
__global__ __launch_bounds__(LL_BLOCK) void ll_expm_reg_kernel(LlParams p, int e0) {
  const auto [k, Kp, Ev, ev, idle] = ll_lane<LL_BLOCK>(p);
  if (idle) return;
  const int b = e0 + blockIdx.y;
  double q[N * N], X[N * N];
#pragma unroll
  for (int e = 0; e < N * N; ++e) q[e] = p.Q[(size_t)e * Kp + k];
  const bool ok = ll_expm_reg<N>(q, p.t[b], X);
  double* out = p.P + (size_t)b * N * N * Kp + k;
#pragma unroll
  for (int e = 0; e < N * N; ++e) out[(size_t)e * Kp] = X[e];
  if (!ok) p.bad[k] = 1u;
}

// C = A B on this lane's matrices in global memory (stride st between entries)
__device__ __forceinline__ void ll_gemm_ws(const double* A, const double* B, double* C, int n, size_t st) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double acc = A[(size_t)(i * n) * st] * B[(size_t)j * st];
      for (int k = 1; k < n; ++k) acc += A[(size_t)(i * n + k) * st] * B[(size_t)(k * n + j) * st];
      C[(size_t)(i * n + j) * st] = acc;
    }
}

// 5..8 states: the same steps as ll_expm_reg on [matrix][entry][model] rows of `work`; X is the lane's column of P itself
__global__ __launch_bounds__(LL_BLOCK) void ll_expm_ws_kernel(LlParams p, int e0) {
  const auto [k, st, Ev, ev, idle] = ll_lane<LL_BLOCK>(p);
  if (idle) return;
  const int n = p.n, nn = n * n;
  const int b = e0 + blockIdx.y;
  const double* __restrict__ q = p.Q + k;
  double* A = p.work + (size_t)blockIdx.y * 4 * nn * st + k;
  double *Em = A + (size_t)nn * st, *Dm = A + (size_t)2 * nn * st, *T2 = A + (size_t)3 * nn * st;
  double* X = p.P + (size_t)b * nn * st + k;
  const double tb = p.t[b];
  const int s = ll_squarings(q, st, n, tb);
  const double sc = ldexp(1.0, s);
  double c = 0.5;
  for (int e = 0; e < nn; ++e) {
    const double a = (q[(size_t)e * st] * tb) / sc;
    A[(size_t)e * st] = a; X[(size_t)e * st] = a;
    const double ca = c * a;
    const bool diag = e / n == e % n;
    Em[(size_t)e * st] = diag ? ca + 1.0 : ca;
    Dm[(size_t)e * st] = diag ? -ca + 1.0 : -ca;
  }
  bool positive = true;
  for (int i = 2; i <= 6; ++i) {
    c = c * (double)(6 - i + 1) / (double)(i * (2 * 6 - i + 1));
    ll_gemm_ws(A, X, T2, n, st);
    for (int e = 0; e < nn; ++e) {
      const double x = T2[(size_t)e * st];
      X[(size_t)e * st] = x;
      Em[(size_t)e * st] += c * x;
      if (positive) Dm[(size_t)e * st] += c * x; else Dm[(size_t)e * st] -= c * x;
    }
    positive = !positive;
  }
  bool ok = true;
  for (int col = 0; col < n; ++col) {
    int piv = col;
    double best = fabs(Dm[(size_t)(col * n + col) * st]);
    for (int r = col + 1; r < n; ++r) {
      const double v = fabs(Dm[(size_t)(r * n + col) * st]);
      if (v > best) { best = v; piv = r; }
    }
    if (!(best > 0.0)) ok = false;
    if (piv != col)
      for (int j = 0; j < n; ++j) {
        const size_t x0 = (size_t)(col * n + j) * st, x1 = (size_t)(piv * n + j) * st;
        double a = Dm[x0]; Dm[x0] = Dm[x1]; Dm[x1] = a;
        a = Em[x0]; Em[x0] = Em[x1]; Em[x1] = a;
      }
    const double d = Dm[(size_t)(col * n + col) * st];
    for (int r = col + 1; r < n; ++r) {
      const double f = Dm[(size_t)(r * n + col) * st] / d;
      for (int j = 0; j < n; ++j) {
        if (j >= col) Dm[(size_t)(r * n + j) * st] -= f * Dm[(size_t)(col * n + j) * st];
        Em[(size_t)(r * n + j) * st] -= f * Em[(size_t)(col * n + j) * st];
      }
    }
  }
  for (int r = n - 1; r >= 0; --r)
    for (int j = 0; j < n; ++j) {
      double acc = Em[(size_t)(r * n + j) * st];
      for (int m = r + 1; m < n; ++m) acc -= Dm[(size_t)(r * n + m) * st] * X[(size_t)(m * n + j) * st];
      X[(size_t)(r * n + j) * st] = acc / Dm[(size_t)(r * n + r) * st];
    }
  for (int i = 0; i < s; ++i) {
    ll_gemm_ws(X, X, T2, n, st);
    for (int e = 0; e < nn; ++e) X[(size_t)e * st] = T2[(size_t)e * st];
  }
  if (!ok) p.bad[k] = 1u;
}

__global__ __launch_bounds__(LL_BLOCK) void ll_tips_kernel(LlParams p, int t0) {
  const auto [k, Kp, Ev, ev, idle] = ll_lane<LL_BLOCK>(p);
  if (idle) return;
  const int t = t0 + blockIdx.y, site = blockIdx.z;
  const int y = p.paired ? p.tips[(size_t)t * Kp + k] : p.tips[(size_t)site * p.n_tips + t];
  for (int i = 0; i < p.n; ++i) p.L[((size_t)t * p.n + i) * Ev + ev] = (y == 0 || p.obs[i] == y) ? 1.0 : 0.0;
  p.sL[(size_t)t * Ev + ev] = 0.0;
}

template <int N>
__global__ __launch_bounds__(LL_BLOCK) void ll_up_kernel(LlParams p, const UpStep* __restrict__ steps, int k0) {
  const auto [k, Kp, Ev, ev, idle] = ll_lane<LL_BLOCK>(p);
  if (idle) return;
  const UpStep u = steps[k0 + blockIdx.y];
  const int r0 = u.child[0] >= 0 ? p.n_tips + u.child[0] : ~u.child[0];
  const int r1 = u.child[1] >= 0 ? p.n_tips + u.child[1] : ~u.child[1];
  const int rp = p.n_tips + u.parent;
  const double* __restrict__ P0 = p.P + (size_t)u.edge[0] * N * N * Kp + k;
  const double* __restrict__ P1 = p.P + (size_t)u.edge[1] * N * N * Kp + k;
  double l0[N], l1[N], v[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    l0[j] = p.L[((size_t)r0 * N + j) * Ev + ev];
    l1[j] = p.L[((size_t)r1 * N + j) * Ev + ev];
  }
  double mx = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      a = fma(P0[(size_t)(i * N + j) * Kp], l0[j], a);
      b = fma(P1[(size_t)(i * N + j) * Kp], l1[j], b);
    }
    v[i] = a * b;
    mx = fmax(mx, v[i]);
  }
  int e = 0;                                                       // ll_rescale's rule, fused with the store: with its call form a
  if (mx > 0.0) (void)frexp(mx, &e);                               // call at 8 states timed 1.3 to 3 % slower (docs/MEASUREMENTS.md)
#pragma unroll
  for (int i = 0; i < N; ++i) p.L[((size_t)rp * N + i) * Ev + ev] = mx > 0.0 ? ldexp(v[i], -e) : v[i];
  p.sL[(size_t)rp * Ev + ev] = p.sL[(size_t)r0 * Ev + ev] + p.sL[(size_t)r1 * Ev + ev] + e;
}

__global__ __launch_bounds__(LL_BLOCK) void ll_root_kernel(LlParams p, int root) {
  const auto [k, Kp, Ev, ev, idle] = ll_lane<LL_BLOCK>(p);
  if (idle) return;
  double l = 0.0;
  for (int i = 0; i < p.n; ++i) l = fma(p.pid[(size_t)i * Kp + k], p.L[((size_t)root * p.n + i) * Ev + ev], l);
  const double v = log(l) + p.sL[(size_t)root * Ev + ev] * LN2;
  p.ll[ev] = (p.bad[k] || !(l > 0.0)) ? -INFINITY : v;
}

}  // namespace

hipError_t launch_ll_expm(const LlParams& p, int e0, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (count > LL_GRID_Y || p.Kp % 64 != 0 || !ll_states_ok(p)) return hipErrorInvalidValue;
  const dim3 g = model_grid(p, LL_BLOCK, count, 1), blk(LL_BLOCK);
  switch (p.n) {
    case 2: hipLaunchKernelGGL((ll_expm_reg_kernel<2>), g, blk, 0, stream, p, e0); break;
    case 3: hipLaunchKernelGGL((ll_expm_reg_kernel<3>), g, blk, 0, stream, p, e0); break;
    case 4: hipLaunchKernelGGL((ll_expm_reg_kernel<4>), g, blk, 0, stream, p, e0); break;
    default:
      if (!p.work) return hipErrorInvalidValue;
      hipLaunchKernelGGL(ll_expm_ws_kernel, g, blk, 0, stream, p, e0);
  }
  return hipGetLastError();
}

hipError_t launch_ll_tips(const LlParams& p, hipStream_t stream) {
  if (!ll_sites_ok(p)) return hipErrorInvalidValue;
  for (int t0 = 0; t0 < p.n_tips; t0 += LL_GRID_Y)
    hipLaunchKernelGGL(ll_tips_kernel, model_grid(p, LL_BLOCK, std::min(LL_GRID_Y, p.n_tips - t0), p.n_sites), dim3(LL_BLOCK), 0, stream, p, t0);
  return hipGetLastError();
}

hipError_t launch_ll_up(const LlParams& p, const UpStep* steps, int count, hipStream_t stream) {
  if (!ll_sites_ok(p) || !ll_states_ok(p)) return hipErrorInvalidValue;
  for (int k0 = 0; k0 < count; k0 += LL_GRID_Y) {
    const dim3 g = model_grid(p, LL_BLOCK, std::min(LL_GRID_Y, count - k0), p.n_sites);
    ll_with_states(p.n, [&](auto ns) { hipLaunchKernelGGL((ll_up_kernel<decltype(ns)::value>), g, dim3(LL_BLOCK), 0, stream, p, steps, k0); });
  }
  return hipGetLastError();
}

hipError_t launch_ll_root(const LlParams& p, int root_row, hipStream_t stream) {
  if (!ll_sites_ok(p)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ll_root_kernel, model_grid(p, LL_BLOCK, 1, p.n_sites), dim3(LL_BLOCK), 0, stream, p, root_row);
  return hipGetLastError();
}

}  // namespace phm
