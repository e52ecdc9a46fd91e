// phm_scores.hip -- E[dwell_i | tips_s, Q_k] and E[N_ij | tips_s, Q_k] for many rate matrices at once:
// section 13's down pass and branch stage with the MODELS across the lanes, on top of section 17's P_k(t_b) and up pass
// (phm_loglik.hip, launched unchanged: log p(tips | Q_k) is that entry point's value bit for bit).
//
// A lane owns one model k.  The tree records and branch lengths it reads are wave-uniform scalar loads; Q, B, P, L, O and F are
// coalesced rows of the model-fastest buffers (phm_scores.h).  What section 13 prepares on the host per call -- mu, B = I + Q / mu
// and the Poisson weights of every branch -- exists here once per (model, branch), so the lane forms it:
//
//   r_0 = x = mu_k t_b,  r_{m+1} = r_m x / (m + 2)      (r_m = x^(m+1) / (m+1)!: Poisson(m + 1; x) up to the factor e^-x)
//   I = sum_m r_m A_m  and  S = 1 + sum_m r_m  side by side; whenever r passes 2^512, r, S and I are divided by 2^512
//   (what flushes then is below 2^-512 of the peak); the sum ends at the first m past the mode whose geometric tail bound
//   r_{m+1} / (1 - x / (m + 3)) is at most 2^-60 S; at the end I is divided by S mu.
//
// No lgamma, no e^-x, and the weights are normalised by their own sum.  A_0 = u_0 v_0^T, A_{m+1} = B^T A_m + u_0 v_{m+1}^T,
// v_{m+1} = B v_m is ex_branch_lane_kernel's recursion.  mu_k = 0 (P = I): I = t_b u_0 v_0^T.
//
// The sum over the branches is taken here, in a fixed order: a lane adds the SC_RUN consecutive edge rows of its run in edge
// order, and sc_total_kernel adds the run totals in run order.  SC_RUN is a compile-time constant, so no chunking and no device
// count changes a bit.  n <= 4: A, I, B, u_0, v and the run total in registers.  5..8 states: B from global memory (coalesced,
// cache-resident), the run total accumulated in its own output row.
#include "phm_scores.h"

#include <algorithm>

#include "phm_ll_device.h"

namespace phm {

namespace {

constexpr int SC_BLOCK = 256;                  // passes
constexpr int SC_BRANCH_BLOCK = 64;            // branch stage: one wave per block (register-heavy, and K is often small)

__global__ __launch_bounds__(SC_BLOCK) void sc_model_kernel(ScParams p) {
  const LlParams& q = p.ll;
  const int k = blockIdx.x * SC_BLOCK + threadIdx.x;
  if (k >= q.Kp) return;
  const int n = q.n;
  const size_t Kp = q.Kp;
  const double mu = model_mu(q.Q + k, Kp, n);
  p.mu[k] = mu;
  if (!p.B) return;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) p.B[(size_t)(i * n + j) * Kp + k] = model_b(q.Q[(size_t)(i * n + j) * Kp + k], mu, i == j ? 1.0 : 0.0);
}

__global__ __launch_bounds__(SC_BLOCK) void sc_root_kernel(ScParams p) {
  const LlParams& q = p.ll;
  const auto [k, Kp, Ev, ev, idle] = ll_lane<SC_BLOCK>(q);
  if (idle) return;
  double l = 0.0;
  for (int i = 0; i < q.n; ++i) {
    const double pi = q.pid[(size_t)i * Kp + k];
    l = fma(pi, q.L[((size_t)p.root * q.n + i) * Ev + ev], l);
    p.O[((size_t)p.root * q.n + i) * Ev + ev] = pi;
  }
  p.sO[(size_t)p.root * Ev + ev] = 0.0;
  p.lam[ev] = l;
}

// ex_down_kernel with P per lane
template <int N>
__global__ __launch_bounds__(SC_BLOCK) void sc_down_kernel(ScParams p, const ExDown* __restrict__ steps, int k0) {
  const LlParams& q = p.ll;
  const auto [k, Kp, Ev, ev, idle] = ll_lane<SC_BLOCK>(q);
  if (idle) return;
  const ExDown d = steps[k0 + blockIdx.y];
  const double* __restrict__ Ps = q.P + (size_t)d.sib_edge * N * N * Kp + k;
  const double* __restrict__ Pb = q.P + (size_t)d.edge * N * N * Kp + k;
  double ls[N], f[N], o[N];
#pragma unroll
  for (int j = 0; j < N; ++j) ls[j] = q.L[((size_t)d.sib_child * N + j) * Ev + ev];
  double mx = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {                                    // F_b = O_p (.) P(t_sib) L_sib
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) a = fma(Ps[(size_t)(i * N + j) * Kp], ls[j], a);
    f[i] = p.O[((size_t)d.parent * N + i) * Ev + ev] * a;
    mx = fmax(mx, f[i]);
  }
  const double sF = p.sO[(size_t)d.parent * Ev + ev] + q.sL[(size_t)d.sib_child * Ev + ev] + ll_rescale<N>(f, mx);
  p.sF[(size_t)d.edge * Ev + ev] = sF;
  mx = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {                                    // O_c = P(t_b)^T F_b
    p.F[((size_t)d.edge * N + i) * Ev + ev] = f[i];
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) a = fma(Pb[(size_t)(j * N + i) * Kp], f[j], a);
    o[i] = a;
    mx = fmax(mx, a);
  }
  p.sO[(size_t)d.child * Ev + ev] = sF + ll_rescale<N>(o, mx);
#pragma unroll
  for (int i = 0; i < N; ++i) p.O[((size_t)d.child * N + i) * Ev + ev] = o[i];
}

template <int N>
__global__ __launch_bounds__(SC_BRANCH_BLOCK) void sc_branch_kernel(ScParams p, int r0) {
  constexpr bool REG = N <= LL_REG_MAX;
  constexpr int NN = N * N;
  const LlParams& q = p.ll;
  const int k = blockIdx.x * SC_BRANCH_BLOCK + threadIdx.x;
  if (k >= q.Kc) return;
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp, ev = (size_t)blockIdx.z * Kp + k;
  const int run = r0 + blockIdx.y;
  const int b_begin = run * SC_RUN, b_end = min(p.n_edge, b_begin + SC_RUN);
  const double mu = p.mu[k];
  const bool still = !(mu > 0.0);                                  // the model leaves no state: P = I
  const double* __restrict__ Qk = q.Q + k;
  const double* __restrict__ Bg = REG ? nullptr : p.B + k;
  double Breg[REG ? NN : 1];
  if constexpr (REG) {
#pragma unroll
    for (int e = 0; e < NN; ++e) {                                 // model_b's cell, in this kernel's own spelling (its code is pinned)
      const double d = e / N == e % N ? 1.0 : 0.0;
      Breg[e] = still ? d : d + Qk[(size_t)e * Kp] / mu;
    }
  }
  auto Bat = [&](int e) -> double {
    if constexpr (REG) return Breg[e]; else return Bg[(size_t)e * Kp];
  };
  const double lam = p.lam[ev], e_root = q.sL[(size_t)p.root * Ev + ev];
  double* out = p.runs + (size_t)blockIdx.y * NN * Ev + ev;        // [col][Ev] of this run
  double tot[REG ? NN : 1];
  if constexpr (REG) {
#pragma unroll
    for (int e = 0; e < NN; ++e) tot[e] = 0.0;
  }
  for (int b = b_begin; b < b_end; ++b) {
    const double t = q.t[b];
    const int c = p.child[b];
    double u0[N], v[N], A[N][N], I[N][N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      u0[i] = p.F[((size_t)b * N + i) * Ev + ev];
      v[i] = q.L[((size_t)c * N + i) * Ev + ev];
    }
    const double x = still ? 0.0 : mu * t;
    double r = still ? t : x;                                      // mu = 0: the one weight t_b, the sum 1 and no division by mu
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
    const double f = ldexp(1.0 / lam, (int)(p.sF[(size_t)b * Ev + ev] + q.sL[(size_t)c * Ev + ev] - e_root));
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int col = i == j ? i : count_col(N, i, j);
        const double val = i == j ? (I[i][i] * inv) * f : (Qk[(size_t)(i * N + j) * Kp] * (I[i][j] * inv)) * f;
        if constexpr (REG) {
          tot[col] += val;
        } else {
          double* o = out + (size_t)col * Ev;
          *o = b == b_begin ? 0.0 + val : *o + val;
        }
      }
  }
  if constexpr (REG) {
#pragma unroll
    for (int e = 0; e < NN; ++e) out[(size_t)e * Ev] = tot[e];
  }
}

__global__ __launch_bounds__(SC_BLOCK) void sc_total_kernel(ScParams p, int count) {
  const LlParams& q = p.ll;
  const auto [k, Kp, Ev, ev, idle] = ll_lane<SC_BLOCK>(q);
  if (idle) return;
  const int cols = q.n * q.n, col = blockIdx.y;
  double acc = p.tot[(size_t)col * Ev + ev];
  for (int r = 0; r < count; ++r) acc += p.runs[((size_t)r * cols + col) * Ev + ev];
  p.tot[(size_t)col * Ev + ev] = acc;
}

inline bool sc_ok(const ScParams& p) { return ll_ok(p.ll); }

}  // namespace

hipError_t launch_sc_model(const ScParams& p, hipStream_t stream) {
  if (!sc_ok(p) || (p.ll.n > LL_REG_MAX && !p.B)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sc_model_kernel, model_grid(p.ll, SC_BLOCK, 1, 1), dim3(SC_BLOCK), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_sc_root(const ScParams& p, hipStream_t stream) {
  if (!sc_ok(p)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sc_root_kernel, model_grid(p.ll, SC_BLOCK, 1, p.ll.n_sites), dim3(SC_BLOCK), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_sc_down(const ScParams& p, const ExDown* steps, int count, hipStream_t stream) {
  if (!sc_ok(p)) return hipErrorInvalidValue;
  for (int k0 = 0; k0 < count; k0 += LL_GRID_Y) {
    const dim3 g = model_grid(p.ll, SC_BLOCK, std::min(LL_GRID_Y, count - k0), p.ll.n_sites);
    ll_with_states(p.ll.n, [&](auto ns) { hipLaunchKernelGGL((sc_down_kernel<decltype(ns)::value>), g, dim3(SC_BLOCK), 0, stream, p, steps, k0); });
  }
  return hipGetLastError();
}

hipError_t launch_sc_branch(const ScParams& p, int r0, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  const int n_runs = (p.n_edge + SC_RUN - 1) / SC_RUN;
  if (!sc_ok(p) || count > LL_GRID_Y || r0 < 0 || r0 + count > n_runs || (p.ll.n > LL_REG_MAX && !p.B)) return hipErrorInvalidValue;
  const dim3 g = model_grid(p.ll, SC_BRANCH_BLOCK, count, p.ll.n_sites);
  ll_with_states(p.ll.n, [&](auto ns) { hipLaunchKernelGGL((sc_branch_kernel<decltype(ns)::value>), g, dim3(SC_BRANCH_BLOCK), 0, stream, p, r0); });
  return hipGetLastError();
}

hipError_t launch_sc_total(const ScParams& p, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!sc_ok(p)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sc_total_kernel, model_grid(p.ll, SC_BLOCK, p.ll.n * p.ll.n, p.ll.n_sites), dim3(SC_BLOCK), 0, stream, p, count);
  return hipGetLastError();
}

}  // namespace phm
