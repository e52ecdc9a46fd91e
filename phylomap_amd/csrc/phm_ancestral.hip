// phm_ancestral.hip -- ancestral states for many rate matrices at once: the joint reconstruction (the one
// assignment of ALL nodes that maximises p(states, tips | Q_k, pid_k); Pupko et al. 2000) by a max-product up pass with back
// pointers and a traceback, and the marginal node posteriors O (.) L, both on top of section 17's P_k(t_b) and section 18's down
// pass (phm_loglik.hip, phm_scores.hip, launched unchanged).
//
// A lane owns one model k.  The tree records are wave-uniform scalar loads; P, M, L, O and the pointer words are coalesced rows
// of the model-fastest buffers (phm_ancestral.h).  The arithmetic of the joint reconstruction is explicit, with no fused
// multiply-add (section 21 is its specification):
//   edge b (parent state a):  w(c) = P_k(t_b)[a, c] * M_child(c), one rounded product; m_b(a) = max_c w(c); ptr_b(a) = the
//                             smallest c that attains it (scan from 0, replace on strict >; all zero: ptr 0, m 0)
//   parent:                   M_p(a) = m_b0(a) * m_b1(a), rescaled by the power of two of its largest entry as ll_up_kernel does
//   root:                     r(a) = pid_k(a) * M_root(a), x_root the first maximal a, log r(x_root) + sM_root ln 2
//   down:                     x_child = ptr_b(x_parent), tips included
// The n <= 8 pointers of one (edge, evaluation) are 3 bits each in one 32-bit word.
#include "phm_ancestral.h"

#include <algorithm>

#include "phm_ll_device.h"

namespace phm {

namespace {

constexpr int AN_BLOCK = 256;

// max-product over one edge: m[a] and the packed pointers of the N parent states
template <int N>
__device__ __forceinline__ uint32_t an_edge(const double* __restrict__ P, size_t Kp, const double (&mc)[N], double (&m)[N]) {
  uint32_t word = 0u;
#pragma unroll
  for (int a = 0; a < N; ++a) {
    double best = 0.0;
    uint32_t at = 0u;
#pragma unroll
    for (int c = 0; c < N; ++c) {
      const double w = P[(size_t)(a * N + c) * Kp] * mc[c];
      if (w > best) { best = w; at = (uint32_t)c; }
    }
    m[a] = best;
    word |= at << (3 * a);
  }
  return word;
}

template <int N>
__global__ __launch_bounds__(AN_BLOCK) void an_up_kernel(AnParams p, const UpStep* __restrict__ steps, int k0) {
  const LlParams& q = p.ll;
  const int k = blockIdx.x * AN_BLOCK + threadIdx.x;
  if (k >= q.Kc) return;
  const UpStep u = steps[k0 + blockIdx.y];
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp, ev = (size_t)blockIdx.z * Kp + k;
  // a tip's vector is its row of L (0/1, exponent 0); an internal child's is its row of M
  const bool tip0 = u.child[0] < 0, tip1 = u.child[1] < 0;
  const double* __restrict__ v0 = tip0 ? q.L + (size_t)(~u.child[0]) * N * Ev : p.M + (size_t)u.child[0] * N * Ev;
  const double* __restrict__ v1 = tip1 ? q.L + (size_t)(~u.child[1]) * N * Ev : p.M + (size_t)u.child[1] * N * Ev;
  double c0[N], c1[N], m0[N], m1[N], v[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    c0[j] = v0[(size_t)j * Ev + ev];
    c1[j] = v1[(size_t)j * Ev + ev];
  }
  const uint32_t w0 = an_edge<N>(q.P + (size_t)u.edge[0] * N * N * Kp + k, Kp, c0, m0);
  const uint32_t w1 = an_edge<N>(q.P + (size_t)u.edge[1] * N * N * Kp + k, Kp, c1, m1);
  double mx = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    v[i] = m0[i] * m1[i];
    mx = fmax(mx, v[i]);
  }
  int e = 0;                                                       // ll_rescale's rule, fused with the store as in ll_up_kernel
  if (mx > 0.0) (void)frexp(mx, &e);
#pragma unroll
  for (int i = 0; i < N; ++i) p.M[((size_t)u.parent * N + i) * Ev + ev] = mx > 0.0 ? ldexp(v[i], -e) : v[i];
  const double s0 = tip0 ? 0.0 : p.sM[(size_t)u.child[0] * Ev + ev];
  const double s1 = tip1 ? 0.0 : p.sM[(size_t)u.child[1] * Ev + ev];
  p.sM[(size_t)u.parent * Ev + ev] = s0 + s1 + e;
  p.ptr[(size_t)u.edge[0] * Ev + ev] = w0;
  p.ptr[(size_t)u.edge[1] * Ev + ev] = w1;
}

__global__ __launch_bounds__(AN_BLOCK) void an_root_kernel(AnParams p) {
  const LlParams& q = p.ll;
  const int k = blockIdx.x * AN_BLOCK + threadIdx.x;
  if (k >= q.Kc) return;
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp, ev = (size_t)blockIdx.z * Kp + k;
  const int ri = p.root - q.n_tips;
  double best = 0.0;
  int at = 0;
  for (int a = 0; a < q.n; ++a) {
    const double r = q.pid[(size_t)a * Kp + k] * p.M[((size_t)ri * q.n + a) * Ev + ev];
    if (r > best) { best = r; at = a; }
  }
  p.x[(size_t)p.root * Ev + ev] = (uint8_t)at;
  const double v = log(best) + p.sM[(size_t)ri * Ev + ev] * LN2;
  p.jlogp[ev] = (q.bad[k] || !(best > 0.0)) ? -INFINITY : v;
}

__global__ __launch_bounds__(AN_BLOCK) void an_trace_kernel(AnParams p, const ExDown* __restrict__ steps, int k0) {
  const LlParams& q = p.ll;
  const int k = blockIdx.x * AN_BLOCK + threadIdx.x;
  if (k >= q.Kc) return;
  const ExDown d = steps[k0 + blockIdx.y];
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp, ev = (size_t)blockIdx.z * Kp + k;
  const uint32_t a = p.x[(size_t)d.parent * Ev + ev] & 7u;
  p.x[(size_t)d.child * Ev + ev] = (uint8_t)((p.ptr[(size_t)d.edge * Ev + ev] >> (3u * a)) & 7u);
}

// ex_post_kernel's arithmetic on the selected rows: O (.) L over its own sum (the log scales cancel)
__global__ __launch_bounds__(AN_BLOCK) void an_post_kernel(AnParams p, int j0) {
  const LlParams& q = p.ll;
  const int k = blockIdx.x * AN_BLOCK + threadIdx.x;
  if (k >= q.Kc) return;
  const int j = j0 + blockIdx.y, r = p.sel[j];
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp, ev = (size_t)blockIdx.z * Kp + k;
  double sum = 0.0;
  for (int i = 0; i < q.n; ++i) {
    const size_t at = ((size_t)r * q.n + i) * Ev + ev;
    sum = fma(p.O[at], q.L[at], sum);
  }
  const double inv = 1.0 / sum;
  for (int i = 0; i < q.n; ++i) {
    const size_t at = ((size_t)r * q.n + i) * Ev + ev;
    p.post[((size_t)j * q.n + i) * Ev + ev] = p.O[at] * q.L[at] * inv;
  }
}

inline bool an_ok(const AnParams& p) { return ll_ok(p.ll) && p.root >= p.ll.n_tips; }

}  // namespace

hipError_t launch_an_up(const AnParams& p, const UpStep* steps, int count, hipStream_t stream) {
  if (!an_ok(p) || !p.M || !p.sM || !p.ptr) return hipErrorInvalidValue;
  for (int k0 = 0; k0 < count; k0 += LL_GRID_Y) {
    const dim3 g = model_grid(p.ll, AN_BLOCK, std::min(LL_GRID_Y, count - k0), p.ll.n_sites);
    ll_with_states(p.ll.n, [&](auto ns) { hipLaunchKernelGGL((an_up_kernel<decltype(ns)::value>), g, dim3(AN_BLOCK), 0, stream, p, steps, k0); });
  }
  return hipGetLastError();
}

hipError_t launch_an_root(const AnParams& p, hipStream_t stream) {
  if (!an_ok(p) || !p.M || !p.sM || !p.x || !p.jlogp) return hipErrorInvalidValue;
  hipLaunchKernelGGL(an_root_kernel, model_grid(p.ll, AN_BLOCK, 1, p.ll.n_sites), dim3(AN_BLOCK), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_an_trace(const AnParams& p, const ExDown* steps, int count, hipStream_t stream) {
  if (!an_ok(p) || !p.ptr || !p.x) return hipErrorInvalidValue;
  for (int k0 = 0; k0 < count; k0 += LL_GRID_Y)
    hipLaunchKernelGGL(an_trace_kernel, model_grid(p.ll, AN_BLOCK, std::min(LL_GRID_Y, count - k0), p.ll.n_sites), dim3(AN_BLOCK), 0, stream, p,
                       steps, k0);
  return hipGetLastError();
}

hipError_t launch_an_post(const AnParams& p, int j0, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!an_ok(p) || !p.O || !p.sel || !p.post || j0 < 0 || count > LL_GRID_Y) return hipErrorInvalidValue;
  hipLaunchKernelGGL(an_post_kernel, model_grid(p.ll, AN_BLOCK, count, p.ll.n_sites), dim3(AN_BLOCK), 0, stream, p, j0);
  return hipGetLastError();
}

}  // namespace phm
