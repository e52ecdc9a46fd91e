// phm_expect.hip -- exact conditional expectations of dwell times and jump counts given the tips:
// the up (pruning) and down (outside) passes of every site and the uniformization integral of every (branch, site).
//
// Layout: every per-site vector is [row][state][site], one lane per site, so the tree records and the P(t_b) entries a lane
// reads are wave-uniform scalar loads and the vector loads are coalesced rows.  Every vector is stored rescaled by a power of
// two (max in [1/2, 1): exact), its base-2 exponent kept beside it per (row, site) as an integer-valued double.  A branch's
// factor 2^(eF + eL - e_root) / lambda is then exact up to the one division: natural-log scales of ~1e4 (a 10 000-tip tree)
// would cost ~1e-12 relative in exp(sF + sL - ll).
//
// Branch stage, I = sum_m w_m A_m with A_0 = u_0 v_0^T, A_{m+1} = B^T A_m + u_0 v_{m+1}^T, v_{m+1} = B v_m: no storage, O(M n^3)
// per (branch, site).  n <= 8: one lane per (branch, site), A and I in registers.  9..64 states: one lane per (branch, site,
// state j) owning column j of A and of I (states padded to 16 / 32 / 64 with zeros); the rows of B are LDS broadcasts and
// v_{m+1} is exchanged through LDS.  The branch (its M_b and weights) is uniform over the workgroup.
#include "phm_expect.h"

#include "phm_ll_device.h"

namespace phm {

namespace {

constexpr int EX_BLOCK = 256;

// 2^e / lambda for the integer e held in a double
__device__ __forceinline__ double ex_factor(double e, double lam) { return ldexp(1.0 / lam, (int)e); }

// ll_rescale's rule (phm_ll_device.h) on v[0 .. n) of stride Sp, n at run time
__device__ __forceinline__ int ex_rescale(double* v, int n, size_t Sp, double mx) {
  if (!(mx > 0.0)) return 0;
  int e = 0;
  (void)frexp(mx, &e);
  for (int i = 0; i < n; ++i) v[(size_t)i * Sp] = ldexp(v[(size_t)i * Sp], -e);
  return e;
}

__global__ __launch_bounds__(EX_BLOCK) void ex_tips_kernel(ExPassParams p, const uint8_t* __restrict__ tips,
                                                           const int32_t* __restrict__ obs, int t0) {
  const int s = blockIdx.x * EX_BLOCK + threadIdx.x;
  if (s >= p.Sp) return;
  const int t = t0 + blockIdx.y;
  const size_t Sp = p.Sp;
  const int y = tips[(size_t)t * Sp + s];
  for (int i = 0; i < p.n; ++i) p.L[((size_t)t * p.n + i) * Sp + s] = (y == 0 || obs[i] == y) ? 1.0 : 0.0;
  p.sL[(size_t)t * Sp + s] = 0.0;
}

__global__ __launch_bounds__(EX_BLOCK) void ex_up_kernel(ExPassParams p, const UpStep* __restrict__ steps, int k0) {
  const int s = blockIdx.x * EX_BLOCK + threadIdx.x;
  if (s >= p.Sp) return;
  const UpStep u = steps[k0 + blockIdx.y];
  const int n = p.n;
  const size_t Sp = p.Sp;
  const int r0 = u.child[0] >= 0 ? p.n_tips + u.child[0] : ~u.child[0];
  const int r1 = u.child[1] >= 0 ? p.n_tips + u.child[1] : ~u.child[1];
  const int rp = p.n_tips + u.parent;
  const double* __restrict__ P0 = p.P + (size_t)u.edge[0] * n * n;
  const double* __restrict__ P1 = p.P + (size_t)u.edge[1] * n * n;
  const double* __restrict__ L0 = p.L + (size_t)r0 * n * Sp + s;
  const double* __restrict__ L1 = p.L + (size_t)r1 * n * Sp + s;
  double* Lp = p.L + (size_t)rp * n * Sp + s;
  double mx = 0.0;
  for (int i = 0; i < n; ++i) {
    double a = 0.0, b = 0.0;
    for (int j = 0; j < n; ++j) {
      a = fma(P0[i * n + j], L0[(size_t)j * Sp], a);
      b = fma(P1[i * n + j], L1[(size_t)j * Sp], b);
    }
    const double v = a * b;
    Lp[(size_t)i * Sp] = v;
    mx = fmax(mx, v);
  }
  const int e = ex_rescale(Lp, n, Sp, mx);
  p.sL[(size_t)rp * Sp + s] = p.sL[(size_t)r0 * Sp + s] + p.sL[(size_t)r1 * Sp + s] + e;
}

__global__ __launch_bounds__(EX_BLOCK) void ex_root_kernel(ExPassParams p, int root, const double* __restrict__ pid) {
  const int s = blockIdx.x * EX_BLOCK + threadIdx.x;
  if (s >= p.Sp) return;
  const size_t Sp = p.Sp;
  double l = 0.0;
  for (int i = 0; i < p.n; ++i) {
    l = fma(pid[i], p.L[((size_t)root * p.n + i) * Sp + s], l);
    p.O[((size_t)root * p.n + i) * Sp + s] = pid[i];
  }
  p.sO[(size_t)root * Sp + s] = 0.0;
  p.lam[s] = l;
  p.ll[s] = log(l) + p.sL[(size_t)root * Sp + s] * LN2;
}

__global__ __launch_bounds__(EX_BLOCK) void ex_down_kernel(ExPassParams p, const ExDown* __restrict__ steps, int k0) {
  const int s = blockIdx.x * EX_BLOCK + threadIdx.x;
  if (s >= p.Sp) return;
  const ExDown d = steps[k0 + blockIdx.y];
  const int n = p.n;
  const size_t Sp = p.Sp;
  const double* __restrict__ Ps = p.P + (size_t)d.sib_edge * n * n;
  const double* __restrict__ Pb = p.P + (size_t)d.edge * n * n;
  const double* __restrict__ Ls = p.L + (size_t)d.sib_child * n * Sp + s;
  const double* __restrict__ Op = p.O + (size_t)d.parent * n * Sp + s;
  double* F = p.F + (size_t)d.edge * n * Sp + s;
  double* Oc = p.O + (size_t)d.child * n * Sp + s;
  double mx = 0.0;
  for (int i = 0; i < n; ++i) {                                   // F_b = O_p (.) P(t_sib) L_sib
    double a = 0.0;
    for (int j = 0; j < n; ++j) a = fma(Ps[i * n + j], Ls[(size_t)j * Sp], a);
    const double v = Op[(size_t)i * Sp] * a;
    F[(size_t)i * Sp] = v;
    mx = fmax(mx, v);
  }
  const double sF = p.sO[(size_t)d.parent * Sp + s] + p.sL[(size_t)d.sib_child * Sp + s] + ex_rescale(F, n, Sp, mx);
  p.sF[(size_t)d.edge * Sp + s] = sF;
  mx = 0.0;
  for (int i = 0; i < n; ++i) {                                   // O_c = P(t_b)^T F_b
    double a = 0.0;
    for (int k = 0; k < n; ++k) a = fma(Pb[k * n + i], F[(size_t)k * Sp], a);
    Oc[(size_t)i * Sp] = a;
    mx = fmax(mx, a);
  }
  p.sO[(size_t)d.child * Sp + s] = sF + ex_rescale(Oc, n, Sp, mx);
}

// O (.) L over its own sum: equal to O (.) L exp(sO + sL - ll) in exact arithmetic, without the rounding of the log scales
__global__ __launch_bounds__(EX_BLOCK) void ex_post_kernel(ExPassParams p, int rows, double* __restrict__ post, int r0) {
  const int s = blockIdx.x * EX_BLOCK + threadIdx.x;
  if (s >= p.Sp) return;
  const int r = r0 + blockIdx.y;
  const size_t Sp = p.Sp;
  double sum = 0.0;
  for (int i = 0; i < p.n; ++i) {
    const size_t x = ((size_t)r * p.n + i) * Sp + s;
    sum = fma(p.O[x], p.L[x], sum);
  }
  const double inv = 1.0 / sum;
  for (int i = 0; i < p.n; ++i) {
    const size_t x = ((size_t)r * p.n + i) * Sp + s;
    post[((size_t)i * rows + r) * Sp + s] = p.O[x] * p.L[x] * inv;
  }
}

template <int NS>
__global__ __launch_bounds__(EX_BLOCK) void ex_branch_lane_kernel(ExBranchParams p) {
  const int s = blockIdx.x * EX_BLOCK + threadIdx.x;
  if (s >= p.Sp) return;
  const int eo = blockIdx.y;
  const int b = p.e0 + eo;
  const int c = p.child[b];
  const size_t Sp = p.Sp;
  const double* __restrict__ B = p.B;
  const double* __restrict__ w = p.w + p.w_off[b];
  const int M = (int)(p.w_off[b + 1] - p.w_off[b]) - 1;
  double u0[NS], v[NS], A[NS][NS], I[NS][NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    u0[i] = p.F[((size_t)b * NS + i) * Sp + s];
    v[i] = p.L[((size_t)c * NS + i) * Sp + s];
  }
  const double w0 = w[0];
#pragma unroll
  for (int i = 0; i < NS; ++i)
#pragma unroll
    for (int j = 0; j < NS; ++j) { A[i][j] = u0[i] * v[j]; I[i][j] = w0 * A[i][j]; }
  for (int m = 1; m <= M; ++m) {
    double nv[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < NS; ++j) a = fma(B[i * NS + j], v[j], a);
      nv[i] = a;
    }
    const double wm = w[m];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      double t[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        double a = u0[i] * nv[j];
#pragma unroll
        for (int k = 0; k < NS; ++k) a = fma(B[k * NS + i], A[k][j], a);
        t[i] = a;
      }
#pragma unroll
      for (int i = 0; i < NS; ++i) { A[i][j] = t[i]; I[i][j] = fma(wm, t[i], I[i][j]); }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) v[i] = nv[i];
  }
  const double f = ex_factor(p.sF[(size_t)b * Sp + s] + p.sL[(size_t)c * Sp + s] - p.sL[(size_t)p.root * Sp + s], p.lam[s]);
  const size_t ld = (size_t)p.n_out_edges * Sp;
  double* out = p.out + (size_t)eo * Sp + s;
#pragma unroll
  for (int i = 0; i < NS; ++i)
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if (i == j) out[(size_t)i * ld] = I[i][i] * f;
      else out[(size_t)count_col(NS, i, j) * ld] = p.qoff[i * NS + j] * I[i][j] * f;
    }
}

// 9..64 states: lane (group g, state j) of a block of G sites; states padded to NP with zeros.  Column j of A_m lives in LDS
// (touched by lane j alone: LDS only to index it by a loop variable); column j of I in registers, or in LDS at NP = 64 (one site
// per block, 128 KB of LDS) where registers would spill.
template <int NP> struct ExWide {
  static constexpr int threads = NP == 64 ? 64 : EX_BLOCK;
  static constexpr int G = threads / NP;
  static constexpr bool i_lds = NP == 64;
};

template <int NP>
__global__ __launch_bounds__(ExWide<NP>::threads) void ex_branch_wide_kernel(ExBranchParams p) {
  constexpr int G = ExWide<NP>::G;
  constexpr bool ILDS = ExWide<NP>::i_lds;
  __shared__ __align__(16) double sB[NP * NP];     // sB[k * NP + i] = B[k][i]
  __shared__ __align__(16) double sBT[NP * NP];    // sBT[k * NP + j] = B[j][k]
  __shared__ __align__(16) double sA[G][NP][NP];   // sA[g][k][j] = A_m[k][j]
  __shared__ __align__(16) double sI[ILDS ? NP : 1][NP];
  __shared__ __align__(16) double sU[G][NP];
  __shared__ __align__(16) double sV[2][G][NP];
  const int n = p.n;
  const int tid = threadIdx.x, g = tid / NP, j = tid % NP;
  const int s = blockIdx.x * G + g;                 // Sp is a multiple of 64 >= G: always a real row of the buffers
  const int eo = blockIdx.y;
  const int b = p.e0 + eo;
  const int c = p.child[b];
  const size_t Sp = p.Sp;
  for (int x = tid; x < NP * NP; x += ExWide<NP>::threads) {
    const int k = x / NP, i = x % NP;
    const double val = (k < n && i < n) ? p.B[k * n + i] : 0.0;
    sB[x] = val;
    sBT[i * NP + k] = val;
  }
  const double* __restrict__ w = p.w + p.w_off[b];
  const int M = (int)(p.w_off[b + 1] - p.w_off[b]) - 1;
  const double vj = j < n ? p.L[((size_t)c * n + j) * Sp + s] : 0.0;
  sU[g][j] = j < n ? p.F[((size_t)b * n + j) * Sp + s] : 0.0;
  sV[0][g][j] = vj;
  __syncthreads();
  double I[ILDS ? 1 : NP];
  const double w0 = w[0];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const double a = sU[g][i] * vj;
    sA[g][i][j] = a;
    if constexpr (ILDS) sI[i][j] = w0 * a; else I[i] = w0 * a;
  }
  for (int m = 1; m <= M; ++m) {
    const int cur = (m - 1) & 1;
    double nv = 0.0;
#pragma unroll 8
    for (int k = 0; k < NP; ++k) nv = fma(sBT[k * NP + j], sV[cur][g][k], nv);
    sV[cur ^ 1][g][j] = nv;
    double t[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) t[i] = sU[g][i] * nv;
#pragma unroll 2
    for (int k = 0; k < NP; ++k) {
      const double ak = sA[g][k][j];
#pragma unroll
      for (int i = 0; i < NP; ++i) t[i] = fma(sB[k * NP + i], ak, t[i]);
    }
    const double wm = w[m];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      sA[g][i][j] = t[i];
      if constexpr (ILDS) sI[i][j] = fma(wm, t[i], sI[i][j]); else I[i] = fma(wm, t[i], I[i]);
    }
    __syncthreads();
  }
  if (j >= n) return;
  const double f = ex_factor(p.sF[(size_t)b * Sp + s] + p.sL[(size_t)c * Sp + s] - p.sL[(size_t)p.root * Sp + s], p.lam[s]);
  const size_t ld = (size_t)p.n_out_edges * Sp;
  double* out = p.out + (size_t)eo * Sp + s;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    if (i >= n) break;
    double Iij;
    if constexpr (ILDS) Iij = sI[i][j]; else Iij = I[i];
    if (i == j) out[(size_t)i * ld] = Iij * f;
    else out[(size_t)count_col(n, i, j) * ld] = p.qoff[i * n + j] * Iij * f;
  }
}

__global__ __launch_bounds__(EX_BLOCK) void ex_reduce_kernel(const double* __restrict__ out, int count, int Sp, double* tot) {
  const int s = blockIdx.x * EX_BLOCK + threadIdx.x;
  if (s >= Sp) return;
  const int col = blockIdx.y;
  const double* x = out + (size_t)col * count * Sp + s;
  double acc = tot[(size_t)col * Sp + s];
  for (int e = 0; e < count; ++e) acc += x[(size_t)e * Sp];
  tot[(size_t)col * Sp + s] = acc;
}

// Section 16: one lane per (item, site), the item uniform over the block (its edge record and P entries are scalar loads).  The
// products run in the passes' order: a as O_c = P(t_b)^T F_b, beta as the up pass's P L, so a point at s = t_b repeats O_c's sums.
__global__ __launch_bounds__(EX_BLOCK) void ex_along_kernel(ExAlongParams p, int k0) {
  const int s = blockIdx.x * EX_BLOCK + threadIdx.x;
  if (s >= p.Sp) return;
  const int k = k0 + blockIdx.y;
  const int n = p.n;
  const size_t Sp = p.Sp;
  const int b = p.edge[k], c = p.child[b];
  const double* __restrict__ Pf = p.P + (size_t)2 * k * n * n;          // P(s)
  const double* __restrict__ Pb = Pf + (size_t)n * n;                    // P(t_b - s)
  const double* __restrict__ F = p.F + (size_t)b * n * Sp + s;
  const double* __restrict__ L = p.L + (size_t)c * n * Sp + s;
  if (p.post) {                                                          // ex_post_kernel's order on (a, beta)
    const size_t ld = (size_t)p.rows * Sp;
    double* out = p.post + (size_t)k * Sp + s;
    for (int i = 0; i < n; ++i) {                                        // beta, parked in the output
      double v = 0.0;
      for (int j = 0; j < n; ++j) v = fma(Pb[i * n + j], L[(size_t)j * Sp], v);
      out[i * ld] = v;
    }
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
      double a = 0.0;
      for (int j = 0; j < n; ++j) a = fma(Pf[j * n + i], F[(size_t)j * Sp], a);
      const double be = out[i * ld];
      sum = fma(a, be, sum);
      out[i * ld] = a * be;
    }
    const double inv = 1.0 / sum;
    for (int i = 0; i < n; ++i) out[i * ld] = out[i * ld] * inv;
    return;
  }
  double* a = p.a + (size_t)k * n * Sp + s;
  double mx = 0.0;
  for (int i = 0; i < n; ++i) {
    double v = 0.0;
    for (int j = 0; j < n; ++j) v = fma(Pf[j * n + i], F[(size_t)j * Sp], v);
    a[(size_t)i * Sp] = v;
    mx = fmax(mx, v);
  }
  p.sa[(size_t)k * Sp + s] = p.sF[(size_t)b * Sp + s] + ex_rescale(a, n, Sp, mx);
  double* be = p.beta + (size_t)k * n * Sp + s;
  mx = 0.0;
  for (int i = 0; i < n; ++i) {
    double v = 0.0;
    for (int j = 0; j < n; ++j) v = fma(Pb[i * n + j], L[(size_t)j * Sp], v);
    be[(size_t)i * Sp] = v;
    mx = fmax(mx, v);
  }
  p.sbeta[(size_t)k * Sp + s] = p.sL[(size_t)c * Sp + s] + ex_rescale(be, n, Sp, mx);
}

// Lane (site, column, range): a dependent chain over the range's items in order, continued from tot across launches, so the sum
// does not depend on how the items were chunked.
__global__ __launch_bounds__(EX_BLOCK) void ex_range_sum_kernel(const double* __restrict__ x, int count, int64_t q0,
                                                                const int64_t* __restrict__ off, int r0, int n_ranges, int Sp,
                                                                double* __restrict__ tot) {
  const int s = blockIdx.x * EX_BLOCK + threadIdx.x;
  if (s >= Sp) return;
  const int col = blockIdx.y, r = r0 + blockIdx.z;
  const int64_t lo = max(off[r], q0), hi = min(off[r + 1], q0 + (int64_t)count);
  if (lo >= hi) return;
  const double* xc = x + (size_t)col * count * Sp + s;
  double* t = tot + ((size_t)col * n_ranges + r) * Sp + s;
  double acc = *t;
  for (int64_t q = lo; q < hi; ++q) acc += xc[(size_t)(q - q0) * Sp];
  *t = acc;
}

inline dim3 site_grid(int Sp, int y) { return dim3((Sp + EX_BLOCK - 1) / EX_BLOCK, y); }

template <int NP>
void launch_wide(const ExBranchParams& p, int count, hipStream_t stream) {
  hipLaunchKernelGGL((ex_branch_wide_kernel<NP>), dim3(p.Sp / ExWide<NP>::G, count), dim3(ExWide<NP>::threads), 0, stream, p);
}

}  // namespace

hipError_t launch_ex_tips(const ExPassParams& p, const uint8_t* tips, const int32_t* obs, hipStream_t stream) {
  for (int t0 = 0; t0 < p.n_tips; t0 += LL_GRID_Y)
    hipLaunchKernelGGL(ex_tips_kernel, site_grid(p.Sp, std::min(LL_GRID_Y, p.n_tips - t0)), dim3(EX_BLOCK), 0, stream, p, tips, obs, t0);
  return hipGetLastError();
}

hipError_t launch_ex_up(const ExPassParams& p, const UpStep* steps, int count, hipStream_t stream) {
  for (int k0 = 0; k0 < count; k0 += LL_GRID_Y)
    hipLaunchKernelGGL(ex_up_kernel, site_grid(p.Sp, std::min(LL_GRID_Y, count - k0)), dim3(EX_BLOCK), 0, stream, p, steps, k0);
  return hipGetLastError();
}

hipError_t launch_ex_root(const ExPassParams& p, int root_row, const double* pid, hipStream_t stream) {
  hipLaunchKernelGGL(ex_root_kernel, site_grid(p.Sp, 1), dim3(EX_BLOCK), 0, stream, p, root_row, pid);
  return hipGetLastError();
}

hipError_t launch_ex_down(const ExPassParams& p, const ExDown* steps, int count, hipStream_t stream) {
  for (int k0 = 0; k0 < count; k0 += LL_GRID_Y)
    hipLaunchKernelGGL(ex_down_kernel, site_grid(p.Sp, std::min(LL_GRID_Y, count - k0)), dim3(EX_BLOCK), 0, stream, p, steps, k0);
  return hipGetLastError();
}

hipError_t launch_ex_post(const ExPassParams& p, int rows, double* post, hipStream_t stream) {
  for (int r0 = 0; r0 < rows; r0 += LL_GRID_Y)
    hipLaunchKernelGGL(ex_post_kernel, site_grid(p.Sp, std::min(LL_GRID_Y, rows - r0)), dim3(EX_BLOCK), 0, stream, p, rows, post, r0);
  return hipGetLastError();
}

hipError_t launch_ex_branch(const ExBranchParams& p, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (count > LL_GRID_Y || p.Sp % 64 != 0) return hipErrorInvalidValue;
  if (p.n >= 2 && p.n <= EX_LANE_MAX)
    ll_with_states(p.n, [&](auto ns) { hipLaunchKernelGGL((ex_branch_lane_kernel<decltype(ns)::value>), site_grid(p.Sp, count), dim3(EX_BLOCK), 0, stream, p); });
  else if (p.n <= 16) launch_wide<16>(p, count, stream);
  else if (p.n <= 32) launch_wide<32>(p, count, stream);
  else if (p.n <= EX_MAX_STATES) launch_wide<64>(p, count, stream);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_ex_reduce(const double* out, int cols, int count, int Sp, double* tot, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (cols > LL_GRID_Y) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ex_reduce_kernel, site_grid(Sp, cols), dim3(EX_BLOCK), 0, stream, out, count, Sp, tot);
  return hipGetLastError();
}

hipError_t launch_ex_along(const ExAlongParams& p, int count, hipStream_t stream) {
  for (int k0 = 0; k0 < count; k0 += LL_GRID_Y)
    hipLaunchKernelGGL(ex_along_kernel, site_grid(p.Sp, std::min(LL_GRID_Y, count - k0)), dim3(EX_BLOCK), 0, stream, p, k0);
  return hipGetLastError();
}

hipError_t launch_ex_range_sum(const double* x, int cols, int count, int64_t q0, const int64_t* off, int r_begin, int r_end,
                               int n_ranges, int Sp, double* tot, hipStream_t stream) {
  if (count <= 0 || r_end <= r_begin) return hipSuccess;
  if (cols > LL_GRID_Y) return hipErrorInvalidValue;
  for (int r0 = r_begin; r0 < r_end; r0 += LL_GRID_Y)
    hipLaunchKernelGGL(ex_range_sum_kernel, dim3((Sp + EX_BLOCK - 1) / EX_BLOCK, cols, std::min(LL_GRID_Y, r_end - r0)),
                       dim3(EX_BLOCK), 0, stream, x, count, q0, off, r0, n_ranges, Sp, tot);
  return hipGetLastError();
}

}  // namespace phm
