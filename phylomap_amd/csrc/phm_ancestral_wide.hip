// phm_ancestral_wide.hip -- ancestral states for many rate matrices at 9..64 states: section 13's up, root,
// down and posterior arithmetic (ex_tips_kernel, ex_up_kernel, ex_root_kernel, ex_down_kernel, ex_post_kernel of phm_expect.hip)
// and section 21's joint reconstruction (phm_ancestral.hip), restated with ONE STATE PER LANE and batched over models and sites.
//
// A group of NP lanes (16 / 32 / 64 for 9..16 / 17..32 / 33..64 states) owns one (evaluation, node) item; lane a holds state a and
// the lanes past n hold zeros.  A workgroup of 256 lanes takes (level step, model, tile of sites): it stages the step's two
// transition matrices of ITS model in LDS once and its 256 / NP groups walk AW_WALK sites each through them.
//   * lane a's chain over j = 0 .. n-1 is the serial fma chain of the one-lane kernels: same operands, same order, same bits
//   * the maximum of a vector is a cross-lane fmax (exact in any order)
//   * the ordered dot products (root, posterior) are one serial chain on the group's first lane, read from LDS
//   * the root's argmax is the cross-lane maximum followed by the lowest lane that attains it
// LDS: a matrix read as v[a] = sum_j P[a][j] c[j] is staged TRANSPOSED, sP[j * (NP + 1) + a], so for fixed j the lanes read
// consecutive doubles (ds_read_b64: 32 lanes x 8 bytes = the 64 banks once) and the staging stores of consecutive j are NP + 1
// doubles apart (odd: the 16 lanes of a ds_write_b64 group fall on 16 different bank pairs).  The down pass' O_c = P^T F reads
// row-major P[k][a] consecutively as stored.  A group's child vector is an LDS broadcast; the rows of two groups of one half-wave
// are NP + 2 doubles apart per vector, which keeps them on different banks at NP = 16.
// Every loop is bounded by n, the step count or the site tile; the arithmetic of the joint reconstruction is explicit products.
// For section 26 (phm_scores_wide.hip) the root stores lam = pid_k . L_root, its chain's value before the log, and the down pass
// has a second instantiation that stores F_b and its exponent (AwParams' lam, F and sF).  The lane pieces (shape, group maximum,
// rescale, transposed staging) are phm_aw_device.h's.
#include "phm_ancestral_wide.h"

#include "phm_aw_device.h"

#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

namespace phm {

namespace {

constexpr int AW_WALK = 4;                     // sites a group walks through the staged matrices

// doubles of LDS: two staged matrices, two vectors per group
template <int NP> inline size_t aw_lds_doubles(int n) { return (size_t)2 * n * AwShape<NP>::LD + (size_t)2 * AwShape<NP>::G * AwShape<NP>::VS; }

__global__ __launch_bounds__(AW_BLOCK) void aw_tips_kernel(AwParams p, int t0) {
  const size_t Ev = (size_t)p.Kc * p.Sc;
  const size_t at = (size_t)blockIdx.x * AW_BLOCK + threadIdx.x;
  if (at >= Ev * p.NP) return;
  const size_t ev = at / p.NP;
  const int a = (int)(at - ev * p.NP);
  const int k = (int)(ev / p.Sc), s = (int)(ev - (size_t)k * p.Sc);
  const int t = t0 + blockIdx.y;
  const int y = p.tips[((size_t)k * p.tip_model + (size_t)s * p.tip_site) * p.n_tips + t];
  p.L[((size_t)t * Ev + ev) * p.NP + a] = (a < p.n && (y == 0 || p.obs[a] == y)) ? 1.0 : 0.0;
  if (a == 0) p.sL[(size_t)t * Ev + ev] = 0;
}

// grid: (step, model, site tile)
template <int NP, bool JOINT>
__global__ __launch_bounds__(AW_BLOCK) void aw_up_kernel(AwParams p, const UpStep* __restrict__ steps) {
  constexpr int G = AwShape<NP>::G, LD = AwShape<NP>::LD, VS = AwShape<NP>::VS;
  extern __shared__ __align__(16) double aw_lds[];
  const int n = p.n;
  double* sP0 = aw_lds;
  double* sP1 = sP0 + n * LD;
  double* sV = sP1 + n * LD;
  const UpStep u = steps[blockIdx.x];
  const int k = blockIdx.y;
  const int g = threadIdx.x / NP, a = threadIdx.x % NP;
  const size_t Ev = (size_t)p.Kc * p.Sc, nn = (size_t)n * n;
  const double* __restrict__ Pm = p.P + (size_t)k * p.n_edge * nn;
  aw_stage_t<NP>(sP0, Pm + (size_t)u.edge[0] * nn, n);
  aw_stage_t<NP>(sP1, Pm + (size_t)u.edge[1] * nn, n);
  const bool tip0 = u.child[0] < 0, tip1 = u.child[1] < 0;
  // sum-product: a child's row of L; max-product: a tip's row of L (0/1, exponent 0) or an internal child's row of M
  const double* __restrict__ v0;
  const double* __restrict__ v1;
  const int32_t* __restrict__ e0;
  const int32_t* __restrict__ e1;
  if (JOINT) {
    v0 = tip0 ? p.L + (size_t)(~u.child[0]) * Ev * NP : p.M + (size_t)u.child[0] * Ev * NP;
    v1 = tip1 ? p.L + (size_t)(~u.child[1]) * Ev * NP : p.M + (size_t)u.child[1] * Ev * NP;
    e0 = tip0 ? p.sL + (size_t)(~u.child[0]) * Ev : p.sM + (size_t)u.child[0] * Ev;
    e1 = tip1 ? p.sL + (size_t)(~u.child[1]) * Ev : p.sM + (size_t)u.child[1] * Ev;
  } else {
    const size_t r0 = tip0 ? (size_t)(~u.child[0]) : (size_t)p.n_tips + u.child[0];
    const size_t r1 = tip1 ? (size_t)(~u.child[1]) : (size_t)p.n_tips + u.child[1];
    v0 = p.L + r0 * Ev * NP; v1 = p.L + r1 * Ev * NP;
    e0 = p.sL + r0 * Ev; e1 = p.sL + r1 * Ev;
  }
  double* out = JOINT ? p.M + (size_t)u.parent * Ev * NP : p.L + ((size_t)p.n_tips + u.parent) * Ev * NP;
  int32_t* eout = JOINT ? p.sM + (size_t)u.parent * Ev : p.sL + ((size_t)p.n_tips + u.parent) * Ev;
  const double* c0 = sV + (g * 2) * VS;
  const double* c1 = sV + (g * 2 + 1) * VS;
  for (int w = 0; w < AW_WALK; ++w) {
    const int sb = (blockIdx.z * AW_WALK + w) * G;                 // uniform over the workgroup
    if (sb >= p.Sc) break;
    const int s = sb + g;
    const bool on = s < p.Sc;
    const size_t ev = (size_t)k * p.Sc + (on ? s : 0);
    __syncthreads();                                               // the matrices are staged; the last item's vectors are read
    if (on) {
      sV[(g * 2) * VS + a] = v0[ev * NP + a];
      sV[(g * 2 + 1) * VS + a] = v1[ev * NP + a];
    }
    __syncthreads();
    if (!on) continue;
    double v;
    if (JOINT) {
      double b0 = 0.0, b1 = 0.0;
      int at0 = 0, at1 = 0;
      for (int c = 0; c < n; ++c) {                                // the first maximum wins
        const double w0 = sP0[c * LD + a] * c0[c];
        const double w1 = sP1[c * LD + a] * c1[c];
        if (w0 > b0) { b0 = w0; at0 = c; }
        if (w1 > b1) { b1 = w1; at1 = c; }
      }
      if (a >= n) { b0 = 0.0; b1 = 0.0; at0 = 0; at1 = 0; }
      v = b0 * b1;
      p.ptr[((size_t)u.edge[0] * Ev + ev) * NP + a] = (uint8_t)at0;
      p.ptr[((size_t)u.edge[1] * Ev + ev) * NP + a] = (uint8_t)at1;
    } else {
      double s0 = 0.0, s1 = 0.0;
      for (int j = 0; j < n; ++j) {
        s0 = fma(sP0[j * LD + a], c0[j], s0);
        s1 = fma(sP1[j * LD + a], c1[j], s1);
      }
      v = a < n ? s0 * s1 : 0.0;
    }
    int e;
    v = aw_rescale(v, aw_group_max<NP>(v), e);
    out[ev * NP + a] = v;
    if (a == 0) eout[ev] = e0[ev] + e1[ev] + e;
  }
}

// grid: (model, site tile).  l = sum_i pid[i] L_root[i] in state order on the group's first lane.
template <int NP>
__global__ __launch_bounds__(AW_BLOCK) void aw_root_kernel(AwParams p) {
  constexpr int G = AwShape<NP>::G, VS = AwShape<NP>::VS;
  __shared__ double sV[2 * G * VS];
  const int n = p.n, k = blockIdx.x;
  const int g = threadIdx.x / NP, a = threadIdx.x % NP;
  const size_t Ev = (size_t)p.Kc * p.Sc;
  const int s = blockIdx.y * G + g;
  const bool on = s < p.Sc;
  const size_t ev = (size_t)k * p.Sc + (on ? s : 0);
  const double pi = a < n ? p.pid[(size_t)k * n + a] : 0.0;
  if (on) {
    sV[(g * 2) * VS + a] = pi;
    sV[(g * 2 + 1) * VS + a] = p.L[((size_t)p.root * Ev + ev) * NP + a];
  }
  __syncthreads();
  if (!on) return;
  if (p.O) {
    p.O[((size_t)p.root * Ev + ev) * NP + a] = pi;
    if (a == 0) p.sO[(size_t)p.root * Ev + ev] = 0;
  }
  if (a == 0) {
    double l = 0.0;
    for (int i = 0; i < n; ++i) l = fma(sV[(g * 2) * VS + i], sV[(g * 2 + 1) * VS + i], l);
    if (p.lam) p.lam[ev] = l;
    p.ll[ev] = log(l) + (double)p.sL[(size_t)p.root * Ev + ev] * LN2;
  }
}

// grid: (step, model, site tile).  F = O_p (.) (P_sib L_sib), O_c = P_b^T F.  STORE_F: F and its exponent are stored per edge row
// (the branch stage of phm_scores_wide.hip reads them).
template <int NP, bool STORE_F>
__global__ __launch_bounds__(AW_BLOCK) void aw_down_kernel(AwParams p, const ExDown* __restrict__ steps) {
  constexpr int G = AwShape<NP>::G, LD = AwShape<NP>::LD, VS = AwShape<NP>::VS;
  extern __shared__ __align__(16) double aw_lds[];
  const int n = p.n;
  double* sPs = aw_lds;                                            // sibling branch, transposed
  double* sPb = sPs + n * LD;                                      // this branch, row-major [k][i] as stored
  double* sV = sPb + n * LD;
  const ExDown d = steps[blockIdx.x];
  const int k = blockIdx.y;
  const int g = threadIdx.x / NP, a = threadIdx.x % NP;
  const size_t Ev = (size_t)p.Kc * p.Sc, nn = (size_t)n * n;
  const double* __restrict__ Pm = p.P + (size_t)k * p.n_edge * nn;
  aw_stage_t<NP>(sPs, Pm + (size_t)d.sib_edge * nn, n);
  {
    const double* __restrict__ Pb = Pm + (size_t)d.edge * nn;
    for (int e = threadIdx.x; e < n * n; e += AW_BLOCK) sPb[e] = Pb[e];
  }
  double* cs = sV + (g * 2) * VS;
  double* cf = sV + (g * 2 + 1) * VS;
  for (int w = 0; w < AW_WALK; ++w) {
    const int sb = (blockIdx.z * AW_WALK + w) * G;
    if (sb >= p.Sc) break;
    const int s = sb + g;
    const bool on = s < p.Sc;
    const size_t ev = (size_t)k * p.Sc + (on ? s : 0);
    __syncthreads();
    if (on) cs[a] = p.L[((size_t)d.sib_child * Ev + ev) * NP + a];
    __syncthreads();
    double f = 0.0;
    int eF = 0;
    if (on) {
      double acc = 0.0;
      for (int j = 0; j < n; ++j) acc = fma(sPs[j * LD + a], cs[j], acc);
      f = a < n ? p.O[((size_t)d.parent * Ev + ev) * NP + a] * acc : 0.0;
      f = aw_rescale(f, aw_group_max<NP>(f), eF);
      cf[a] = f;
      if constexpr (STORE_F) p.F[((size_t)d.edge * Ev + ev) * NP + a] = f;
    }
    __syncthreads();
    if (!on) continue;
    double o = 0.0;
    for (int kk = 0; kk < n; ++kk) o = fma(sPb[kk * n + a], cf[kk], o);   // lanes past n read inside the staged block and are zeroed
    if (a >= n) o = 0.0;
    int eO;
    o = aw_rescale(o, aw_group_max<NP>(o), eO);
    p.O[((size_t)d.child * Ev + ev) * NP + a] = o;
    if (a == 0) {
      const int32_t sF = p.sO[(size_t)d.parent * Ev + ev] + p.sL[(size_t)d.sib_child * Ev + ev] + eF;
      if constexpr (STORE_F) p.sF[(size_t)d.edge * Ev + ev] = sF;
      p.sO[(size_t)d.child * Ev + ev] = sF + eO;
    }
  }
}

// grid: (selected row, model, site tile).  sum = sum_i O[i] L[i] in state order on the group's first lane, one reciprocal.
template <int NP>
__global__ __launch_bounds__(AW_BLOCK) void aw_post_kernel(AwParams p, int j0) {
  constexpr int G = AwShape<NP>::G, VS = AwShape<NP>::VS;
  __shared__ double sV[2 * G * VS];
  __shared__ double sS[G];
  const int n = p.n, k = blockIdx.y;
  const int j = j0 + blockIdx.x, r = p.sel[j];
  const int g = threadIdx.x / NP, a = threadIdx.x % NP;
  const size_t Ev = (size_t)p.Kc * p.Sc;
  const int s = blockIdx.z * G + g;
  const bool on = s < p.Sc;
  const size_t ev = (size_t)k * p.Sc + (on ? s : 0);
  const size_t at = ((size_t)r * Ev + ev) * NP + a;
  const double o = on ? p.O[at] : 0.0, l = on ? p.L[at] : 0.0;
  sV[(g * 2) * VS + a] = o;
  sV[(g * 2 + 1) * VS + a] = l;
  __syncthreads();
  if (a == 0) {
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum = fma(sV[(g * 2) * VS + i], sV[(g * 2 + 1) * VS + i], sum);
    sS[g] = 1.0 / sum;
  }
  __syncthreads();
  if (on && a < n) p.post[(ev * p.J + j) * n + a] = o * l * sS[g];
}

// grid: (model, site tile)
template <int NP>
__global__ __launch_bounds__(AW_BLOCK) void aw_jroot_kernel(AwParams p) {
  constexpr int G = AwShape<NP>::G;
  const int n = p.n, k = blockIdx.x;
  const int g = threadIdx.x / NP, a = threadIdx.x % NP;
  const size_t Ev = (size_t)p.Kc * p.Sc;
  const int s = blockIdx.y * G + g;
  if (s >= p.Sc) return;                                           // a whole group leaves: the shuffles stay inside a group
  const size_t ev = (size_t)k * p.Sc + s;
  const int ri = p.root - p.n_tips;
  const double r = a < n ? p.pid[(size_t)k * n + a] * p.M[((size_t)ri * Ev + ev) * NP + a] : 0.0;
  const double best = aw_group_max<NP>(r);
  int at = (best > 0.0 && r == best) ? a : NP;
#pragma unroll
  for (int off = NP / 2; off >= 1; off >>= 1) at = min(at, __shfl_xor(at, off, NP));
  if (a == 0) {
    p.x[(size_t)p.root * Ev + ev] = (uint8_t)(at == NP ? 0 : at);
    const double v = log(best) + (double)p.sM[(size_t)ri * Ev + ev] * LN2;
    p.jlogp[ev] = best > 0.0 ? v : -INFINITY;
  }
}

// grid: (evaluations / block, step)
template <int NP>
__global__ __launch_bounds__(AW_BLOCK) void aw_trace_kernel(AwParams p, const ExDown* __restrict__ steps) {
  const size_t Ev = (size_t)p.Kc * p.Sc;
  const size_t ev = (size_t)blockIdx.x * AW_BLOCK + threadIdx.x;
  if (ev >= Ev) return;
  const ExDown d = steps[blockIdx.y];
  const uint32_t a = p.x[(size_t)d.parent * Ev + ev] & (uint32_t)(NP - 1);
  p.x[(size_t)d.child * Ev + ev] = p.ptr[((size_t)d.edge * Ev + ev) * NP + a];
}

inline bool aw_ok(const AwParams& p) {
  return p.n >= AW_MIN_STATES && p.n <= EX_MAX_STATES && p.NP == aw_lanes(p.n) && p.Kc >= 1 && p.Kc <= AW_GRID_MAX && p.Sc >= 1 &&
         p.Sc <= AW_GRID_MAX && (size_t)p.Kc * p.Sc <= (size_t)INT32_MAX && p.root >= p.n_tips && p.P && p.pid && p.L && p.sL;
}

template <int NP> inline int aw_tiles(const AwParams& p) { return (p.Sc + AwShape<NP>::G * AW_WALK - 1) / (AwShape<NP>::G * AW_WALK); }
template <int NP> inline int aw_rows(const AwParams& p) { return (p.Sc + AwShape<NP>::G - 1) / AwShape<NP>::G; }

template <int NP, bool JOINT>
hipError_t aw_up(const AwParams& p, const UpStep* steps, int count, hipStream_t stream) {
  const size_t lds = sizeof(double) * aw_lds_doubles<NP>(p.n);
  const hipError_t e = aw_allow_lds(reinterpret_cast<const void*>(aw_up_kernel<NP, JOINT>), (int)(sizeof(double) * aw_lds_doubles<NP>(NP)));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((aw_up_kernel<NP, JOINT>), dim3(count, p.Kc, aw_tiles<NP>(p)), dim3(AW_BLOCK), lds, stream, p, steps);
  return hipGetLastError();
}

template <int NP, bool STORE_F>
hipError_t aw_down(const AwParams& p, const ExDown* steps, int count, hipStream_t stream) {
  const size_t lds = sizeof(double) * aw_lds_doubles<NP>(p.n);
  const hipError_t e = aw_allow_lds(reinterpret_cast<const void*>(aw_down_kernel<NP, STORE_F>), (int)(sizeof(double) * aw_lds_doubles<NP>(NP)));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((aw_down_kernel<NP, STORE_F>), dim3(count, p.Kc, aw_tiles<NP>(p)), dim3(AW_BLOCK), lds, stream, p, steps);
  return hipGetLastError();
}

}  // namespace

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the function object of the current device: set once per (function,
// device) to the most its class can ask for (here n = NP: 70 784 bytes at 64 states, above the 64 KiB a launch gets unasked);
// phm_sample_wide.hip's table kernel asks through it as well
hipError_t aw_allow_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::vector<std::pair<const void*, int>> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> guard(mu);
  for (const auto& d : done) if (d.first == fn && d.second == dev) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.emplace_back(fn, dev);
  return e;
}

hipError_t launch_aw_tips(const AwParams& p, hipStream_t stream) {
  if (!aw_ok(p) || !p.tips || !p.obs) return hipErrorInvalidValue;
  const size_t cells = (size_t)p.Kc * p.Sc * p.NP;
  for (int t0 = 0; t0 < p.n_tips; t0 += AW_GRID_MAX)
    hipLaunchKernelGGL(aw_tips_kernel, dim3((unsigned)((cells + AW_BLOCK - 1) / AW_BLOCK), std::min(AW_GRID_MAX, p.n_tips - t0)),
                       dim3(AW_BLOCK), 0, stream, p, t0);
  return hipGetLastError();
}

hipError_t launch_aw_up(const AwParams& p, const UpStep* steps, int count, bool joint, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!aw_ok(p) || !steps || (joint && (!p.M || !p.sM || !p.ptr))) return hipErrorInvalidValue;
  return aw_with_lanes(p.NP, [&](auto np) {
    constexpr int NP_ = decltype(np)::value;
    return joint ? aw_up<NP_, true>(p, steps, count, stream) : aw_up<NP_, false>(p, steps, count, stream);
  });
}

hipError_t launch_aw_root(const AwParams& p, hipStream_t stream) {
  if (!aw_ok(p) || !p.ll || (p.O && !p.sO)) return hipErrorInvalidValue;
  return aw_with_lanes(p.NP, [&](auto np) {
    constexpr int NP_ = decltype(np)::value;
    hipLaunchKernelGGL((aw_root_kernel<NP_>), dim3(p.Kc, aw_rows<NP_>(p)), dim3(AW_BLOCK), 0, stream, p);
    return hipGetLastError();
  });
}

hipError_t launch_aw_down(const AwParams& p, const ExDown* steps, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!aw_ok(p) || !steps || !p.O || !p.sO || (p.F && !p.sF) || count > AW_GRID_MAX) return hipErrorInvalidValue;
  return aw_with_lanes(p.NP, [&](auto np) {
    constexpr int NP_ = decltype(np)::value;
    return p.F ? aw_down<NP_, true>(p, steps, count, stream) : aw_down<NP_, false>(p, steps, count, stream);
  });
}

hipError_t launch_aw_post(const AwParams& p, int j0, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!aw_ok(p) || !p.O || !p.sel || !p.post || j0 < 0 || j0 + count > p.J) return hipErrorInvalidValue;
  return aw_with_lanes(p.NP, [&](auto np) {
    constexpr int NP_ = decltype(np)::value;
    hipLaunchKernelGGL((aw_post_kernel<NP_>), dim3(count, p.Kc, aw_rows<NP_>(p)), dim3(AW_BLOCK), 0, stream, p, j0);
    return hipGetLastError();
  });
}

hipError_t launch_aw_jroot(const AwParams& p, hipStream_t stream) {
  if (!aw_ok(p) || !p.M || !p.sM || !p.x || !p.jlogp) return hipErrorInvalidValue;
  return aw_with_lanes(p.NP, [&](auto np) {
    constexpr int NP_ = decltype(np)::value;
    hipLaunchKernelGGL((aw_jroot_kernel<NP_>), dim3(p.Kc, aw_rows<NP_>(p)), dim3(AW_BLOCK), 0, stream, p);
    return hipGetLastError();
  });
}

hipError_t launch_aw_trace(const AwParams& p, const ExDown* steps, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!aw_ok(p) || !steps || !p.ptr || !p.x || count > AW_GRID_MAX) return hipErrorInvalidValue;
  const size_t Ev = (size_t)p.Kc * p.Sc;
  const dim3 grid((unsigned)((Ev + AW_BLOCK - 1) / AW_BLOCK), count);
  return aw_with_lanes(p.NP, [&](auto np) {
    hipLaunchKernelGGL((aw_trace_kernel<decltype(np)::value>), grid, dim3(AW_BLOCK), 0, stream, p, steps);
    return hipGetLastError();
  });
}

}  // namespace phm
