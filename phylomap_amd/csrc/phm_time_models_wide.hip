// phm_time_models_wide.hip -- the exact expectations through time for many rate matrices at 9..64 states:
// section 28's along-branch vectors, sub-branch integrals and fixed-order sums with ONE STATE PER LANE, on top of section 23's
// P_k(t_b), up pass, root (lam stored) and down pass (F_b stored) and section 26's model kernel (mu_k, B_k), all launched unchanged.
//
// The mapping is scw_branch_kernel's and brw_branch_kernel's: groups of NP lanes (16 / 32 / 64 for 9..16 / 17..32 / 33..64 states),
// lane a holds state a and the lanes past n hold zeros; a workgroup takes (TMW_WALK consecutive items of the launch, one model, a
// tile of sites) and stages B_k once, row-major and transposed, rows NP + 1 doubles apart.  Its groups walk TMW_SITES sites each
// and, per site, the items.  At any moment all groups of a workgroup are on the same model and the same item, and everything that
// decides how often a loop with a barrier turns -- x = mu_k t of the uniformization sums, the end of a branch, the form and M of the
// branch stage -- depends on (model, item) alone: a workgroup never diverges over a barrier.
//
// tmw_along_kernel: beta = P_k(t2) L_c, then a = P_k(t1)^T F_b, both by section 28's uniformization sum with x = mu_k t:
//   P(t) v = sum_m w_m B^m v / sum_m w_m,   w_0 = 1,  w_{m+1} = w_m x / (m + 1)
// rescaled by 2^-512 whenever w passes 2^512 and ended at the first m past the mode whose geometric tail bound
// w_{m+1} / (1 - x / (m + 2)) is at most 2^-60 of the sum (hard end SC_M_CAP).  Each B^m v is a mat-vec through LDS: lane a runs
// the ordered fma chain over row a of B (of B^T for a), the vector is an LDS broadcast and ping-pongs between two rows.  The ends
// of a branch take no sum: t = 0 returns the stored vector unchanged and t = t_b multiplies by the stored P_k(t_b) in the passes'
// own order (beta as aw_up_kernel's P L, a as aw_down_kernel's O_c = P^T F), so a point at a node repeats the node's sums.
// mu_k = 0 gives x = 0 and the vector unchanged at every t.  Posterior mode forms pi = a (.) beta / sum in state order; vector mode
// stores a and beta rescaled (aw_rescale) with their exponents.
//
// tmw_branch_kernel: brw_branch_kernel's body (scw_branch_kernel's, operation for operation) on a sub-branch: (F_b, L_c, t_b) are
// (a(s1), beta(s2), h) with the factor 2^(e_a + e_beta - e_root) / lam.  RESTATED here for section 27's reason: those kernels stay
// as they are.  Which form an item takes, and the short form's M, is sw_form_terms' word, evaluated by every lane from the same two
// scalars (tmw_form_terms, phm_time_models_wide_form.h): no K x items table is made on the host.
//
// tmw_range_sum_kernel: tm_range_sum_kernel's sum for this family's [item][Ev][col] layout: a lane owns one cell of one range and
// adds the range's items in item order, continued across launches.  No atomics.
// Every loop is bounded by n, M <= SW_M_CAP, SC_M_CAP, the walk, the site tile or the item count.
#include "phm_time_models_wide.h"

#include "phm_aw_device.h"

#include <algorithm>

namespace phm {

namespace {

constexpr int TMW_SUM_BLOCK = 256;

// scw_branch_kernel's shape: few groups per workgroup, because a call has one site or a few
template <int NP> struct TmwShape {
  static constexpr int G = NP == 16 ? 4 : 2;   // tmw_groups(NP)
  static constexpr int threads = G * NP;       // 64, 64, 128
  static constexpr int LD = AwShape<NP>::LD;
  static constexpr int VS = AwShape<NP>::VS;
  static constexpr int VR = SW_M_CAP + 1;      // rows of a group's V in the branch stage
  // along stage: B, B^T; a group's vector ping-pong; a and beta of the posterior
  static constexpr size_t along_doubles = (size_t)2 * NP * LD + (size_t)4 * G * VS;
  // branch stage (brw_branch_kernel's): B, B^T; V (A_m of the long form in its place); u ping-pong, the long form's v ping-pong;
  // the weights
  static constexpr size_t branch_doubles = (size_t)2 * NP * LD + (size_t)G * VR * VS + (size_t)4 * G * VS + VR;
  static_assert(NP * NP <= VR * VS, "A_m of the long form lives in a group's V");
};

// sB[k * LD + i] = B[k][i] and sBT[k * LD + j] = B[j][k], zeros for the columns n .. NP - 1, as scw_branch_kernel stages them
template <int NP, int THREADS>
__device__ __forceinline__ void tmw_stage_b(double* sB, double* sBT, const double* __restrict__ Bk, int n) {
  constexpr int LD = AwShape<NP>::LD;
  const int tid = threadIdx.x;
  for (int e = tid; e < n * n; e += THREADS) {
    const int i = e / n, j = e - i * n;
    const double v = Bk[e];
    sB[i * LD + j] = v;
    sBT[j * LD + i] = v;
  }
  const int pad = NP - n;
  for (int e = tid; e < n * pad; e += THREADS) {
    const int r = e / pad, c = n + (e - r * pad);
    sB[r * LD + c] = 0.0;
    sBT[r * LD + c] = 0.0;
  }
}

// This lane's component of P(t) v (M = sBT: M[j * LD + a] = B[a][j]) or of P(t)^T v (M = sB: M[j * LD + a] = B[j][a]) for
// x = mu t; v is this lane's component of the vector, x0 and x1 the group's two vector rows.  tm_apply's sum (phm_time_models.hip)
// with the vector across the lanes.  Every lane of the workgroup calls it with the same x.
template <int NP>
__device__ __forceinline__ double tmw_apply(const double* __restrict__ M, double* x0, double* x1, int n, int a, double x, double v) {
  constexpr int LD = AwShape<NP>::LD;
  x0[a] = v;
  __syncthreads();
  double acc = v, w = 1.0, S = 1.0;
  int cur = 0;
  // a barrier a turn: the trip count depends on x = mu_k t alone, that is on (model, item), the same in every group
  for (int m = 0; m < SC_M_CAP; ++m) {
    const double wn = w * (x / (double)(m + 1));
    // past the mode (x < m + 1) the terms fall at least geometrically: sum_{j > m} w_j <= w_{m+1} / (1 - x / (m + 2))
    if (x < (double)(m + 1) && wn <= 0x1p-60 * S * (1.0 - x / (double)(m + 2))) break;
    const double* src = cur ? x1 : x0;
    double nv = 0.0;
#pragma unroll 8
    for (int j = 0; j < n; ++j) nv = fma(M[j * LD + a], src[j], nv);
    (cur ? x0 : x1)[a] = nv;
    w = wn;
    S += w;
    acc = fma(w, nv, acc);
    if (w > 0x1p512) {
      w *= 0x1p-512;
      S *= 0x1p-512;
      acc *= 0x1p-512;
    }
    cur ^= 1;
    __syncthreads();
  }
  return acc * (1.0 / S);
}

// grid: (walks of the launch's items, model, site tile)
template <int NP>
__global__ __launch_bounds__(TmwShape<NP>::threads) void tmw_along_kernel(TmwParams p, int count) {
  using Sh = TmwShape<NP>;
  constexpr int G = Sh::G, LD = Sh::LD, VS = Sh::VS, THREADS = Sh::threads;
  extern __shared__ __align__(16) double tmw_lds[];
  const ScwParams& q = p.sc;
  const AwParams& w = q.aw;
  const int n = w.n;
  double* sB = tmw_lds;                                            // sB[k * LD + i] = B[k][i]
  double* sBT = sB + NP * LD;                                      // sBT[k * LD + j] = B[j][k]
  double* sX = sBT + NP * LD;                                      // [2][G][VS] a group's vector ping-pong
  double* sY = sX + 2 * G * VS;                                    // [2][G][VS] a and beta of the posterior
  const int tid = threadIdx.x, g = tid / NP, a = tid % NP;
  const int k = blockIdx.y;
  const int j_begin = blockIdx.x * TMW_WALK, j_end = min(count, j_begin + TMW_WALK);
  const size_t Ev = (size_t)w.Kc * w.Sc, nn = (size_t)n * n;
  const double mu = q.mu[k];
  const bool still = !(mu > 0.0);                                  // the model leaves no state: P = I
  tmw_stage_b<NP, THREADS>(sB, sBT, q.B + (size_t)k * nn, n);
  const double* __restrict__ Pm = w.P + (size_t)k * w.n_edge * nn; // P_k(t_b) of every edge row, row-major
  double* x0 = sX + (size_t)g * VS;
  double* x1 = sX + (size_t)(G + g) * VS;
  double* ya = sY + (size_t)g * VS;
  double* yb = sY + (size_t)(G + g) * VS;
  const bool posterior = p.post != nullptr;
  for (int ws = 0; ws < TMW_SITES; ++ws) {
    const int sb = (blockIdx.z * TMW_SITES + ws) * G;              // uniform over the workgroup
    if (sb >= w.Sc) break;
    const int s = sb + g;
    const bool on = s < w.Sc;                                      // a group past the last site repeats site sb and stores nothing
    const size_t ev = (size_t)k * w.Sc + (on ? s : sb);
    // no barrier inside this loop is conditional on anything but the item: its bounds are the workgroup's
    for (int j = j_begin; j < j_end; ++j) {
      const TmItem it = p.items[j];                                // uniform over the workgroup
      const int b = it.edge, c = q.child[b];
      const double tb = q.t[b];
      const double* __restrict__ Pb = Pm + (size_t)b * nn;
      const double vL = w.L[((size_t)c * Ev + ev) * NP + a];
      const double vF = w.F[((size_t)b * Ev + ev) * NP + a];
      __syncthreads();                                             // B is staged; the last item's vectors are read
      // beta = P(t2) L_c
      double be = vL;
      if (it.t2 == tb && tb != 0.0) {                              // the parent end: the up pass's P L
        x0[a] = vL;
        __syncthreads();
        double acc = 0.0;
        if (a < n)
          for (int jj = 0; jj < n; ++jj) acc = fma(Pb[(size_t)a * n + jj], x0[jj], acc);
        be = acc;
      } else if (it.t2 != 0.0) {
        be = tmw_apply<NP>(sBT, x0, x1, n, a, still ? 0.0 : mu * it.t2, vL);
      }
      __syncthreads();                                             // beta's reads of the group's rows are done
      // a = P(t1)^T F_b
      double av = vF;
      if (it.t1 == tb && tb != 0.0) {                              // the child end: aw_down_kernel's O_c = P(t_b)^T F_b
        x0[a] = vF;
        __syncthreads();
        double acc = 0.0;
        if (a < n)
          for (int kk = 0; kk < n; ++kk) acc = fma(Pb[(size_t)kk * n + a], x0[kk], acc);
        av = acc;
      } else if (it.t1 != 0.0) {
        av = tmw_apply<NP>(sB, x0, x1, n, a, still ? 0.0 : mu * it.t1, vF);
      }
      if (posterior) {                                             // aw_post_kernel's order on (a, beta): one chain in state order
        ya[a] = av;
        yb[a] = be;
        __syncthreads();
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum = fma(ya[i], yb[i], sum);
        const double inv = 1.0 / sum;
        if (on && a < n) p.post[((size_t)j * Ev + ev) * n + a] = (av * be) * inv;
        continue;
      }
      int ea, eb;
      av = aw_rescale(av, aw_group_max<NP>(av), ea);
      be = aw_rescale(be, aw_group_max<NP>(be), eb);
      if (on) {
        p.a[((size_t)j * Ev + ev) * NP + a] = av;
        p.beta[((size_t)j * Ev + ev) * NP + a] = be;
        if (a == 0) {
          p.sa[(size_t)j * Ev + ev] = w.sF[(size_t)b * Ev + ev] + ea;
          p.sbeta[(size_t)j * Ev + ev] = w.sL[(size_t)c * Ev + ev] + eb;
        }
      }
    }
  }
}

// grid: (walks of the launch's sub-branches, model, site tile)
template <int NP>
__global__ __launch_bounds__(TmwShape<NP>::threads) void tmw_branch_kernel(TmwParams tp, int count) {
  using Sh = TmwShape<NP>;
  constexpr int G = Sh::G, LD = Sh::LD, VS = Sh::VS, VR = Sh::VR, THREADS = Sh::threads;
  extern __shared__ __align__(16) double tmw_lds[];
  const ScwParams& q = tp.sc;
  const AwParams& p = q.aw;
  const int n = p.n;
  double* sB = tmw_lds;                                            // sB[k * LD + i] = B[k][i], zeros for n <= i < NP
  double* sBT = sB + NP * LD;                                      // sBT[k * LD + j] = B[j][k], zeros for n <= j < NP
  double* sV = sBT + NP * LD;                                      // [G][VR][VS]; long form: [G][NP][NP]
  double* sU = sV + G * VR * VS;                                   // [2][G][VS]
  double* sX = sU + 2 * G * VS;                                    // [2][G][VS]
  double* sW = sX + 2 * G * VS;                                    // [VR]: one (model, item) a workgroup at a time
  const int tid = threadIdx.x, g = tid / NP, a = tid % NP;
  const int k = blockIdx.y;
  const int j_begin = blockIdx.x * TMW_WALK, j_end = min(count, j_begin + TMW_WALK);
  const size_t Ev = (size_t)p.Kc * p.Sc, nn = (size_t)n * n;
  const int cols = n * n;
  const double mu = q.mu[k];
  const bool still = !(mu > 0.0);                                  // the model leaves no state: P = I
  const double* __restrict__ Qk = q.Q + (size_t)k * nn;
  tmw_stage_b<NP, THREADS>(sB, sBT, q.B + (size_t)k * nn, n);
  double* V = sV + (size_t)g * VR * VS;
  double* A = V;                                                   // A[k * NP + j] = A_m[k][j]; lane j touches column j alone
  for (int w = 0; w < TMW_SITES; ++w) {
    const int sb = (blockIdx.z * TMW_SITES + w) * G;               // uniform over the workgroup
    if (sb >= p.Sc) break;
    const int s = sb + g;
    const bool on = s < p.Sc;                                      // a group past the last site repeats site sb and stores nothing
    const size_t ev = (size_t)k * p.Sc + (on ? s : sb);
    const double lam = p.lam[ev];
    const int e_root = p.sL[(size_t)p.root * Ev + ev];
    // an item's vectors and exponents are loaded while the item before it is computed
    double u0n = tp.a[((size_t)j_begin * Ev + ev) * NP + a];
    double v0n = tp.beta[((size_t)j_begin * Ev + ev) * NP + a];
    int eFn = tp.sa[(size_t)j_begin * Ev + ev], eLn = tp.sbeta[(size_t)j_begin * Ev + ev];
    for (int j = j_begin; j < j_end; ++j) {
      const double t = tp.items[j].h;                              // uniform over the workgroup
      const double u0 = u0n, v0 = v0n;
      const int eF = eFn, eL = eLn;
      if (j + 1 < j_end) {
        u0n = tp.a[((size_t)(j + 1) * Ev + ev) * NP + a];
        v0n = tp.beta[((size_t)(j + 1) * Ev + ev) * NP + a];
        eFn = tp.sa[(size_t)(j + 1) * Ev + ev];
        eLn = tp.sbeta[(size_t)(j + 1) * Ev + ev];
      }
      const double x = still ? 0.0 : mu * t;
      // sw_form_terms' word from (mu_k, h): the same in every lane of the workgroup, so the loops below that hold a barrier turn
      // as often in every group
      const int M = tmw_form_terms(x, SW_M_CAP);
      double r = still ? t : x;                                    // mu = 0: the one weight h, the sum 1 and no division by mu
      double S = still ? 1.0 : 1.0 + x;
      double I[NP];
      __syncthreads();                                             // B is staged; the last item's vectors are read
      if (M <= SW_M_CAP) {
        V[a] = v0;
        sU[g * VS + a] = u0;
        if (tid == 0) sW[0] = r;
        for (int m = 0; m < M; ++m) {
          r = r * (x / (double)(m + 2));
          S += r;
          if (tid == 0) sW[m + 1] = r;
        }
        __syncthreads();
        // a barrier a turn: M depends on (model, item) alone
        for (int rr = 0; rr < M; ++rr) {                           // v_{r+1} = B v_r
          double nv = 0.0;
#pragma unroll 8
          for (int jj = 0; jj < n; ++jj) nv = fma(sBT[jj * LD + a], V[rr * VS + jj], nv);
          V[(rr + 1) * VS + a] = nv;
          __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) I[i] = 0.0;
        // a barrier a turn: M depends on (model, item) alone
        for (int l = 0; l <= M; ++l) {
          double gl = 0.0;
#pragma unroll 8
          for (int rr = 0; rr <= M - l; ++rr) gl = fma(sW[l + rr], V[rr * VS + a], gl);
          const double* u = sU + ((l & 1) * G + g) * VS;
#pragma unroll
          for (int i = 0; i < NP; ++i) I[i] = fma(u[i], gl, I[i]);
          if (l < M) {                                             // u_{l+1} = B^T u_l
            double nu = 0.0;
#pragma unroll 8
            for (int kk = 0; kk < n; ++kk) nu = fma(sB[kk * LD + a], u[kk], nu);
            sU[(((l + 1) & 1) * G + g) * VS + a] = nu;
          }
          __syncthreads();
        }
      } else {
        sU[g * VS + a] = u0;
        sX[g * VS + a] = v0;
        __syncthreads();
        const double* u = sU + g * VS;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const double av = u[i] * v0;
          A[i * NP + a] = av;
          I[i] = r * av;
        }
        int cur = 0;
        // a barrier a turn: the trip count depends on x = mu_k h alone, that is on (model, item)
        for (int m = 0; m < SC_M_CAP; ++m) {
          const double rn = r * (x / (double)(m + 2));
          // past the mode (x < m + 2) the terms fall at least geometrically: sum_{j > m} r_j <= r_{m+1} / (1 - x / (m + 3))
          if (x < (double)(m + 2) && rn <= 0x1p-60 * S * (1.0 - x / (double)(m + 3))) break;
          double nv = 0.0;
#pragma unroll 8
          for (int kk = 0; kk < n; ++kk) nv = fma(sBT[kk * LD + a], sX[(cur * G + g) * VS + kk], nv);
          sX[((cur ^ 1) * G + g) * VS + a] = nv;
          double tc[NP];
#pragma unroll
          for (int i = 0; i < NP; ++i) tc[i] = u[i] * nv;
          for (int kk = 0; kk < n; ++kk) {
            const double ak = A[kk * NP + a];
#pragma unroll
            for (int i = 0; i < NP; ++i) tc[i] = fma(sB[kk * LD + i], ak, tc[i]);
          }
          r = rn;
          S += r;
#pragma unroll
          for (int i = 0; i < NP; ++i) {
            A[i * NP + a] = tc[i];
            I[i] = fma(r, tc[i], I[i]);
          }
          if (r > 0x1p512) {
            r *= 0x1p-512;
            S *= 0x1p-512;
#pragma unroll
            for (int i = 0; i < NP; ++i) I[i] *= 0x1p-512;
          }
          cur ^= 1;
          __syncthreads();
        }
      }
      if (on && a < n) {
        const double inv = 1.0 / (still ? S : S * mu);
        const double f = ldexp(1.0 / lam, eF + eL - e_root);
        // Nothing in Q's column depends on the item, so the compiler would lift its n loads out of the walk's loop and hold them
        // in registers through every item (128 registers at 64 states).  A zero it cannot see through keeps them here.
        int z = 0;
        asm volatile("" : "+v"(z));
        const double* __restrict__ Qz = Qk + z;
        double* oz = tp.rows + ((size_t)j * Ev + ev) * cols;                 // the item's own row: nothing is added
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          if (i < n) oz[i == a ? i : count_col(n, i, a)] = i == a ? (I[i] * inv) * f : (Qz[(size_t)i * n + a] * (I[i] * inv)) * f;
        }
      }
    }
  }
}

// grid: (cells / 256, ranges of the launch).  A dependent chain over the range's items in order, continued from tot across
// launches, so the sum does not depend on how the items were chunked.
__global__ __launch_bounds__(TMW_SUM_BLOCK) void tmw_range_sum_kernel(const double* __restrict__ x, int64_t cells, int count, int64_t q0,
                                                                      const int64_t* __restrict__ off, int r0, double* __restrict__ tot) {
  const int64_t c = (int64_t)blockIdx.x * TMW_SUM_BLOCK + threadIdx.x;
  if (c >= cells) return;
  const int r = r0 + blockIdx.y;
  const int64_t lo = max(off[r], q0), hi = min(off[r + 1], q0 + (int64_t)count);
  if (lo >= hi) return;
  double* t = tot + (int64_t)r * cells + c;
  double acc = *t;
  for (int64_t j = lo; j < hi; ++j) acc += x[(j - q0) * cells + c];
  *t = acc;
}

inline bool tmw_ok(const TmwParams& tp, int count) {
  const ScwParams& q = tp.sc;
  const AwParams& p = q.aw;
  return p.n >= AW_MIN_STATES && p.n <= EX_MAX_STATES && p.NP == aw_lanes(p.n) && p.Kc >= 1 && p.Kc <= AW_GRID_MAX && p.Sc >= 1 &&
         p.Sc <= AW_GRID_MAX && (size_t)p.Kc * p.Sc <= (size_t)INT32_MAX && p.root >= p.n_tips && p.n_edge >= 1 && p.P && p.L && p.sL &&
         p.F && p.sF && p.lam && q.Q && q.t && q.child && q.mu && q.B && tp.items && count <= TM_GRID_MAX;
}

template <int NP> inline int tmw_tiles(const AwParams& p) { return (p.Sc + TmwShape<NP>::G * TMW_SITES - 1) / (TmwShape<NP>::G * TMW_SITES); }

template <int NP>
hipError_t tmw_along(const TmwParams& p, int count, hipStream_t stream) {
  constexpr size_t lds = sizeof(double) * TmwShape<NP>::along_doubles;
  const hipError_t e = aw_allow_lds(reinterpret_cast<const void*>(tmw_along_kernel<NP>), (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((tmw_along_kernel<NP>), dim3((count + TMW_WALK - 1) / TMW_WALK, p.sc.aw.Kc, tmw_tiles<NP>(p.sc.aw)),
                     dim3(TmwShape<NP>::threads), lds, stream, p, count);
  return hipGetLastError();
}

template <int NP>
hipError_t tmw_branch(const TmwParams& p, int count, hipStream_t stream) {
  constexpr size_t lds = sizeof(double) * TmwShape<NP>::branch_doubles;
  const hipError_t e = aw_allow_lds(reinterpret_cast<const void*>(tmw_branch_kernel<NP>), (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((tmw_branch_kernel<NP>), dim3((count + TMW_WALK - 1) / TMW_WALK, p.sc.aw.Kc, tmw_tiles<NP>(p.sc.aw)),
                     dim3(TmwShape<NP>::threads), lds, stream, p, count);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_tmw_along(const TmwParams& p, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!tmw_ok(p, count) || (!p.post && (!p.a || !p.sa || !p.beta || !p.sbeta))) return hipErrorInvalidValue;
  return aw_with_lanes(p.sc.aw.NP, [&](auto np) { return tmw_along<decltype(np)::value>(p, count, stream); });
}

hipError_t launch_tmw_branch(const TmwParams& p, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!tmw_ok(p, count) || !p.a || !p.sa || !p.beta || !p.sbeta || !p.rows) return hipErrorInvalidValue;
  return aw_with_lanes(p.sc.aw.NP, [&](auto np) { return tmw_branch<decltype(np)::value>(p, count, stream); });
}

hipError_t launch_tmw_range_sum(const double* x, int64_t cells, int count, int64_t q0, const int64_t* off, int r_begin, int r_end,
                                int n_ranges, double* tot, hipStream_t stream) {
  if (count <= 0 || r_end <= r_begin) return hipSuccess;
  const int64_t gx = (cells + TMW_SUM_BLOCK - 1) / TMW_SUM_BLOCK;
  if (!x || !off || !tot || cells < 1 || gx > (int64_t)INT32_MAX || r_begin < 0 || r_end > n_ranges) return hipErrorInvalidValue;
  for (int r0 = r_begin; r0 < r_end; r0 += AW_GRID_MAX)
    hipLaunchKernelGGL(tmw_range_sum_kernel, dim3((unsigned)gx, std::min(AW_GRID_MAX, r_end - r0)), dim3(TMW_SUM_BLOCK), 0, stream, x, cells,
                       count, q0, off, r0, tot);
  return hipGetLastError();
}

}  // namespace phm
