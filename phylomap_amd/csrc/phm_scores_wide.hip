// phm_scores_wide.hip -- E[dwell_i | tips_s, Q_k] and E[N_ij | tips_s, Q_k] for many rate matrices at 9..64 states (DESIGN.md
// section 26): section 18's branch stage and run totals in section 23's mapping, ONE STATE PER LANE, on top of section 23's
// P_k(t_b), up pass, root and down pass (phm_ancestral_wide.hip: log p(tips | Q_k) is phm_loglik_models' value bit for bit; the
// root stores lam = pid_k . L_root and the down pass F_b with its exponent, AwParams' lam, F and sF).
//
// A group of NP lanes (16 / 32 / 64 for 9..16 / 17..32 / 33..64 states) owns an item; lane a holds state a, the lanes past n hold
// zeros.  An evaluation of a chunk is ev = model * Sc + site; vectors are rows of NP doubles, exponents int32.
//   * branch stage, a workgroup per (run of SC_RUN edge rows, model, tile of sites): B_k staged once, row-major and transposed,
//     rows NP + 1 doubles apart; its groups walk SCW_WALK sites each and, per site, the edge rows of the run in edge order.
//     I_b = sum_{l + r <= M} w_{l+r} u_l v_r^T with u_l = (B^T)^l F_b, v_r = B^r L_c; lane j owns column j of I in registers.
//     Weights and stopping rule are section 18's: r_0 = x = mu_k t_b, r_{m+1} = r_m x / (m + 2), S = 1 + sum r_m, the sum divided
//     by S mu at the end; mu_k = 0: the one weight t_b, S = 1, no division by mu.
//       short form (M <= SW_M_CAP, M from the host's word): v_0 .. v_M by M mat-vecs into LDS (lane a runs the fma chain over
//       B's row a), then for l = 0 .. M: g_l = sum_{r <= M - l} w_{l+r} v_r (lane j its own component, r ascending),
//       I[i][j] = fma(u_l[i], g_l[j], I[i][j]) and u_{l+1} = B^T u_l.  O(M n + M^2 / 2) multiply-adds per lane.
//       long form (the rest): ex_branch_wide_kernel's recursion A_{m+1} = B^T A_m + u_0 v_{m+1}^T, I += r_m A_m with the running
//       weights and section 18's rescaling by 2^-512; A_m lives where the short form keeps v_r.  Hard end: SC_M_CAP.
//     Which form an item takes depends on (model, edge) alone, so a workgroup never diverges over it.
//   * the sum over the branches is taken in a fixed order: a lane adds the edge rows of its run in edge order into the run's row,
//     scw_total_kernel adds the run totals in run order.  Nothing at run time enters the grouping.
// LDS holds few workgroups a CU (one wave a SIMD at most), so nothing hides an LDS read's latency but the wave's own
// independent reads: the chains over j are unrolled by 8 (their fma order is unchanged).
// Every loop is bounded by n, M <= SW_M_CAP, SC_M_CAP, the run or the site tile.
#include "phm_scores_wide.h"

#include "phm_aw_device.h"

#include <algorithm>

namespace phm {

namespace {

constexpr int SCW_BLOCK = 256;                 // model and total kernels
constexpr int SCW_WALK = 4;                    // sites a group walks through the staged matrices

// branch stage: few groups per workgroup, because a fit calls with one site or a few and LDS holds SW_M_CAP + 1 vectors a group
template <int NP> struct ScwBranch {
  static constexpr int G = NP == 16 ? 4 : 2;
  static constexpr int threads = G * NP;       // 64, 64, 128
  static constexpr int LD = AwShape<NP>::LD;
  static constexpr int VS = AwShape<NP>::VS;
  static constexpr int VR = SW_M_CAP + 1;      // rows of a group's V
  // B, B^T; V (A_m of the long form in its place); u ping-pong, the long form's v ping-pong; the weights
  static constexpr size_t lds_doubles = (size_t)2 * NP * LD + (size_t)G * VR * VS + (size_t)4 * G * VS + VR;
  static_assert(NP * NP <= VR * VS, "A_m of the long form lives in a group's V");
};

// grid: (model).  sc_model_kernel's values.
__global__ __launch_bounds__(SCW_BLOCK) void scw_model_kernel(ScwParams q) {
  const int n = q.aw.n, k = blockIdx.x;
  const size_t nn = (size_t)n * n;
  const double* __restrict__ Qk = q.Q + (size_t)k * nn;
  const double mu = model_mu(Qk, 1, n);
  if (threadIdx.x == 0) q.mu[k] = mu;
  for (int e = threadIdx.x; e < n * n; e += SCW_BLOCK) q.B[(size_t)k * nn + e] = model_b(Qk[e], mu, e / n == e % n ? 1.0 : 0.0);
}


// grid: (run, model, site tile)
template <int NP>
__global__ __launch_bounds__(ScwBranch<NP>::threads) void scw_branch_kernel(ScwParams q, int r0) {
  using Sh = ScwBranch<NP>;
  constexpr int G = Sh::G, LD = Sh::LD, VS = Sh::VS, VR = Sh::VR, THREADS = Sh::threads;
  extern __shared__ __align__(16) double scw_lds[];
  const AwParams& p = q.aw;
  const int n = p.n;
  double* sB = scw_lds;                                            // sB[k * LD + i] = B[k][i], zeros for n <= i < NP
  double* sBT = sB + NP * LD;                                      // sBT[k * LD + j] = B[j][k], zeros for n <= j < NP
  double* sV = sBT + NP * LD;                                      // [G][VR][VS]; long form: [G][NP][NP]
  double* sU = sV + G * VR * VS;                                   // [2][G][VS]
  double* sX = sU + 2 * G * VS;                                    // [2][G][VS]
  double* sW = sX + 2 * G * VS;                                    // [VR]: one (model, edge) a workgroup at a time
  const int tid = threadIdx.x, g = tid / NP, a = tid % NP;
  const int k = blockIdx.y;
  const int b_begin = (r0 + blockIdx.x) * SC_RUN, b_end = min(p.n_edge, b_begin + SC_RUN);
  const size_t Ev = (size_t)p.Kc * p.Sc, nn = (size_t)n * n;
  const int cols = n * n;
  const double mu = q.mu[k];
  const bool still = !(mu > 0.0);                                  // the model leaves no state: P = I
  const double* __restrict__ Qk = q.Q + (size_t)k * nn;
  {
    const double* __restrict__ Bk = q.B + (size_t)k * nn;
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
  double* V = sV + (size_t)g * VR * VS;
  double* A = V;                                                   // A[k * NP + j] = A_m[k][j]; lane j touches column j alone
  for (int w = 0; w < SCW_WALK; ++w) {
    const int sb = (blockIdx.z * SCW_WALK + w) * G;                // uniform over the workgroup
    if (sb >= p.Sc) break;
    const int s = sb + g;
    const bool on = s < p.Sc;                                      // a group past the last site repeats site sb and stores nothing
    const size_t ev = (size_t)k * p.Sc + (on ? s : sb);
    const double lam = p.lam[ev];
    const int e_root = p.sL[(size_t)p.root * Ev + ev];
    double* out = q.runs + ((size_t)blockIdx.x * Ev + ev) * cols;
    // an item's vectors and exponents are loaded while the item before it is computed
    double u0n = p.F[((size_t)b_begin * Ev + ev) * NP + a];
    double v0n = p.L[((size_t)q.child[b_begin] * Ev + ev) * NP + a];
    int eFn = p.sF[(size_t)b_begin * Ev + ev], eLn = p.sL[(size_t)q.child[b_begin] * Ev + ev];
    for (int b = b_begin; b < b_end; ++b) {
      const int M = q.form[(size_t)k * p.n_edge + b];              // uniform over the workgroup
      const double t = q.t[b];
      const double u0 = u0n, v0 = v0n;
      const int eF = eFn, eL = eLn;
      if (b + 1 < b_end) {
        const int cn = q.child[b + 1];
        u0n = p.F[((size_t)(b + 1) * Ev + ev) * NP + a];
        v0n = p.L[((size_t)cn * Ev + ev) * NP + a];
        eFn = p.sF[(size_t)(b + 1) * Ev + ev];
        eLn = p.sL[(size_t)cn * Ev + ev];
      }
      const double x = still ? 0.0 : mu * t;
      double r = still ? t : x;                                    // mu = 0: the one weight t_b, the sum 1 and no division by mu
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
        for (int rr = 0; rr < M; ++rr) {                           // v_{r+1} = B v_r
          double nv = 0.0;
#pragma unroll 8
          for (int j = 0; j < n; ++j) nv = fma(sBT[j * LD + a], V[rr * VS + j], nv);
          V[(rr + 1) * VS + a] = nv;
          __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) I[i] = 0.0;
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
        // Nothing below depends on the edge row, so the compiler would lift the n loads of Q's column and the n cell addresses out
        // of the run's loop and hold them in registers through every item (128 + 128 registers at 64 states).  A zero it cannot
        // see through keeps them here.
        int z = 0;
        asm volatile("" : "+v"(z));
        const double* __restrict__ Qz = Qk + z;
        double* oz = out + z;
        // the run's row so far is read 16 cells at a time in one batch (a lane alone touches its cells), then written back with
        // this edge row added: one round trip to memory per 16 cells, not one per cell
#pragma unroll
        for (int i0 = 0; i0 < NP; i0 += 16) {
          double prev[16];
#pragma unroll
          for (int i = i0; i < i0 + 16; ++i) prev[i - i0] = (i < n && b != b_begin) ? oz[i == a ? i : count_col(n, i, a)] : 0.0;
#pragma unroll
          for (int i = i0; i < i0 + 16; ++i) {
            if (i < n) {
              const double val = i == a ? (I[i] * inv) * f : (Qz[(size_t)i * n + a] * (I[i] * inv)) * f;
              oz[i == a ? i : count_col(n, i, a)] = prev[i - i0] + val;
            }
          }
        }
      }
    }
  }
}

// one lane per (evaluation, column)
__global__ __launch_bounds__(SCW_BLOCK) void scw_total_kernel(ScwParams q, int count) {
  const AwParams& p = q.aw;
  const size_t cells = (size_t)p.Kc * p.Sc * p.n * p.n;
  const size_t at = (size_t)blockIdx.x * SCW_BLOCK + threadIdx.x;
  if (at >= cells) return;
  double acc = q.tot[at];
  for (int r = 0; r < count; ++r) acc += q.runs[(size_t)r * cells + at];
  q.tot[at] = acc;
}

inline bool scw_ok(const ScwParams& q) {
  const AwParams& p = q.aw;
  return p.n >= AW_MIN_STATES && p.n <= EX_MAX_STATES && p.NP == aw_lanes(p.n) && p.Kc >= 1 && p.Kc <= AW_GRID_MAX && p.Sc >= 1 &&
         p.Sc <= AW_GRID_MAX && (size_t)p.Kc * p.Sc * p.n * p.n <= (size_t)INT32_MAX && p.root >= p.n_tips && p.P && p.pid && p.L &&
         p.sL && p.O && p.sO && p.F && p.sF && p.lam && q.Q && q.t && q.child && q.mu && q.B && q.form && q.runs && q.tot;
}

template <int NP> inline int scw_branch_tiles(const AwParams& p) { return (p.Sc + ScwBranch<NP>::G * SCW_WALK - 1) / (ScwBranch<NP>::G * SCW_WALK); }

template <int NP>
hipError_t scw_branch(const ScwParams& q, int r0, int count, hipStream_t stream) {
  const AwParams& p = q.aw;
  constexpr size_t lds = sizeof(double) * ScwBranch<NP>::lds_doubles;
  const hipError_t e = aw_allow_lds(reinterpret_cast<const void*>(scw_branch_kernel<NP>), (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((scw_branch_kernel<NP>), dim3(count, p.Kc, scw_branch_tiles<NP>(p)), dim3(ScwBranch<NP>::threads), lds, stream, q, r0);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_scw_model(const ScwParams& q, hipStream_t stream) {
  if (!scw_ok(q)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scw_model_kernel, dim3(q.aw.Kc), dim3(SCW_BLOCK), 0, stream, q);
  return hipGetLastError();
}

hipError_t launch_scw_branch(const ScwParams& q, int r0, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  const int n_runs = (q.aw.n_edge + SC_RUN - 1) / SC_RUN;
  if (!scw_ok(q) || count > AW_GRID_MAX || r0 < 0 || r0 + count > n_runs) return hipErrorInvalidValue;
  return aw_with_lanes(q.aw.NP, [&](auto np) { return scw_branch<decltype(np)::value>(q, r0, count, stream); });
}

hipError_t launch_scw_total(const ScwParams& q, int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!scw_ok(q)) return hipErrorInvalidValue;
  const size_t cells = (size_t)q.aw.Kc * q.aw.Sc * q.aw.n * q.aw.n;
  hipLaunchKernelGGL(scw_total_kernel, dim3((unsigned)((cells + SCW_BLOCK - 1) / SCW_BLOCK)), dim3(SCW_BLOCK), 0, stream, q, count);
  return hipGetLastError();
}

}  // namespace phm
