// phm_branch_rows_wide.hip -- E[dwell_i | tips_s, Q_k] and E[N_ij | tips_s, Q_k] PER BRANCH for many rate matrices at 9..64
// states: section 26's branch stage with the rows kept, on top of section 23's P_k(t_b), up pass, root and
// down pass and section 26's model kernel, all launched unchanged.
//
// The mapping is scw_branch_kernel's: one state per lane in groups of NP lanes (16 / 32 / 64), a workgroup per (BRW_WALK
// consecutive entries of the selected list, model, tile of sites), B_k staged once per workgroup, row-major and transposed; its
// groups walk SCW_WALK sites each and, per site, the entries.  Where that kernel adds an edge's row into its run's row this one
// stores it: rows[entry of the launch][ev][col].  The per-item body -- both forms, the weights, the stopping rule, the rescaling
// by 2^-512, inv and f -- is scw_branch_kernel's, RESTATED here operation for operation (that kernel stays as it is; see
// phm_branch_rows.hip), and tests/test_gpu_branch_rows.py holds the two to the same bits.  Which form an item takes is the
// host's word form[model][edge] (sw_form_terms), so a workgroup never diverges over it.
// Every loop is bounded by n, M <= SW_M_CAP, SC_M_CAP, the walk or the site tile.
#include "phm_branch_rows_wide.h"

#include "phm_aw_device.h"

#include <algorithm>

namespace phm {

namespace {

constexpr int BRW_WALK = SC_RUN;               // consecutive entries of the selected list a workgroup walks through the staged matrices
constexpr int BRW_SITES = 4;                   // sites a group walks (SCW_WALK)

// scw_branch_kernel's shape: few groups per workgroup, LDS holds SW_M_CAP + 1 vectors a group
template <int NP> struct BrwBranch {
  static constexpr int G = NP == 16 ? 4 : 2;
  static constexpr int threads = G * NP;       // 64, 64, 128
  static constexpr int LD = AwShape<NP>::LD;
  static constexpr int VS = AwShape<NP>::VS;
  static constexpr int VR = SW_M_CAP + 1;      // rows of a group's V
  // B, B^T; V (A_m of the long form in its place); u ping-pong, the long form's v ping-pong; the weights
  static constexpr size_t lds_doubles = (size_t)2 * NP * LD + (size_t)G * VR * VS + (size_t)4 * G * VS + VR;
  static_assert(NP * NP <= VR * VS, "A_m of the long form lives in a group's V");
};

// grid: (walks of the launch's entries, model, site tile)
template <int NP>
__global__ __launch_bounds__(BrwBranch<NP>::threads) void brw_branch_kernel(ScwParams q, const int32_t* __restrict__ sel, int count,
                                                                           double* __restrict__ rows) {
  using Sh = BrwBranch<NP>;
  constexpr int G = Sh::G, LD = Sh::LD, VS = Sh::VS, VR = Sh::VR, THREADS = Sh::threads;
  extern __shared__ __align__(16) double brw_lds[];
  const AwParams& p = q.aw;
  const int n = p.n;
  double* sB = brw_lds;                                            // sB[k * LD + i] = B[k][i], zeros for n <= i < NP
  double* sBT = sB + NP * LD;                                      // sBT[k * LD + j] = B[j][k], zeros for n <= j < NP
  double* sV = sBT + NP * LD;                                      // [G][VR][VS]; long form: [G][NP][NP]
  double* sU = sV + G * VR * VS;                                   // [2][G][VS]
  double* sX = sU + 2 * G * VS;                                    // [2][G][VS]
  double* sW = sX + 2 * G * VS;                                    // [VR]: one (model, edge) a workgroup at a time
  const int tid = threadIdx.x, g = tid / NP, a = tid % NP;
  const int k = blockIdx.y;
  const int j_begin = blockIdx.x * BRW_WALK, j_end = min(count, j_begin + BRW_WALK);
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
  for (int w = 0; w < BRW_SITES; ++w) {
    const int sb = (blockIdx.z * BRW_SITES + w) * G;               // uniform over the workgroup
    if (sb >= p.Sc) break;
    const int s = sb + g;
    const bool on = s < p.Sc;                                      // a group past the last site repeats site sb and stores nothing
    const size_t ev = (size_t)k * p.Sc + (on ? s : sb);
    const double lam = p.lam[ev];
    const int e_root = p.sL[(size_t)p.root * Ev + ev];
    // an item's vectors and exponents are loaded while the item before it is computed
    int bn = sel[j_begin];
    double u0n = p.F[((size_t)bn * Ev + ev) * NP + a];
    double v0n = p.L[((size_t)q.child[bn] * Ev + ev) * NP + a];
    int eFn = p.sF[(size_t)bn * Ev + ev], eLn = p.sL[(size_t)q.child[bn] * Ev + ev];
    for (int j = j_begin; j < j_end; ++j) {
      const int b = bn;
      const int M = q.form[(size_t)k * p.n_edge + b];              // uniform over the workgroup
      const double t = q.t[b];
      const double u0 = u0n, v0 = v0n;
      const int eF = eFn, eL = eLn;
      if (j + 1 < j_end) {
        bn = sel[j + 1];
        const int cn = q.child[bn];
        u0n = p.F[((size_t)bn * Ev + ev) * NP + a];
        v0n = p.L[((size_t)cn * Ev + ev) * NP + a];
        eFn = p.sF[(size_t)bn * Ev + ev];
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
          for (int jj = 0; jj < n; ++jj) nv = fma(sBT[jj * LD + a], V[rr * VS + jj], nv);
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
        // Nothing in Q's column depends on the entry, so the compiler would lift its n loads out of the walk's loop and hold them
        // in registers through every item (128 registers at 64 states).  A zero it cannot see through keeps them here.
        int z = 0;
        asm volatile("" : "+v"(z));
        const double* __restrict__ Qz = Qk + z;
        double* oz = rows + ((size_t)j * Ev + ev) * cols;                    // the entry's own row: nothing is added
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          if (i < n) oz[i == a ? i : count_col(n, i, a)] = i == a ? (I[i] * inv) * f : (Qz[(size_t)i * n + a] * (I[i] * inv)) * f;
        }
      }
    }
  }
}

inline bool brw_ok(const ScwParams& q) {
  const AwParams& p = q.aw;
  return p.n >= AW_MIN_STATES && p.n <= EX_MAX_STATES && p.NP == aw_lanes(p.n) && p.Kc >= 1 && p.Kc <= AW_GRID_MAX && p.Sc >= 1 &&
         p.Sc <= AW_GRID_MAX && p.root >= p.n_tips && p.L && p.sL && p.F && p.sF && p.lam && q.Q && q.t && q.child && q.mu && q.B &&
         q.form;
}

template <int NP>
hipError_t brw_branch(const ScwParams& q, const int32_t* sel, int count, double* rows, hipStream_t stream) {
  const AwParams& p = q.aw;
  constexpr size_t lds = sizeof(double) * BrwBranch<NP>::lds_doubles;
  const hipError_t e = aw_allow_lds(reinterpret_cast<const void*>(brw_branch_kernel<NP>), (int)lds);
  if (e != hipSuccess) return e;
  const int tiles = (p.Sc + BrwBranch<NP>::G * BRW_SITES - 1) / (BrwBranch<NP>::G * BRW_SITES);
  hipLaunchKernelGGL((brw_branch_kernel<NP>), dim3((count + BRW_WALK - 1) / BRW_WALK, p.Kc, tiles), dim3(BrwBranch<NP>::threads), lds,
                     stream, q, sel, count, rows);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_brw_branch(const ScwParams& q, const int32_t* sel, int count, double* rows, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!brw_ok(q) || !sel || !rows) return hipErrorInvalidValue;
  return aw_with_lanes(q.aw.NP, [&](auto np) { return brw_branch<decltype(np)::value>(q, sel, count, rows, stream); });
}

}  // namespace phm
