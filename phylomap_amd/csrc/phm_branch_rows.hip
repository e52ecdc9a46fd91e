// phm_branch_rows.hip -- E[dwell_i | tips_s, Q_k] and E[N_ij | tips_s, Q_k] PER BRANCH for many rate matrices at 2..8 states
// (DESIGN.md section 27): section 18's branch stage with the rows kept, on top of section 17's P_k(t_b) and up pass and section
// 18's root and down pass, all launched unchanged.
//
// A lane owns one model k, as in phm_scores.hip; a wave takes ONE selected edge row (sc_branch_kernel walks a run of SC_RUN), so
// a small tree fills SC_RUN times the waves.  The per-edge body -- the recursion A_{m+1} = B^T A_m + u_0 v_{m+1}^T, the weights
// r_{m+1} = r_m x / (m + 2), the stopping rule, the rescaling by 2^-512, inv and f -- is sc_branch_kernel's, RESTATED here
// operation for operation: that kernel's code stays as it is (its spelling is pinned, and a shared device function would change
// how it is compiled), and tests/test_gpu_branch_rows.py holds the two to the same bits (the rows added in run order are
// phm_expected_stats_models' totals).  n <= 4: A, I, B, u_0 and v in registers.  5..8 states: B from global memory.
// The row goes to [edge of the launch][col][site][model of the chunk], coalesced along the models.
//
// br_label_kernel reduces finished rows to labelled sums for both families (2..64 states): one lane per (evaluation, row,
// label), the columns in order, a multiply and an add rounded separately (__dmul_rn, __dadd_rn: never contracted), so that plain
// double arithmetic on the host reproduces a labelled value from the full row bit for bit.
// Every loop is bounded by n, SC_M_CAP or the column count.
#include "phm_branch_rows.h"

#include "phm_ll_device.h"

namespace phm {

namespace {

constexpr int BR_BLOCK = 64;                   // branch stage: one wave per block, as SC_BRANCH_BLOCK
constexpr int BR_LABEL_BLOCK = 256;

// grid: (models / 64, selected edges of the launch, sites)
template <int N>
__global__ __launch_bounds__(BR_BLOCK) void br_branch_kernel(ScParams p, const int32_t* __restrict__ sel, double* __restrict__ rows) {
  constexpr bool REG = N <= LL_REG_MAX;
  constexpr int NN = N * N;
  const LlParams& q = p.ll;
  const int k = blockIdx.x * BR_BLOCK + threadIdx.x;
  if (k >= q.Kc) return;
  const size_t Kp = q.Kp, Ev = (size_t)q.n_sites * Kp, ev = (size_t)blockIdx.z * Kp + k;
  const int b = sel[blockIdx.y];                                   // uniform over the wave
  const double mu = p.mu[k];
  const bool still = !(mu > 0.0);                                  // the model leaves no state: P = I
  const double* __restrict__ Qk = q.Q + k;
  const double* __restrict__ Bg = REG ? nullptr : p.B + k;
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
  const double lam = p.lam[ev], e_root = q.sL[(size_t)p.root * Ev + ev];
  // rows hold the chunk's Kc models alone, not the padded lanes: a call of one model copies out 1 lane, not 64
  const size_t Eo = (size_t)q.n_sites * q.Kc;
  double* out = rows + (size_t)blockIdx.y * NN * Eo + (size_t)blockIdx.z * q.Kc + k;   // [col][Eo] of this entry
  const double t = q.t[b];
  const int c = p.child[b];
  double u0[N], v[N], A[N][N], I[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    u0[i] = p.F[((size_t)b * N + i) * Ev + ev];
    v[i] = q.L[((size_t)c * N + i) * Ev + ev];
  }
  const double x = still ? 0.0 : mu * t;
  double r = still ? t : x;                                        // mu = 0: the one weight t_b, the sum 1 and no division by mu
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
      out[(size_t)col * Eo] = i == j ? (I[i][i] * inv) * f : (Qk[(size_t)(i * N + j) * Kp] * (I[i][j] * inv)) * f;
    }
}

// grid: (evaluations / 256, rows of the launch, labels)
__global__ __launch_bounds__(BR_LABEL_BLOCK) void br_label_kernel(BrLabelParams p) {
  const int64_t ev = (int64_t)blockIdx.x * BR_LABEL_BLOCK + threadIdx.x;
  if (ev >= p.n_ev) return;
  const int j = blockIdx.y, l = blockIdx.z;
  const double* __restrict__ row = p.rows + (int64_t)j * p.row_j + ev * p.row_ev;
  const double* __restrict__ w = p.w + (size_t)l * p.cols;
  double acc = 0.0;
  for (int col = 0; col < p.cols; ++col) acc = __dadd_rn(acc, __dmul_rn(w[col], row[(int64_t)col * p.row_col]));
  p.out[((int64_t)j * p.n_labels + l) * p.n_ev + ev] = acc;
}

}  // namespace

hipError_t launch_br_branch(const ScParams& p, const int32_t* sel, int count, double* rows, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (!ll_ok(p.ll) || count > BR_GRID_MAX || !sel || !rows || (p.ll.n > LL_REG_MAX && !p.B)) return hipErrorInvalidValue;
  const dim3 g = model_grid(p.ll, BR_BLOCK, count, p.ll.n_sites);
  ll_with_states(p.ll.n, [&](auto ns) { hipLaunchKernelGGL((br_branch_kernel<decltype(ns)::value>), g, dim3(BR_BLOCK), 0, stream, p, sel, rows); });
  return hipGetLastError();
}

hipError_t launch_br_labels(const BrLabelParams& p, hipStream_t stream) {
  if (p.count <= 0) return hipSuccess;
  if (!p.rows || !p.w || !p.out || p.cols < 1 || p.n_labels < 1 || p.n_labels > BR_MAX_LABELS || p.count > BR_GRID_MAX || p.n_ev < 1 ||
      (p.n_ev + BR_LABEL_BLOCK - 1) / BR_LABEL_BLOCK > (int64_t)INT32_MAX)
    return hipErrorInvalidValue;
  const dim3 g((unsigned)((p.n_ev + BR_LABEL_BLOCK - 1) / BR_LABEL_BLOCK), p.count, p.n_labels);
  hipLaunchKernelGGL(br_label_kernel, g, dim3(BR_LABEL_BLOCK), 0, stream, p);
  return hipGetLastError();
}

}  // namespace phm
