// phm_sample_branch.h -- the one branch draw of the two exact samplers of histories: the categorical draw,
// the jump count of a branch (the two-pass series with the inline stopping rule and the 2^512 rescaling, section 19) and the
// jump times with the walk over the states.  phm_sample.hip (2..8 states, model-fastest buffers) and phm_sample_wide.hip (9..64
// states, a model's table contiguous, B in LDS) differ only in where B and beta live: each kernel builds an SmTable and calls the
// two functions.  They stay two, because the wide kernel stages B between them.  Every sum and product is written out left to
// right (the library is built with -ffp-contract=off): a change here changes both state ranges alike.
#pragma once

#include <type_traits>

#include "phm_device.h"
#include "phm_sample.h"

namespace phm {

// first j with u * sum(w) <= w_0 + .. + w_j, w_c = a[c sa] * b[c sb], sums left to right (section 2's rule)
template <int NS>
__device__ __forceinline__ int sm_draw(const double* __restrict__ a, size_t sa, const double* __restrict__ b, size_t sb, int n,
                                       double u, uint32_t& err) {
  if constexpr (NS > 0) {
    double w[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) w[c] = a[c * sa] * b[c * sb];
    return sample_cat<NS>(w, u, err);
  } else {
    double total = a[0] * b[0];
    for (int c = 1; c < n; ++c) total += a[c * sa] * b[c * sb];
    if (!(total > 0.0) || isinf(total)) err |= DERR_ZERO_PROB;
    const double thr = u * total;
    double cum = a[0] * b[0];
    int idx = (thr <= cum) ? 0 : 1;
    for (int c = 1; c < n - 1; ++c) { cum += a[c * sa] * b[c * sb]; idx += (thr <= cum) ? 0 : 1; }
    return idx;
  }
}

// Where one model's B and table live.  B[c, j] at B[c B_row + j B_col]; (B^m)[c, e] at beta[m beta_m + c beta_c + e beta_e], beta
// with the model's offset applied.  U: the type of B_col and beta_c, size_t or SmUnit, the literal 1 (the wide layout: rows of B
// and the n weights beta_m[., e] of a state draw contiguous), with which the addressing folds as if written with no stride at all.
using SmUnit = std::integral_constant<size_t, 1>;
template <typename U>
struct SmTable {
  const double* B;  size_t B_row;  U B_col;
  const double* beta;  size_t beta_m;  U beta_c;  size_t beta_e;
};

// The jump count N of a branch a -> e with x = mu t > 0: the first m with u S <= cum_m.  sr: the branch's stream, opened; draw 0.
template <typename U>
__device__ __forceinline__ int sm_jump_count(const SmTable<U>& tab, int a, int e, double x, int depth, Stream& sr, uint32_t& err) {
  const double* __restrict__ ba = tab.beta + a * tab.beta_c + e * tab.beta_e;      // beta_m[a, e] at ba[m beta_m]
  // first pass: the stopping index and the series' own total
  double r = 1.0, Sp = 1.0, Sa = ba[0];
  int R = 0, M = 0;
  for (int m = 1;; ++m) {
    const double rn = r * (x / (double)m);
    if (m >= 2 && x < (double)m && rn <= 0x1p-60 * Sp * (1.0 - x / (double)(m + 1))) break;
    if (m > depth) { err |= DERR_CAPACITY; break; }                // never with the host's depth: M is monotone in x
    r = rn;
    Sp += r;
    Sa += r * ba[m * tab.beta_m];
    M = m;
    if (r > 0x1p512) { r *= 0x1p-512; Sp *= 0x1p-512; Sa *= 0x1p-512; ++R; }
  }
  if (!(Sa > 0.0) || isinf(Sa)) err |= DERR_ZERO_PROB;
  const double thr = sr.draw(0) * Sa;
  // second pass: the first m whose partial sum reaches the threshold
  double cum = ba[0];
  int rho = 0;
  r = 1.0;
  if (thr <= ldexp(cum, -512 * R)) return 0;
  for (int m = 1; m <= M; ++m) {
    r = r * (x / (double)m);
    cum += r * ba[m * tab.beta_m];
    if (r > 0x1p512) { r *= 0x1p-512; cum *= 0x1p-512; ++rho; }
    if (thr <= ldexp(cum, -512 * (R - rho))) return m;
  }
  return M;
}

// The history of a branch a -> e of length tb with N jumps (0: mu = 0, t = 0 or none drawn: the parent's state throughout):
// jump times T_i = tb (c_i / G) from the exponential draws 1 .. N + 1 of sr, taken twice (G first, then the walk); states x_i
// from draws N + 1 + i with weights B[x_{i-1}, .] beta_{N-i}[., e]; equal neighbours merge.  segment(state, dwell) and
// count(from, to) receive the result in order.  ltab: neglog_u32's table in LDS.
template <int NS, typename U, typename Segment, typename Count>
__device__ __forceinline__ void sm_walk(const SmTable<U>& tab, int n, int a, int e, double tb, int N, Stream& sr,
                                        const double* ltab, uint32_t& err, Segment&& segment, Count&& count) {
  if (N <= 0) { segment(a, tb); return; }
  double G = 0.0;
  for (int i = 1; i <= N + 1; ++i) G += neglog_u32(sr.draw_word((uint32_t)i), ltab);
  Stream su;
  su.open(sr.ent, sr.iter, sr.rep, sr.k0, sr.k1);
  int prev = a, sprev = a;
  double tprev = 0.0, c = 0.0;
  for (int i = 1; i <= N; ++i) {
    c += neglog_u32(sr.draw_word((uint32_t)i), ltab);
    int di = e;
    if (i < N) {
      const double u = su.draw((uint32_t)(N + 1 + i));
      di = sm_draw<NS>(tab.B + prev * tab.B_row, tab.B_col, tab.beta + (size_t)(N - i) * tab.beta_m + e * tab.beta_e, tab.beta_c, n,
                       u, err);
    }
    if (prev != di) {
      const double ti = tb * (c / G);
      segment(sprev, ti - tprev);
      count(sprev, di);
      tprev = ti; sprev = di;
    }
    prev = di;
  }
  segment(sprev, tb - tprev);
}

}  // namespace phm
