// phm_draw_tab.h -- the categorical draw of a branch's segment states as integer thresholds on the raw random word.
//
// The branch kernel of phm_tiles.hip draws s_i ~ B[s_prev, :] (.) B^kk e_cs with sample_cat(p, u01(x)) (phm_device.h) from the
// 32 random bits x.  For a fixed (kk, cs, s_prev) the products p_c, their total and their running sums cum_j are constants, and
//   u01(x) = (x + 0.5) 2^-32        is exact and increasing in x,
//   thr(x) = RN(u01(x) * total)     is non-decreasing in x for total > 0 (a rounded product by a positive constant is monotone),
// so { x : thr(x) <= cum_j } is a prefix { x <= T_j } of the 2^32 words (possibly empty, possibly all of them) and
//   sample_cat = #{ j < NS - 1 : !(thr(x) <= cum_j) } = #{ j < NS - 1 : x > T_j }:
// NS - 1 unsigned compares and no floating-point operation.  T_j is found by bisection on the predicate itself, written with the
// expressions and the order of sample_cat and u01, so the index is the one sample_cat returns for every word -- whatever the signs
// of the p_c, as long as the total is positive and finite.
//
// One entry is 16 bytes, four 32-bit words:
//   words 0 .. NS-2   T_j, the largest word with thr(x) <= cum_j; 0xFFFFFFFF when EVERY word satisfies it (x > T_j never holds) and
//                     also when NO word does -- those j are counted in `extra` instead;
//   words NS-1 .. 2   0xFFFFFFFF (NS < 4: compares that never count);
//   word 3            extra (0 .. NS-1, added to the index) | DRAW_TAB_FALLBACK when the entry cannot be tabulated: !(total > 0) or a
//                     total that is not finite, where sample_cat raises DERR_ZERO_PROB -- the caller then runs the arithmetic draw, so
//                     flags and indices stay what they are.
// Host and device evaluate this one text; both sides are built with -ffp-contract=off (the sums of products below must not fuse).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PHM_DRAW_TAB_HD __host__ __device__
#else
#define PHM_DRAW_TAB_HD
#endif

namespace phm {

constexpr int DRAW_TAB_ROWS = 64;                      // chain rows kk = 0 .. 63 are tabulated (fewer when the chain tables are shorter)
constexpr uint32_t DRAW_TAB_FALLBACK = 0x80000000u;    // in word 3
constexpr uint32_t DRAW_TAB_NEVER = 0xFFFFFFFFu;       // a threshold no word exceeds

// thr(x) <= cum, as sample_cat compares it: thr = u01(x) * total
PHM_DRAW_TAB_HD inline bool draw_tab_below(uint32_t x, double total, double cum) {
  const double u = ((double)x + 0.5) * 2.3283064365386962890625e-10;
  const double thr = u * total;
  return thr <= cum;
}

// total and the running sums cum_0 .. cum_{NS-2} of p_c = b2row[c] * beta[c], added as sample_cat adds them
template <int NS>
PHM_DRAW_TAB_HD inline void draw_tab_sums(const double* b2row, const double* beta, double& total, double (&cum)[NS]) {
  double p[NS];
  for (int c = 0; c < NS; ++c) p[c] = b2row[c] * beta[c];
  total = p[0];
  for (int j = 1; j < NS; ++j) total += p[j];
  double run = p[0];
  cum[0] = run;
  for (int j = 1; j < NS; ++j) { run += p[j]; cum[j] = run; }
}

PHM_DRAW_TAB_HD inline bool draw_tab_tabulable(double total) {
  return total > 0.0 && total <= 1.7976931348623157e308;      // !(total > 0) or an infinite / NaN total: sample_cat flags it
}

// Word `w` (0 .. 3) of the entry of (b2row, beta): a thread per word on the device, four calls on the host.
template <int NS>
PHM_DRAW_TAB_HD inline uint32_t draw_tab_word(const double* b2row, const double* beta, int w) {
  static_assert(NS >= 2 && NS <= 4, "an entry holds three thresholds");
  double total, cum[NS];
  draw_tab_sums<NS>(b2row, beta, total, cum);
  const bool ok = draw_tab_tabulable(total);
  if (w == 3) {
    if (!ok) return DRAW_TAB_FALLBACK;
    uint32_t extra = 0;
    for (int j = 0; j < NS - 1; ++j) extra += draw_tab_below(0u, total, cum[j]) ? 0u : 1u;      // no word at all: every draw counts j
    return extra;
  }
  if (!ok || w >= NS - 1) return DRAW_TAB_NEVER;
  double c = cum[0];
  for (int j = 1; j < NS - 1; ++j) if (j == w) c = cum[j];                  // a select, not an indexed register array
  if (!draw_tab_below(0u, total, c)) return DRAW_TAB_NEVER;                 // counted in extra
  if (draw_tab_below(0xFFFFFFFFu, total, c)) return DRAW_TAB_NEVER;         // every word: never counted
  uint32_t lo = 0u, hi = 0xFFFFFFFFu;                                       // below(lo), !below(hi)
  while (hi - lo > 1u) {                                                    // at most 32 halvings
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (draw_tab_below(mid, total, c)) lo = mid; else hi = mid;
  }
  return lo;
}

template <int NS>
PHM_DRAW_TAB_HD inline void draw_tab_entry(const double* b2row, const double* beta, uint32_t (&out)[4]) {
  for (int w = 0; w < 4; ++w) out[w] = draw_tab_word<NS>(b2row, beta, w);
}

// the draw: the index sample_cat would return for the word x (the entry's fallback bit clear)
template <int NS>
PHM_DRAW_TAB_HD inline int draw_tab_index(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t last, uint32_t x) {
  int idx = (int)last + (x > t0 ? 1 : 0);
  if (NS > 2) idx += x > t1 ? 1 : 0;
  if (NS > 3) idx += x > t2 ? 1 : 0;
  return idx;
}

}  // namespace phm
