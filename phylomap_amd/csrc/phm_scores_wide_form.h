// phm_scores_wide_form.h -- which form of the branch stage a (model, edge) item of phm_expected_stats_models_wide takes (DESIGN.md
// section 26): section 18's Poisson weights and stopping rule, run on the HOST for at most cap + 1 terms.  Pure arithmetic, no
// HIP: tests/native/scores_wide_form_check.cpp runs it without a device.  The short form of phm_scores_wide.hip takes its M from
// the word this function returns, so host and device cannot disagree about it.
#pragma once

namespace phm {

constexpr int SW_M_CAP = 63;                   // short form: v_0 .. v_M of an item live in LDS, M <= SW_M_CAP (every lane class)

// x = mu_k t_b >= 0.  r_0 = x, r_{m+1} = r_m x / (m + 2), S = 1 + sum r_m; r and S are multiplied by 2^-512 whenever r passes
// 2^512; the sum ends at the first m past the mode (x < m + 2) whose geometric tail bound r_{m+1} / (1 - x / (m + 3)) is at
// most 2^-60 S.  Returns that m -- the item keeps r_0 .. r_m -- when it is at most cap, else cap + 1 (the long form).
inline int sw_form_terms(double x, int cap) {
  double r = x, S = 1.0 + x;
  for (int m = 0; m <= cap; ++m) {
    const double rn = r * (x / (double)(m + 2));
    if (x < (double)(m + 2) && rn <= 0x1p-60 * S * (1.0 - x / (double)(m + 3))) return m;
    r = rn;
    S += r;
    if (r > 0x1p512) { r *= 0x1p-512; S *= 0x1p-512; }
  }
  return cap + 1;
}

}  // namespace phm
