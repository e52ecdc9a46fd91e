// phm_time_models_wide_form.h -- which form of the branch stage a (model, sub-branch) item of phm_expected_through_time_models_wide
// takes: sw_form_terms' rule (phm_scores_wide_form.h), RESTATED operation for operation so that the device
// can run it.  A call has K models x (bins x edges) sub-branches, so a table of host words as section 26 keeps per (model, edge)
// would be the one thing of this entry point that grows with K x items; here every lane of a workgroup evaluates the rule from
// the same two scalars (mu_k, h) and so gets the same M.  Multiplications, divisions, additions and comparisons of doubles alone,
// each rounded as IEEE 754 rounds it on either side (no contraction: -ffp-contract=off), so host and device agree on M for every
// x; tests/native/time_models_wide_host_check.cpp holds this function to sw_form_terms on the host, and
// tests/test_gpu_time_models_wide.py holds the kernel that calls it to section 26's totals bit for bit.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PHM_TMW_HD __host__ __device__
#else
#define PHM_TMW_HD
#endif

namespace phm {

// x = mu_k h >= 0.  Returns the m at which sw_form_terms(x, cap) ends when that is at most cap, else cap + 1 (the long form).
PHM_TMW_HD inline int tmw_form_terms(double x, int cap) {
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
