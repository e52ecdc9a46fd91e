// scores_wide_form_check.cpp -- prints which form of the branch stage phm_expected_stats_models_wide's host gives an item
// (phylomap_amd/csrc/phm_scores_wide_form.h: sw_form_terms).  Arguments: a cap (0: SW_M_CAP) and then
// x = mu t_b values as C99 hexadecimal floating-point strings, exact doubles.  One line "x terms" per value after the cap.  It
// makes no HIP call and needs no device; tests/test_scores_wide_cpu.py compares it with a Python restatement of the rule.
#include "phm_scores_wide_form.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  int cap = std::atoi(argv[1]);
  if (cap <= 0) cap = phm::SW_M_CAP;
  std::printf("cap %d\n", cap);
  for (int i = 2; i < argc; ++i) {
    char* end = nullptr;
    const double x = std::strtod(argv[i], &end);
    if (end == argv[i] || *end != '\0') return 2;
    std::printf("%a %d\n", x, phm::sw_form_terms(x, cap));
  }
  return 0;
}
