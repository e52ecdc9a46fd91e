// time_models_wide_host_check.cpp -- runs the pure host pieces that phm_expected_through_time_models_wide adds
// (phylomap_amd/csrc/phm_time_models_wide_form.h and phm_time_models_wide_host.h): the restated form rule
// against sw_form_terms over a sweep of x that crosses every M, the switch to the long form and the rescaling by 2^-512; the state
// counts served; what an item writes and what an evaluation takes; the fit of a chunk and the items of a launch against the
// scratch bound.  It checks everything itself (exit status 1 with a line on stderr) and prints "ok".  It makes no HIP call and
// needs no device.  Built with hipcc and -fsanitize=address,undefined on the host side by tests/test_time_models_wide_cpu.py.
#include "phm_scores_wide_form.h"
#include "phm_time_models_wide_form.h"
#include "phm_time_models_wide_host.h"

#include <cmath>
#include <cstdio>

using namespace phm_tmw;

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);               \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

static void form_rule() {
  const int cap = phm::SW_M_CAP;
  int seen_short = 0, seen_long = 0, last = -1, mismatches = 0;
  // a fine sweep over [0, 40] crosses every M and the switch (near x = 17.1); then decades up to the limit 1e6
  for (int i = 0; i <= 400000; ++i) {
    const double x = 1e-4 * (double)i;
    const int want = phm::sw_form_terms(x, cap), got = phm::tmw_form_terms(x, cap);
    if (want != got) ++mismatches;
    if (want <= cap) ++seen_short; else ++seen_long;
    EXPECT(want >= last || want == cap + 1);              // M does not fall as x grows
    last = want <= cap ? want : last;
  }
  for (double x = 1e-300; x < 2e6; x *= 1.37) {
    if (phm::sw_form_terms(x, cap) != phm::tmw_form_terms(x, cap)) ++mismatches;
    for (int c : {0, 1, 7}) if (phm::sw_form_terms(x, c) != phm::tmw_form_terms(x, c)) ++mismatches;
  }
  EXPECT(mismatches == 0);
  EXPECT(seen_short > 0 && seen_long > 0);
  EXPECT(phm::tmw_form_terms(0.0, cap) == 0);
  EXPECT(phm::tmw_form_terms(17.0, cap) <= cap && phm::tmw_form_terms(17.2, cap) == cap + 1);   // the switch lies between
  EXPECT(phm::tmw_form_terms(1e6, cap) == cap + 1);
}

static void sizes() {
  EXPECT(!tmw_serves(8) && tmw_serves(9) && tmw_serves(64) && !tmw_serves(65) && !tmw_serves(0) && !tmw_serves(-3));
  EXPECT(tmw_point_cell(9) == 9 && tmw_point_cell(64) == 64);
  EXPECT(tmw_sub_cell(9) == 2 * 16 + 2 + 81 && tmw_sub_cell(16) == 2 * 16 + 2 + 256 && tmw_sub_cell(17) == 2 * 32 + 2 + 289);
  EXPECT(tmw_sub_cell(33) == 2 * 64 + 2 + 33 * 33 && tmw_sub_cell(64) == 2 * 64 + 2 + 4096);
  // per evaluation: O and F rows of NP doubles with an int32 exponent each, lam, and the sums that are asked for
  const size_t vec16 = 8 * 16 + 4;
  EXPECT(tmw_per_eval_bytes(9, 17, 16, 0, false, false, 0) == vec16 * 17 + vec16 * 16 + 8);
  EXPECT(tmw_per_eval_bytes(9, 17, 16, 5, true, false, 0) == vec16 * 33 + 8 * (1 + 9 * 5));
  EXPECT(tmw_per_eval_bytes(9, 17, 16, 5, true, true, 0) == vec16 * 33 + 8 * (1 + 9 * 5 + 81 * 4));
  EXPECT(tmw_per_eval_bytes(9, 17, 16, 5, false, true, 3) == vec16 * 33 + 8 * (1 + 81 * 4 + 3 * 4));
  EXPECT(tmw_per_eval_bytes(9, 17, 16, 1, true, true, 3) == vec16 * 33 + 8 * (1 + 9));            // one bound: no bin
}

static void launches() {
  const size_t scratch = phm_tm::TM_SCRATCH;
  {                                                       // a small call: everything in one launch, the chunk untouched
    int64_t Kc = 16, Sc = 8;
    const TmwLaunch l = tmw_launches(20, 300, 500, 0, Kc, Sc);
    EXPECT(Kc == 16 && Sc == 8 && l.np_max == 300 && l.ns_max == 500);
  }
  {                                                       // no points, no sub-branches
    int64_t Kc = 3, Sc = 2;
    const TmwLaunch l = tmw_launches(9, 0, 0, 0, Kc, Sc);
    EXPECT(l.np_max == 0 && l.ns_max == 0 && Kc == 3 && Sc == 2);
  }
  {                                                       // past one grid: 65 535 items at most
    int64_t Kc = 1, Sc = 1;
    const TmwLaunch l = tmw_launches(9, 66000, 0, 0, Kc, Sc);
    EXPECT(l.np_max == 65535 && l.ns_max == 0);
  }
  {                                                       // expect_chunk caps the items
    int64_t Kc = 1, Sc = 1;
    const TmwLaunch l = tmw_launches(9, 100, 100, 5, Kc, Sc);
    EXPECT(l.np_max == 5 && l.ns_max == 5);
  }
  {                                                       // the scratch bound: a launch's writes stay within it
    int64_t Kc = 64, Sc = 100;
    const TmwLaunch l = tmw_launches(64, 50000, 50000, 0, Kc, Sc);
    const size_t Ev = (size_t)Kc * (size_t)Sc;
    EXPECT(Kc == 64 && Sc == 100);
    EXPECT(l.ns_max >= 1 && sizeof(double) * tmw_sub_cell(64) * Ev * (size_t)l.ns_max <= scratch);
    EXPECT(sizeof(double) * tmw_sub_cell(64) * Ev * (size_t)(l.ns_max + 1) > scratch);
    EXPECT(l.np_max >= 1 && sizeof(double) * tmw_point_cell(64) * Ev * (size_t)l.np_max <= scratch);
  }
  {                                                       // one item does not fit: first the models shrink, then the sites
    int64_t Kc = 4096, Sc = 4096;
    const TmwLaunch l = tmw_launches(64, 10, 10, 0, Kc, Sc);
    EXPECT(Kc >= 1 && Sc >= 1 && Kc < 4096);
    EXPECT(sizeof(double) * tmw_sub_cell(64) * (size_t)Kc * (size_t)Sc <= scratch);
    EXPECT(l.ns_max == 1 && l.np_max >= 1);
    int64_t K1 = 1, S1 = 60000;                           // one model alone is too much: the sites shrink
    const TmwLaunch m = tmw_launches(64, 0, 10, 0, K1, S1);
    EXPECT(K1 == 1 && S1 < 60000 && S1 >= 1 && sizeof(double) * tmw_sub_cell(64) * (size_t)S1 <= scratch && m.ns_max == 1);
  }
}

int main() {
  form_rule();
  sizes();
  launches();
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
