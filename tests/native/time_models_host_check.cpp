// time_models_host_check.cpp -- runs the pure host pieces of phm_expected_through_time_models
// (phylomap_amd/csrc/phm_time_models_host.h): the checks of the counts, the bounds and the points with their
// messages, the plan (depths, crossings per boundary, sub-branches per bin, the caller's points) on a hand-made 4-tip tree whose
// edge rows are out of order and hold a branch of length 0, the items of a launch against the scratch bound and the ranges that a
// launch can meet.  It checks everything itself (exit status 1 with a line on stderr) and prints "ok".  It makes no HIP call and
// needs no device.  Built with hipcc and -fsanitize=address,undefined on the host side by tests/test_time_models_cpu.py.
#include "phm_time_models_host.h"

#include <cstdio>
#include <limits>

using namespace phm_tm;

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);               \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

// node rows: tips 0..3, root 4, inner 5 and 6.  Depths: 5 at 1.0, 6 at 0.5, tips 0..3 at 2.0, 1.0, 2.0, 2.5.
static const double LEN[6] = {1.0, 1.0, 2.0, 0.5, 0.0, 1.5};
static TmTree tree() {
  TmTree tr;
  tr.E = 6; tr.NT = 7; tr.root = 4; tr.t = LEN;
  tr.parent = {5, 4, 6, 4, 5, 6};
  tr.child = {0, 5, 3, 6, 1, 2};
  tr.order = {1, 3, 0, 4, 2, 5};                        // parent first, not row order
  return tr;
}

static void refusals() {
  const TmTree tr = tree();
  std::string err;
  const double b2[2] = {0.0, 1.0};
  const int32_t pe[2] = {0, 5};
  const double pp[2] = {0.5, 1.5};
  EXPECT(tm_check_counts(2, b2, true, true, 2, pe, pp, true, err) == PHM_OK);
  EXPECT(tm_check_counts(0, nullptr, false, false, 0, nullptr, nullptr, false, err) == PHM_OK);   // loglik alone
  EXPECT(tm_check_counts(-1, b2, false, false, 0, nullptr, nullptr, false, err) == PHM_ERR_BAD_INPUT && err == "bounds must hold n_bounds >= 0 values");
  EXPECT(tm_check_counts(2, nullptr, false, false, 0, nullptr, nullptr, false, err) == PHM_ERR_BAD_INPUT);
  EXPECT(tm_check_counts(0, nullptr, true, false, 0, nullptr, nullptr, false, err) == PHM_ERR_BAD_INPUT && err == "occupancy needs n_bounds >= 1");
  EXPECT(tm_check_counts(1, b2, true, true, 0, nullptr, nullptr, false, err) == PHM_ERR_BAD_INPUT && err == "bin_stats needs n_bounds >= 2");
  EXPECT(tm_check_counts(2, b2, true, true, 2, pe, nullptr, false, err) == PHM_ERR_BAD_INPUT && err == "point_edge and point_pos must hold n_points >= 0 values");
  EXPECT(tm_check_counts(2, b2, true, true, -1, pe, pp, false, err) == PHM_ERR_BAD_INPUT);
  EXPECT(tm_check_counts(2, b2, true, true, 0, pe, pp, true, err) == PHM_ERR_BAD_INPUT && err == "point_post needs n_points >= 1");

  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (double v : {-0.5, nan, inf}) {
    const std::vector<double> b = {0.0, v, 2.0};        // a heap array of its own: a read past it is caught
    TmPlan pl;
    EXPECT(tm_plan(tr, 3, b.data(), true, true, 0, nullptr, nullptr, false, pl, err) == PHM_ERR_BAD_INPUT && err == "bounds[1] must be finite and >= 0");
  }
  for (double v : {1.0, 0.5}) {
    const std::vector<double> b = {0.0, 1.0, v};
    TmPlan pl;
    EXPECT(tm_plan(tr, 3, b.data(), true, true, 0, nullptr, nullptr, false, pl, err) == PHM_ERR_BAD_INPUT &&
           err == "bounds[2] is not above bounds[1] (bounds must increase strictly)");
  }
  for (int32_t e : {-1, 6}) {
    const std::vector<int32_t> edges = {0, e};
    const std::vector<double> pos = {0.0, 0.0};
    TmPlan pl;
    EXPECT(tm_plan(tr, 0, nullptr, false, false, 2, edges.data(), pos.data(), true, pl, err) == PHM_ERR_BAD_INPUT &&
           err == "point 1: edge row " + std::to_string(e) + " is not in 0..n_edge-1");
  }
  for (double s : {-0.25, 1.75, nan}) {
    const std::vector<int32_t> edges = {2, 5};
    const std::vector<double> pos = {2.0, s};             // the first sits exactly on t_b: allowed
    TmPlan pl;
    EXPECT(tm_plan(tr, 0, nullptr, false, false, 2, edges.data(), pos.data(), true, pl, err) == PHM_ERR_BAD_INPUT &&
           err.find("point 1: position ") == 0 && err.find(" is not in [0, t_b] of edge row 5") != std::string::npos);
  }
}

static bool is_item(const phm::TmItem& it, int edge, double t1, double t2, double h) {
  return it.edge == edge && it.pad == 0 && it.t1 == t1 && it.t2 == t2 && it.h == h;
}

static void plan() {
  const TmTree tr = tree();
  std::string err;
  const std::vector<double> bounds = {0.0, 0.5, 1.0, 2.0, 3.0};
  const std::vector<int32_t> pe = {4, 2, 2, 2};
  const std::vector<double> pp = {0.0, 0.0, 2.0, 0.75};
  TmPlan pl;
  EXPECT(tm_plan(tr, 5, bounds.data(), true, true, 4, pe.data(), pp.data(), true, pl, err) == PHM_OK);
  EXPECT(pl.n_bounds == 5 && pl.n_cross == 9 && pl.pts.size() == 13);
  EXPECT((pl.cross_off == std::vector<int64_t>{0, 1, 3, 6, 9, 9}));
  // tau = 0: the root through the start of its lowest branch row; a node on a boundary counts through its parent branch at t_b;
  // the branch of length 0 (row 4) never counts
  EXPECT(is_item(pl.pts[0], 1, 0.0, 1.0, 0.0));
  EXPECT(is_item(pl.pts[1], 1, 0.5, 0.5, 0.0) && is_item(pl.pts[2], 3, 0.5, 0.0, 0.0));
  EXPECT(is_item(pl.pts[3], 1, 1.0, 0.0, 0.0) && is_item(pl.pts[4], 2, 0.5, 1.5, 0.0) && is_item(pl.pts[5], 5, 0.5, 1.0, 0.0));
  EXPECT(is_item(pl.pts[6], 0, 1.0, 0.0, 0.0) && is_item(pl.pts[7], 2, 1.5, 0.5, 0.0) && is_item(pl.pts[8], 5, 1.5, 0.0, 0.0));
  // the caller's points follow in the caller's order
  EXPECT(is_item(pl.pts[9], 4, 0.0, 0.0, 0.0) && is_item(pl.pts[10], 2, 0.0, 2.0, 0.0) && is_item(pl.pts[11], 2, 2.0, 0.0, 0.0) &&
         is_item(pl.pts[12], 2, 0.75, 1.25, 0.0));
  // sub-branches by (bin, edge row); together they are the tree
  EXPECT((pl.bin_off == std::vector<int64_t>{0, 2, 5, 8, 9}) && pl.sub.size() == 9);
  EXPECT(is_item(pl.sub[0], 1, 0.0, 0.5, 0.5) && is_item(pl.sub[1], 3, 0.0, 0.0, 0.5));
  EXPECT(is_item(pl.sub[2], 1, 0.5, 0.0, 0.5) && is_item(pl.sub[3], 2, 0.0, 1.5, 0.5) && is_item(pl.sub[4], 5, 0.0, 1.0, 0.5));
  EXPECT(is_item(pl.sub[5], 0, 0.0, 0.0, 1.0) && is_item(pl.sub[6], 2, 0.5, 0.5, 1.0) && is_item(pl.sub[7], 5, 0.5, 0.0, 1.0));
  EXPECT(is_item(pl.sub[8], 2, 1.5, 0.0, 0.5));
  double total = 0.0;
  for (const phm::TmItem& it : pl.sub) total += it.h;
  EXPECT(total == 6.0);

  // only what is asked for is planned
  TmPlan only;
  EXPECT(tm_plan(tr, 5, bounds.data(), false, false, 4, pe.data(), pp.data(), true, only, err) == PHM_OK);
  EXPECT(only.n_cross == 0 && only.pts.size() == 4 && only.sub.empty() && only.cross_off.empty() && only.bin_off.empty());
  TmPlan bins;
  EXPECT(tm_plan(tr, 5, bounds.data(), false, true, 4, pe.data(), pp.data(), false, bins, err) == PHM_OK);
  EXPECT(bins.pts.empty() && bins.sub.size() == 9);
}

static void launches() {
  // cells of 26 doubles (n = 4 sub-branches) for 1 024 evaluations: 213 KB an item, 1 260 items in 256 MB
  EXPECT(tm_items_per_launch(66547, 26, 1024, 0) == (int)(TM_SCRATCH / (8 * 26 * 1024)));
  EXPECT(tm_items_per_launch(66547, 26, 1024, 5) == 5 && tm_items_per_launch(3, 26, 1024, 5) == 3);
  EXPECT(tm_items_per_launch(70000, 2, 1, 0) == phm::TM_GRID_MAX);
  EXPECT(tm_items_per_launch(10, 64, (size_t)1 << 30, 0) == 1);           // never below one item
  for (size_t Ev : {(size_t)1, (size_t)65, (size_t)4096, (size_t)1 << 20})
    for (size_t cell : {(size_t)2, (size_t)26, (size_t)82}) {
      const int cap = tm_items_per_launch(100000, cell, Ev, 0);
      EXPECT(cap >= 1 && cap <= phm::TM_GRID_MAX && (cap == 1 || sizeof(double) * cell * Ev * (size_t)cap <= TM_SCRATCH));
    }
  const std::vector<int64_t> off = {0, 1, 3, 6, 9, 9};
  int r0 = -1, r1 = -1;
  tm_ranges(off, 0, 9, r0, r1);
  EXPECT(r0 == 0 && r1 >= 4 && r1 <= 5);
  tm_ranges(off, 3, 6, r0, r1);                                           // exactly range 2
  EXPECT(r0 <= 2 && r1 >= 3 && r0 >= 0 && r1 <= 5);
  tm_ranges(off, 4, 5, r0, r1);                                           // inside range 2
  EXPECT(r0 <= 2 && r1 >= 3 && r1 <= 5);
  tm_ranges(off, 8, 9, r0, r1);
  EXPECT(r0 <= 3 && r1 >= 4 && r1 <= 5);
  // every item of a launch lies in one of the ranges the launch is given, for every split of the items
  for (int64_t step = 1; step <= 9; ++step)
    for (int64_t q0 = 0; q0 < 9; q0 += step) {
      const int64_t q1 = std::min<int64_t>(9, q0 + step);
      tm_ranges(off, q0, q1, r0, r1);
      EXPECT(r0 >= 0 && r1 <= 5 && r0 <= r1);
      for (int64_t q = q0; q < q1; ++q) {
        bool held = false;
        for (int r = r0; r < r1; ++r) held = held || (off[r] <= q && q < off[r + 1]);
        EXPECT(held);
      }
    }
}

int main() {
  refusals();
  plan();
  launches();
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
