// branch_rows_host_check.cpp -- runs the pure host pieces of phm_expected_branch_stats_models
// (phylomap_amd/csrc/phm_branch_rows_host.h): the edge selection with its refusals, the label weights in
// column order, the limit on mu t_b over the SELECTED edges, and the plan of models, sites and selected edges per branch-stage
// launch over a grid of shapes.  It checks the first three itself (exit status 1 with a line on stderr) and prints one line
// "plan n labels unit Kc0 Sc0 chunk n_sel Kc Sc ne" per planned shape.  It makes no HIP call and needs no device.  Built with
// hipcc and -fsanitize=address,undefined on the host side by tests/test_branch_rows_cpu.py, which checks the printed plans
// against the scratch bound.
#include "phm_branch_rows_host.h"

#include <cinttypes>
#include <cstdio>
#include <limits>

using namespace phm_br;

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);               \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

static void selection() {
  const int n = 3, E = 10;
  BrSelection sel;
  std::string err;
  // every edge row, in row order; n_edges is ignored
  EXPECT(br_select(n, E, -7, nullptr, 0, nullptr, sel, err) == PHM_OK);
  EXPECT(sel.n_sel == E && sel.n_labels == 0 && sel.out_cols == 9 && sel.w.empty());
  for (int b = 0; b < E; ++b) EXPECT(sel.edges[b] == b);
  // any order, repeats; the list is copied exactly as long as it is (a heap array of its own: a read past it is caught)
  std::vector<int32_t> list = {9, 0, 4, 4, 3};
  EXPECT(br_select(n, E, (int32_t)list.size(), list.data(), 0, nullptr, sel, err) == PHM_OK);
  EXPECT(sel.n_sel == 5 && sel.edges == list);
  EXPECT(br_select(n, E, 0, list.data(), 0, nullptr, sel, err) == PHM_ERR_BAD_INPUT && err.find("n_edges must be >= 1") == 0);
  EXPECT(br_select(n, E, -1, list.data(), 0, nullptr, sel, err) == PHM_ERR_BAD_INPUT);
  list[3] = E;
  EXPECT(br_select(n, E, 5, list.data(), 0, nullptr, sel, err) == PHM_ERR_BAD_INPUT && err.find("edges[3] = 10 is outside 0..9") == 0);
  list[3] = -1;
  EXPECT(br_select(n, E, 5, list.data(), 0, nullptr, sel, err) == PHM_ERR_BAD_INPUT && err.find("edges[3] = -1") == 0);
  EXPECT(br_select(n, E, 3, list.data(), 0, nullptr, sel, err) == PHM_OK && sel.n_sel == 3);   // the bad entry lies past the list

  // labels: [L][n][n] column-major; (i, i) -> column i, (i, j) -> count_col
  std::vector<double> lab(2 * 9);
  for (int l = 0; l < 2; ++l)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) lab[(size_t)l * 9 + j * n + i] = 100.0 * l + 10.0 * i + j;     // the value names (l, from, to)
  EXPECT(br_select(n, E, 0, nullptr, 2, lab.data(), sel, err) == PHM_OK);
  EXPECT(sel.n_labels == 2 && sel.out_cols == 2 && sel.w.size() == 18);
  const double want0[9] = {0, 11, 22, 1, 2, 10, 12, 20, 21};               // dwell 0..2, then (0,1) (0,2) (1,0) (1,2) (2,0) (2,1)
  for (int c = 0; c < 9; ++c) EXPECT(sel.w[c] == want0[c] && sel.w[9 + c] == 100.0 + want0[c]);
  EXPECT(br_count_col(3, 0, 1) == 3 && br_count_col(3, 2, 1) == 8 && br_count_col(64, 63, 62) == 64 + 63 * 63 + 62);
  EXPECT(br_select(n, E, 0, nullptr, 0, lab.data(), sel, err) == PHM_ERR_BAD_INPUT && err.find("n_labels must be >= 1") == 0);
  EXPECT(br_select(n, E, 0, nullptr, BR_LABELS_MAX + 1, lab.data(), sel, err) == PHM_ERR_BAD_INPUT);
  lab[9 + 4] = std::numeric_limits<double>::quiet_NaN();
  EXPECT(br_select(n, E, 0, nullptr, 2, lab.data(), sel, err) == PHM_ERR_BAD_INPUT && err == "label 1 has a non-finite weight");
  EXPECT(br_select(n, E, 0, nullptr, 1, lab.data(), sel, err) == PHM_OK && sel.n_labels == 1);   // the poisoned matrix lies past the list
  lab[9 + 4] = -std::numeric_limits<double>::infinity();
  EXPECT(br_select(n, E, 0, nullptr, 2, lab.data(), sel, err) == PHM_ERR_BAD_INPUT);
}

static void jump_mean() {
  const int n = 2;
  const std::vector<double> Qr = {-1.0, 1.0, 2.0, -2.0, -0.5, 0.5, 3e6, -3e6, 0.0, 0.0, 0.0, 0.0};   // mu = 2, 3e6, 0
  std::vector<double> mu;
  br_model_mu(Qr.data(), n, 3, mu);
  EXPECT(mu.size() == 3 && mu[0] == 2.0 && mu[1] == 3e6 && mu[2] == 0.0);
  const std::vector<double> t = {0.1, 0.5, 0.0, 0.2};
  BrSelection sel;
  std::string err;
  EXPECT(br_select(n, 4, 0, nullptr, 0, nullptr, sel, err) == PHM_OK);
  EXPECT(br_check_jump_mean(mu, t.data(), sel, 1e6, err) == PHM_ERR_UNSUPPORTED && err == "model 1, edge row 2: max(-q_ii) * t_b above 1e6");
  const int32_t under[3] = {2, 0, 2};                                      // 3e6 * 0.1 = 3e5: the long edges are not selected
  EXPECT(br_select(n, 4, 3, under, 0, nullptr, sel, err) == PHM_OK);
  EXPECT(br_check_jump_mean(mu, t.data(), sel, 1e6, err) == PHM_OK);
  const int32_t order[2] = {3, 1};                                         // both above a limit of 5e5: the list's first is named
  EXPECT(br_select(n, 4, 2, order, 0, nullptr, sel, err) == PHM_OK);
  EXPECT(br_check_jump_mean(mu, t.data(), sel, 5e5, err) == PHM_ERR_UNSUPPORTED && err.find("model 1, edge row 4:") == 0);
}

static void plans() {
  struct Shape { int n, labels; int64_t unit, Kc, Sc; };
  const Shape shapes[] = {{4, 0, 64, 64, 3},        {8, 0, 64, 1024, 1},     {8, 0, 64, 1024, 65535}, {8, 3, 64, 64, 65535},
                          {2, 60000, 64, 128, 700}, {20, 0, 1, 64, 1},       {61, 0, 1, 64, 1},       {61, 3, 1, 64, 1},
                          {64, 0, 1, 65535, 1},     {64, 0, 1, 1, 65535},    {64, 65535, 1, 4, 4000}, {9, 0, 1, 1, 1}};
  const int chunks[] = {0, 2, 64};
  const int sels[] = {1, 78, 100000};
  for (const Shape& s : shapes) {
    BrSelection sel;
    sel.n_labels = s.labels;
    const size_t cell = br_cell_doubles(s.n, sel);
    EXPECT(cell == std::max<size_t>((size_t)s.n * s.n, (size_t)s.labels));
    for (int chunk : chunks)
      for (int n_sel : sels) {
        int64_t Kc = s.Kc, Sc = s.Sc;
        br_fit_chunk(cell, s.unit, Kc, Sc);
        const int ne = br_edges_per_launch(n_sel, cell, (size_t)Kc * (size_t)Sc, chunk, 65535);
        std::printf("plan %d %d %" PRId64 " %" PRId64 " %" PRId64 " %d %d %" PRId64 " %" PRId64 " %d\n", s.n, s.labels, s.unit, s.Kc, s.Sc,
                    chunk, n_sel, Kc, Sc, ne);
      }
  }
}

int main() {
  selection();
  jump_mean();
  plans();
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
