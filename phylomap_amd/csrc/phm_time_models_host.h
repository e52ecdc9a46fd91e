// phm_time_models_host.h -- the pure host pieces of phm_expected_through_time_models (phm_time_models_api.cpp, DESIGN.md section
// 28): the checks of the bounds and the caller's points, and the plan that every model and every device of a call shares -- node
// depths, the crossings of every boundary, the sub-branches of every bin and the caller's points as items (phm::TmItem).  The
// plan depends on the tree and the bounds alone, not on any Q.  It is section 16's (tt_plan in phm_expect_time.cpp, which is not
// callable from outside its file), restated rule for rule and message for message; what is per model there -- Pade squaring
// counts and Poisson weight tables -- does not exist here: the lanes form their weights on the device.  No HIP call and no
// library state: a refusal comes back as a status and a message.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/phylomap_hip.h"
#include "phm_time_models.h"

namespace phm_tm {

constexpr size_t TM_SCRATCH = size_t(256) << 20;       // what the stages of one launch write: posteriors, or a, beta and rows

// The tree as the plan reads it: per edge row the node rows of its ends, and the edge rows parent first.
struct TmTree {
  int E = 0, NT = 0, root = 0;                          // root: node row of the root
  const double* t = nullptr;                            // [E] branch lengths
  std::vector<int32_t> order, parent, child;            // [E] each
};

struct TmPlan {
  int n_bounds = 0;
  std::vector<phm::TmItem> pts;                         // the boundaries' crossings (by boundary, then edge row), then the caller's points
  int64_t n_cross = 0;
  std::vector<int64_t> cross_off;                       // [n_bounds + 1]: boundary k's crossings in pts
  std::vector<phm::TmItem> sub;                         // sub-branches by (bin, edge row)
  std::vector<int64_t> bin_off;                         // [n_bounds]: bin k's sub-branches
};

inline phm::TmItem tm_item(const TmTree& tr, int32_t b, double s1, double s2) { return {b, 0, s1, tr.t[b] - s2, s2 - s1}; }

// the argument checks that phm_expected_through_time makes on its outputs and counts, in its order and words
inline int32_t tm_check_counts(int32_t n_bounds, const double* bounds, bool occ, bool bins, int64_t n_points, const int32_t* pe,
                               const double* pp, bool points, std::string& err) {
  if (n_bounds < 0 || (n_bounds > 0 && !bounds)) { err = "bounds must hold n_bounds >= 0 values"; return PHM_ERR_BAD_INPUT; }
  if (occ && n_bounds < 1) { err = "occupancy needs n_bounds >= 1"; return PHM_ERR_BAD_INPUT; }
  if (bins && n_bounds < 2) { err = "bin_stats needs n_bounds >= 2"; return PHM_ERR_BAD_INPUT; }
  if (n_points < 0 || (n_points > 0 && (!pe || !pp))) { err = "point_edge and point_pos must hold n_points >= 0 values"; return PHM_ERR_BAD_INPUT; }
  if (points && n_points < 1) { err = "point_post needs n_points >= 1"; return PHM_ERR_BAD_INPUT; }
  return PHM_OK;
}

// the value checks of the bounds and the points, then the plan
inline int32_t tm_plan(const TmTree& tr, int32_t K, const double* bounds, bool occ, bool bins, int64_t P, const int32_t* pe,
                       const double* pp, bool points, TmPlan& pl, std::string& err) {
  for (int k = 0; k < K; ++k) {
    const double tau = bounds[k];
    if (!std::isfinite(tau) || tau < 0.0) { err = "bounds[" + std::to_string(k) + "] must be finite and >= 0"; return PHM_ERR_BAD_INPUT; }
    if (k > 0 && !(tau > bounds[k - 1])) {
      err = "bounds[" + std::to_string(k) + "] is not above bounds[" + std::to_string(k - 1) + "] (bounds must increase strictly)";
      return PHM_ERR_BAD_INPUT;
    }
  }
  for (int64_t i = 0; i < P; ++i) {
    const int32_t b = pe[i];
    if (b < 0 || b >= tr.E) {
      err = "point " + std::to_string(i) + ": edge row " + std::to_string(b) + " is not in 0..n_edge-1";
      return PHM_ERR_BAD_INPUT;
    }
    if (!(pp[i] >= 0.0 && pp[i] <= tr.t[b])) {
      err = "point " + std::to_string(i) + ": position " + std::to_string(pp[i]) + " is not in [0, t_b] of edge row " + std::to_string(b);
      return PHM_ERR_BAD_INPUT;
    }
  }
  // depths parent first: d(root) = 0, d(c) = d(p) + t_b
  std::vector<double> d((size_t)tr.NT, 0.0);
  for (int32_t b : tr.order) d[tr.child[b]] = d[tr.parent[b]] + tr.t[b];
  int32_t root_edge = 0;                                // tau = 0 counts the root through the start of its lowest branch row
  while (tr.parent[root_edge] != tr.root) ++root_edge;
  pl.n_bounds = K;
  if (occ) {
    pl.cross_off.assign(1, 0);
    for (int k = 0; k < K; ++k) {
      const double tau = bounds[k];
      if (tau == 0.0) pl.pts.push_back(tm_item(tr, root_edge, 0.0, 0.0));
      for (int b = 0; b < tr.E; ++b) {
        const double dp = d[tr.parent[b]], dc = d[tr.child[b]], tb = tr.t[b];
        if (dp < tau && tau <= dc) {
          const double s = tau >= dc ? tb : std::min(tau - dp, tb);
          pl.pts.push_back(tm_item(tr, b, s, s));
        }
      }
      pl.cross_off.push_back((int64_t)pl.pts.size());
    }
  }
  pl.n_cross = (int64_t)pl.pts.size();
  if (points)
    for (int64_t i = 0; i < P; ++i) pl.pts.push_back(tm_item(tr, pe[i], pp[i], pp[i]));
  if (bins) {
    pl.bin_off.assign(1, 0);
    for (int k = 0; k + 1 < K; ++k) {
      const double lo = bounds[k], hi = bounds[k + 1];
      for (int b = 0; b < tr.E; ++b) {
        const double dp = d[tr.parent[b]], dc = d[tr.child[b]], tb = tr.t[b];
        if (!(dp < hi && dc > lo)) continue;
        const double s1 = lo <= dp ? 0.0 : std::min(lo - dp, tb), s2 = hi >= dc ? tb : std::min(hi - dp, tb);
        if (!(s2 > s1)) continue;
        pl.sub.push_back(tm_item(tr, b, s1, s2));
      }
      pl.bin_off.push_back((int64_t)pl.sub.size());
    }
  }
  return PHM_OK;
}

// items of one launch whose cells of cell_doubles doubles per (item, evaluation) stay within TM_SCRATCH for Evm evaluations;
// chunk: phm_debug_options.expect_chunk
inline int tm_items_per_launch(int64_t n_items, size_t cell_doubles, size_t Evm, int chunk) {
  const size_t fit = TM_SCRATCH / (sizeof(double) * cell_doubles * std::max<size_t>(Evm, 1));
  int cap = (int)std::max<size_t>(1, std::min<size_t>({(size_t)std::max<int64_t>(n_items, 1), (size_t)phm::TM_GRID_MAX, fit}));
  if (chunk > 0) cap = std::min(cap, chunk);
  return cap;
}

// the ranges [r_begin, r_end) of off (range r: items off[r] .. off[r + 1] - 1) that can meet items [q0, q1)
inline void tm_ranges(const std::vector<int64_t>& off, int64_t q0, int64_t q1, int& r_begin, int& r_end) {
  r_begin = std::max(0, (int)(std::upper_bound(off.begin(), off.end(), q0) - off.begin()) - 1);
  r_end = std::min((int)off.size() - 1, (int)(std::lower_bound(off.begin(), off.end(), q1) - off.begin()));
}

}  // namespace phm_tm
