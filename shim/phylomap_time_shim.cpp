// phylomap_time_shim.cpp -- `.Call` binding of the exact expectations through time (phm_expected_through_time,
// include/phylomap_hip.h) behind sumstatExpectedTime() in shim/R/phylomap_time.R.  Kept apart from phylomap_shim.cpp, which mirrors
// the reference's RcppExports one for one; this export has no counterpart there.  Built the same way
// (PKG_CPPFLAGS=-I<repo>/include PKG_LIBS=-L<repo>/phylomap_amd -lphylomap_hip).
#include <Rcpp.h>

#include <cmath>
#include <vector>

#include "phylomap_hip.h"

using namespace Rcpp;

namespace {

void check(int32_t st) {
  if (st != PHM_OK) stop("phylomap_hip: %s: %s", phm_status_string(st), phm_last_error());
}

}  // namespace

// x: the tree (x$edge, x$edge.length, x$Nnode are read); sites: S x n_tips integer matrix of tip states (0 = missing, else
// 1..n); Q: n x n rate matrix; pid: root prior; observe: n values in 1..n or a length-0 vector for the identity; bounds: K depths
// from the root (strictly increasing, >= 0; may be empty); points: P x 2 numeric matrix of (1-based edge row, distance from the
// parent end), P may be 0.
// Returns list(loglik = S, occupancy, bins, points): occupancy (K >= 1), bins (K >= 2) and points (P >= 1) are the column-major
// arrays S x K x n, S x (K - 1) x (n + n(n-1)) and S x P x n as plain vectors (the R wrapper sets their dim).
RcppExport SEXP phylomap_expected_through_time(SEXP xSEXP, SEXP sitesSEXP, SEXP QSEXP, SEXP pidSEXP, SEXP observeSEXP,
                                               SEXP boundsSEXP, SEXP pointsSEXP) {
  BEGIN_RCPP
  List x = as<List>(xSEXP);
  IntegerMatrix e = as<IntegerMatrix>(x["edge"]);
  NumericVector el = as<NumericVector>(x["edge.length"]);
  IntegerMatrix sites(sitesSEXP);
  NumericMatrix Q(QSEXP);
  NumericVector pid(pidSEXP);
  IntegerVector observe(observeSEXP);
  NumericVector bounds(boundsSEXP);
  NumericMatrix points(pointsSEXP);
  const int n = Q.nrow(), S = sites.nrow(), T = sites.ncol(), Nn = as<int>(x["Nnode"]), E = e.nrow();
  const int K = (int)bounds.size(), P = points.nrow();
  if (S < 1) stop("sites must have at least one row");
  if (observe.size() != 0 && observe.size() != n) stop("observe must have %d entries", n);
  if (pid.size() != n) stop("pid must have %d entries", n);
  if (P > 0 && points.ncol() != 2) stop("points must have two columns (edge row, position)");
  std::vector<int32_t> edge(e.begin(), e.end());                    // column-major, 1-based
  std::vector<double> len(el.begin(), el.end());
  std::vector<int32_t> tips((size_t)S * T);                          // R's column-major -> replica-major
  for (int s = 0; s < S; ++s)
    for (int i = 0; i < T; ++i) tips[(size_t)s * T + i] = sites.begin()[s + (size_t)S * i];
  std::vector<int32_t> pe(P);                                        // 1-based edge rows -> 0-based
  std::vector<double> pp(P);
  for (int i = 0; i < P; ++i) {
    pe[i] = (int32_t)std::floor(points.begin()[i] + 0.5) - 1;
    pp[i] = points.begin()[i + (size_t)P];
  }
  phm_tree t = phm_tree();
  t.n_tips = T; t.n_node = Nn; t.n_edge = E;
  t.edge = edge.data(); t.edge_length = len.data(); t.states = tips.data();
  phm_options o = phm_options();
  o.device = -1;
  o.n_replicas = S;
  o.tips_per_replica = 1;
  const int cols = n + n * (n - 1);
  NumericVector loglik(S);
  NumericVector occ(K >= 1 ? S * K * n : 0);
  NumericVector bins(K >= 2 ? S * (K - 1) * cols : 0);
  NumericVector post(P >= 1 ? S * P * n : 0);
  check(phm_expected_through_time(&t, n, Q.begin(), pid.begin(), observe.size() ? observe.begin() : nullptr, &o, K,
                                  K ? bounds.begin() : nullptr, K >= 1 ? occ.begin() : nullptr, K >= 2 ? bins.begin() : nullptr, P,
                                  P ? pe.data() : nullptr, P ? pp.data() : nullptr, P ? post.begin() : nullptr, loglik.begin()));
  List out = List::create(Named("loglik") = loglik);
  if (K >= 1) out["occupancy"] = occ;
  if (K >= 2) out["bins"] = bins;
  if (P >= 1) out["points"] = post;
  return out;
  END_RCPP
}
