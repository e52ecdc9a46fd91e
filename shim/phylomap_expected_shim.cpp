// phylomap_expected_shim.cpp -- `.Call` binding of the exact conditional expectations (phm_expected_stats,
// include/phylomap_hip.h) behind sumstatExpected() in shim/R/phylomap_expected.R.  Kept apart from phylomap_shim.cpp, which
// mirrors the reference's RcppExports one for one; this export has no counterpart there.  Built the same way
// (PKG_CPPFLAGS=-I<repo>/include PKG_LIBS=-L<repo>/phylomap_amd -lphylomap_hip).
#include <Rcpp.h>

#include <vector>

#include "phylomap_hip.h"

using namespace Rcpp;

namespace {

void check(int32_t st) {
  if (st != PHM_OK) stop("phylomap_hip: %s: %s", phm_status_string(st), phm_last_error());
}

}  // namespace

// x: the tree (x$edge, x$edge.length, x$Nnode are read); sites: S x n_tips integer matrix of tip states (0 = missing, else
// 1..n); Q: n x n rate matrix; pid: root prior; observe: n values in 1..n (the tip state each true state is seen as) or a
// length-0 vector for the identity; per_branch / nodes: TRUE for the per-branch array / the node posteriors.
// Returns list(stats = S x (n + n(n-1)), loglik = S, branch, nodes): branch and nodes are the column-major arrays
// S x n_edge x (n + n(n-1)) and S x (n_tips + Nnode) x n as plain vectors (the C-ABI writes R's layout directly; the R wrapper
// sets their dim).
RcppExport SEXP phylomap_expected_stats(SEXP xSEXP, SEXP sitesSEXP, SEXP QSEXP, SEXP pidSEXP, SEXP observeSEXP,
                                        SEXP branchSEXP, SEXP nodesSEXP) {
  BEGIN_RCPP
  List x = as<List>(xSEXP);
  IntegerMatrix e = as<IntegerMatrix>(x["edge"]);
  NumericVector el = as<NumericVector>(x["edge.length"]);
  IntegerMatrix sites(sitesSEXP);
  NumericMatrix Q(QSEXP);
  NumericVector pid(pidSEXP);
  IntegerVector observe(observeSEXP);
  const int n = Q.nrow(), S = sites.nrow(), T = sites.ncol(), Nn = as<int>(x["Nnode"]), E = e.nrow();
  const bool want_branch = as<bool>(branchSEXP), want_nodes = as<bool>(nodesSEXP);
  if (S < 1) stop("sites must have at least one row");
  if (observe.size() != 0 && observe.size() != n) stop("observe must have %d entries", n);
  if (pid.size() != n) stop("pid must have %d entries", n);
  std::vector<int32_t> edge(e.begin(), e.end());                    // column-major, 1-based
  std::vector<double> len(el.begin(), el.end());
  std::vector<int32_t> tips((size_t)S * T);                          // R's column-major -> replica-major
  for (int s = 0; s < S; ++s)
    for (int i = 0; i < T; ++i) tips[(size_t)s * T + i] = sites.begin()[s + (size_t)S * i];
  phm_tree t = phm_tree();
  t.n_tips = T; t.n_node = Nn; t.n_edge = E;
  t.edge = edge.data(); t.edge_length = len.data(); t.states = tips.data();
  phm_options o = phm_options();
  o.device = -1;
  o.n_replicas = S;
  o.tips_per_replica = 1;
  const int cols = n + n * (n - 1);
  NumericMatrix stats(S, cols);
  NumericVector loglik(S);
  NumericVector branch(want_branch ? S * E * cols : 0);              // dims set by the R wrapper
  NumericVector post(want_nodes ? S * (T + Nn) * n : 0);
  check(phm_expected_stats(&t, n, Q.begin(), pid.begin(), observe.size() ? observe.begin() : nullptr, &o, stats.begin(),
                           loglik.begin(), want_branch ? branch.begin() : nullptr, want_nodes ? post.begin() : nullptr));
  List out = List::create(Named("stats") = stats, Named("loglik") = loglik);
  if (want_branch) out["branch"] = branch;
  if (want_nodes) out["nodes"] = post;
  return out;
  END_RCPP
}
