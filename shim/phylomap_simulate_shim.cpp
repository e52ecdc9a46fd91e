// phylomap_simulate_shim.cpp -- `.Call` binding of the forward simulator (phm_simulate_histories, include/phylomap_hip.h): the
// device replacement of sample2statehistory / samplethebranch (R/sourceme.R:346-414) behind the wrappers of
// shim/R/phylomap_simulate.R.  Kept apart from phylomap_shim.cpp, which mirrors the reference's RcppExports one for one; this
// export has no counterpart there.  Built the same way (PKG_CPPFLAGS=-I<repo>/include PKG_LIBS=-L<repo>/phylomap_amd -lphylomap_hip).
#include <Rcpp.h>

#include <vector>

#include "phylomap_hip.h"

using namespace Rcpp;

namespace {

void check(int32_t st) {
  if (st != PHM_OK) stop("phylomap_hip: %s: %s", phm_status_string(st), phm_last_error());
}

}  // namespace

// x: the tree (x$edge, x$edge.length, x$Nnode, length(x$states) are read); Q: n x n rate matrix; pid: root prior;
// R: number of histories; observe: integer vector of n values in 1..n (reported tip state per true state) or a length-0 vector
// for the identity; want_nodes: TRUE for the node-state matrix.  Returns list(tips = R x n_tips, stats = R x (n + n*n + 1),
// nodes = R x (n_tips + Nnode) when want_nodes).  The Philox seed is drawn from R's stream inside the RNGScope, so set.seed() controls
// the result, as in every other export.
RcppExport SEXP phylomap_hip_simulate_histories(SEXP xSEXP, SEXP QSEXP, SEXP pidSEXP, SEXP RSEXP, SEXP observeSEXP,
                                                SEXP nodesSEXP) {
  BEGIN_RCPP
  RNGScope scope;
  List x = as<List>(xSEXP);
  IntegerMatrix e = as<IntegerMatrix>(x["edge"]);
  NumericVector el = as<NumericVector>(x["edge.length"]);
  IntegerVector st = as<IntegerVector>(x["states"]);
  NumericMatrix Q(QSEXP);
  NumericVector pid(pidSEXP);
  IntegerVector observe(observeSEXP);
  const int n = Q.nrow(), R = as<int>(RSEXP), T = (int)st.size(), Nn = as<int>(x["Nnode"]);
  const bool want_nodes = as<bool>(nodesSEXP);
  if (R < 1) stop("R must be >= 1");
  if (observe.size() != 0 && observe.size() != n) stop("observe must have %d entries", n);
  if (pid.size() != n) stop("pid must have %d entries", n);
  std::vector<int32_t> edge(e.begin(), e.end());                    // column-major, 1-based
  std::vector<double> len(el.begin(), el.end());
  phm_tree t = phm_tree();
  t.n_tips = T; t.n_node = Nn; t.n_edge = e.nrow();
  t.edge = edge.data(); t.edge_length = len.data();
  phm_options o = phm_options();
  uint64_t hi = (uint64_t)(unif_rand() * 4294967296.0), lo = (uint64_t)(unif_rand() * 4294967296.0);
  o.seed = (hi << 32) | lo;
  o.device = -1;
  o.n_replicas = R;
  std::vector<int32_t> tips((size_t)R * T), nodes(want_nodes ? (size_t)R * (T + Nn) : 0);
  NumericMatrix stats(R, n + n * n + 1);                            // column-major: the C-ABI layout
  check(phm_simulate_histories(&t, n, Q.begin(), pid.begin(), observe.size() ? observe.begin() : nullptr, &o, tips.data(),
                               want_nodes ? nodes.data() : nullptr, stats.begin()));
  IntegerMatrix tm(R, T);                                            // replica-major -> R's column-major
  for (int r = 0; r < R; ++r)
    for (int i = 0; i < T; ++i) tm.begin()[r + (size_t)R * i] = tips[(size_t)r * T + i];
  if (!want_nodes) return List::create(Named("tips") = tm, Named("stats") = stats);
  IntegerMatrix nm(R, T + Nn);
  for (int r = 0; r < R; ++r)
    for (int i = 0; i < T + Nn; ++i) nm.begin()[r + (size_t)R * i] = nodes[(size_t)r * (T + Nn) + i];
  return List::create(Named("tips") = tm, Named("stats") = stats, Named("nodes") = nm);
  END_RCPP
}
