// phylomap_scores_shim.cpp -- `.Call` binding of the expected statistics of many rate matrices (phm_expected_stats_models,
// include/phylomap_hip.h) behind sumstatExpectedModels() in shim/R/phylomap_scores.R.  Kept apart from phylomap_shim.cpp, which
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

// The arguments are phylomap_loglik_models' (shim/phylomap_loglik_shim.cpp): x the tree, sites an S x n_tips integer matrix, Qs
// n * n * K values (each matrix column-major, model slowest), n the number of states, pid n or n * K values, observe n values or
// length 0, site_of_model length 0 or K 1-BASED site indices.
// Returns list(stats, loglik): stats has one row per evaluation (S * K of them with the site fastest, or K with site_of_model) and
// n + n(n-1) columns, loglik one value per evaluation; an impossible evaluation is -Inf with a row of NaN.  The R wrapper sets
// the dims.
RcppExport SEXP phylomap_expected_stats_models(SEXP xSEXP, SEXP sitesSEXP, SEXP QsSEXP, SEXP nSEXP, SEXP pidSEXP, SEXP observeSEXP,
                                               SEXP siteOfModelSEXP) {
  BEGIN_RCPP
  List x = as<List>(xSEXP);
  IntegerMatrix e = as<IntegerMatrix>(x["edge"]);
  NumericVector el = as<NumericVector>(x["edge.length"]);
  IntegerMatrix sites(sitesSEXP);
  NumericVector Qs(QsSEXP);
  NumericVector pid(pidSEXP);
  IntegerVector observe(observeSEXP);
  IntegerVector som(siteOfModelSEXP);
  const int n = as<int>(nSEXP), S = sites.nrow(), T = sites.ncol(), Nn = as<int>(x["Nnode"]), E = e.nrow();
  if (n < 1 || Qs.size() == 0 || Qs.size() % ((int64_t)n * n) != 0) stop("Qs must hold n * n * K values");
  const int K = (int)(Qs.size() / ((int64_t)n * n));
  if (S < 1) stop("sites must have at least one row");
  if (observe.size() != 0 && observe.size() != n) stop("observe must have %d entries", n);
  if (pid.size() != n && pid.size() != (int64_t)n * K) stop("pid must have n or n * K entries");
  if (som.size() != 0 && som.size() != K) stop("site_of_model must have one entry per model");
  std::vector<int32_t> edge(e.begin(), e.end());                    // column-major, 1-based
  std::vector<double> len(el.begin(), el.end());
  std::vector<int32_t> tips((size_t)S * T);                          // R's column-major -> replica-major
  for (int s = 0; s < S; ++s)
    for (int i = 0; i < T; ++i) tips[(size_t)s * T + i] = sites.begin()[s + (size_t)S * i];
  std::vector<int32_t> som0(som.size());
  for (int64_t k = 0; k < som.size(); ++k) som0[k] = som[k] - 1;
  phm_tree t = phm_tree();
  t.n_tips = T; t.n_node = Nn; t.n_edge = E;
  t.edge = edge.data(); t.edge_length = len.data(); t.states = tips.data();
  phm_options o = phm_options();
  o.device = -1;
  o.n_replicas = S;
  o.tips_per_replica = 1;
  const bool paired = som.size() != 0;
  const int64_t n_eval = paired ? (int64_t)K : (int64_t)S * K;
  NumericVector loglik(n_eval);
  NumericVector stats(n_eval * ((int64_t)n * n));                  // evaluation fastest: an n_eval x cols matrix, column-major
  check(phm_expected_stats_models(&t, n, K, Qs.begin(), pid.begin(), pid.size() == n ? 1 : K,
                                  observe.size() ? observe.begin() : nullptr, paired ? som0.data() : nullptr, &o, stats.begin(),
                                  loglik.begin()));
  return List::create(Named("stats") = stats, Named("loglik") = loglik);
  END_RCPP
}
