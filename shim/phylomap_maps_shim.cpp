// phylomap_maps_shim.cpp -- `.Call` binding of the stochastic-map entry points (phm_simulate_histories_maps,
// phm_maketreelistEXP_maps, include/phylomap_hip.h) behind the wrappers of shim/R/phylomap_maps.R: the simulated or sampled
// histories themselves, one map per (history, edge row), from which shim/R/phylomap_maps.R builds divtophy-shaped trees
// (R/sourceme.R:1-60).  Kept apart from phylomap_shim.cpp (the reference's RcppExports one for one) and the other shims; built
// the same way (PKG_CPPFLAGS=-I<repo>/include PKG_LIBS=-L<repo>/phylomap_amd -lphylomap_hip).
#include <Rcpp.h>

#include <vector>

#include "phylomap_hip.h"

using namespace Rcpp;

namespace {

void check(int32_t st) {
  if (st != PHM_OK) stop("phylomap_hip: %s: %s", phm_status_string(st), phm_last_error());
}

uint64_t seed_from_R() {                 // inside the RNGScope: set.seed() controls the result
  uint64_t hi = (uint64_t)(unif_rand() * 4294967296.0), lo = (uint64_t)(unif_rand() * 4294967296.0);
  return (hi << 32) | lo;
}

// the maps as R gets them: offsets as doubles (exact to 2^53), dwell, 1-based states
List maps_list(const std::vector<int64_t>& off, const std::vector<double>& dwell, const std::vector<int32_t>& state, int R, int E) {
  NumericVector o((int)off.size());
  for (size_t k = 0; k < off.size(); ++k) o[(long)k] = (double)off[k];
  NumericVector d((int)dwell.size());
  IntegerVector s((int)state.size());
  for (size_t k = 0; k < dwell.size(); ++k) { d[(long)k] = dwell[k]; s[(long)k] = state[k]; }
  return List::create(Named("off") = o, Named("dwell") = d, Named("state") = s, Named("n_hist") = R, Named("n_edge") = E);
}

// sizing call, then the filling call into arrays of the size it reported
template <typename Call>
List two_phase(Call call, int R, int E) {
  std::vector<int64_t> off((size_t)R * E + 1, 0);
  check(call(off.data(), 0, nullptr, nullptr));
  const int64_t total = off[(size_t)R * E];
  std::vector<double> dwell((size_t)(total > 0 ? total : 1));
  std::vector<int32_t> state(dwell.size());
  check(call(off.data(), total, dwell.data(), state.data()));
  dwell.resize((size_t)total);
  state.resize((size_t)total);
  return maps_list(off, dwell, state, R, E);
}

}  // namespace

// x: the tree (x$edge, x$edge.length, x$Nnode, length(x$states) are read); Q: n x n rate matrix; pid: root prior; R: number of
// histories; observe: n values in 1..n or a length-0 vector (identity).  Returns list(tips = R x n_tips, stats = R x
// (n + n*n + 1), nodes = R x (n_tips + Nnode), maps = list(off, dwell, state, n_hist, n_edge)) -- the maps hold TRUE states.
RcppExport SEXP phylomap_hip_simulate_maps(SEXP xSEXP, SEXP QSEXP, SEXP pidSEXP, SEXP RSEXP, SEXP observeSEXP) {
  BEGIN_RCPP
  RNGScope scope;
  List x = as<List>(xSEXP);
  IntegerMatrix e = as<IntegerMatrix>(x["edge"]);
  NumericVector el = as<NumericVector>(x["edge.length"]);
  IntegerVector st = as<IntegerVector>(x["states"]);
  NumericMatrix Q(QSEXP);
  NumericVector pid(pidSEXP);
  IntegerVector observe(observeSEXP);
  const int n = Q.nrow(), R = as<int>(RSEXP), T = (int)st.size(), Nn = as<int>(x["Nnode"]), E = e.nrow();
  if (R < 1) stop("R must be >= 1");
  if (observe.size() != 0 && observe.size() != n) stop("observe must have %d entries", n);
  if (pid.size() != n) stop("pid must have %d entries", n);
  std::vector<int32_t> edge(e.begin(), e.end());
  std::vector<double> len(el.begin(), el.end());
  phm_tree t = phm_tree();
  t.n_tips = T; t.n_node = Nn; t.n_edge = E;
  t.edge = edge.data(); t.edge_length = len.data();
  phm_options o = phm_options();
  o.seed = seed_from_R();
  o.device = -1;
  o.n_replicas = R;
  std::vector<int32_t> tips((size_t)R * T), nodes((size_t)R * (T + Nn));
  NumericMatrix stats(R, n + n * n + 1);
  const int32_t* obs = observe.size() ? observe.begin() : nullptr;
  List maps = two_phase([&](int64_t* off, int64_t cap, double* dw, int32_t* ms) {
    return phm_simulate_histories_maps(&t, n, Q.begin(), pid.begin(), obs, &o, tips.data(), nodes.data(), stats.begin(), off, cap, dw, ms);
  }, R, E);
  IntegerMatrix tm(R, T), nm(R, T + Nn);                             // replica-major -> R's column-major
  for (int r = 0; r < R; ++r) {
    for (int i = 0; i < T; ++i) tm.begin()[r + (size_t)R * i] = tips[(size_t)r * T + i];
    for (int i = 0; i < T + Nn; ++i) nm.begin()[r + (size_t)R * i] = nodes[(size_t)r * (T + Nn) + i];
  }
  return List::create(Named("tips") = tm, Named("stats") = stats, Named("nodes") = nm, Named("maps") = maps);
  END_RCPP
}

// sumstatEXP with the sampled histories: z the phylomap tree (x$edge, x$edge.length, x$Nnode, x$states, x$maps, x$mapnames);
// lefts / rights / d: eigen(Q) as R/sumstatEXP.R:26-29 computes it; rescale: the rescaled pruning pass.  Returns list(stats = N x
// (n + n(n-1)), maps = list(off, dwell, state, n_hist, n_edge)).
RcppExport SEXP phylomap_hip_exp_maps(SEXP xSEXP, SEXP QSEXP, SEXP pidSEXP, SEXP NSEXP, SEXP leftsSEXP, SEXP rightsSEXP, SEXP dSEXP,
                                      SEXP rescaleSEXP) {
  BEGIN_RCPP
  RNGScope scope;
  List x = as<List>(xSEXP);
  IntegerMatrix e = as<IntegerMatrix>(x["edge"]);
  NumericVector el = as<NumericVector>(x["edge.length"]);
  IntegerVector st = as<IntegerVector>(x["states"]);
  List maps_in = as<List>(x["maps"]), names_in = as<List>(x["mapnames"]);
  NumericMatrix Q(QSEXP), lefts(leftsSEXP), rights(rightsSEXP), d(dSEXP);
  NumericVector pid(pidSEXP);
  const int n = Q.nrow(), N = as<int>(NSEXP), T = (int)st.size(), Nn = as<int>(x["Nnode"]), E = e.nrow();
  if (N < 1) stop("N must be >= 1");
  if (pid.size() != n) stop("pid must have %d entries", n);
  std::vector<int32_t> edge(e.begin(), e.end()), states(st.begin(), st.end()), map_off(1, 0), mapnames;
  std::vector<double> len(el.begin(), el.end()), segs;
  for (int b = 0; b < E; ++b) {                                      // x$maps / x$mapnames flattened (phm_tree)
    NumericVector m = as<NumericVector>(maps_in[b]);
    IntegerVector mn = as<IntegerVector>(names_in[b]);
    if (mn.size() != m.size()) stop("x$maps and x$mapnames differ on edge row %d", b + 1);
    segs.insert(segs.end(), m.begin(), m.end());
    mapnames.insert(mapnames.end(), mn.begin(), mn.end());
    map_off.push_back((int32_t)segs.size());
  }
  std::vector<int32_t> nen((size_t)2 * Nn), nodelist((size_t)(Nn > 1 ? Nn - 1 : 1));
  int32_t root = 0;
  check(phm_tree_orders(T, E, edge.data(), nen.data(), nodelist.data(), &root));
  phm_tree t = phm_tree();
  t.n_tips = T; t.n_node = Nn; t.n_edge = E;
  t.edge = edge.data(); t.edge_length = len.data(); t.states = states.data();
  t.map_off = map_off.data(); t.maps = segs.data(); t.mapnames = mapnames.data();
  phm_options o = phm_options();
  o.seed = seed_from_R();
  o.device = -1;
  o.rescale_pruning = as<bool>(rescaleSEXP) ? 1 : 0;
  NumericMatrix out(N, n + n * (n - 1));
  List maps = two_phase([&](int64_t* off, int64_t cap, double* dw, int32_t* ms) {
    return phm_maketreelistEXP_maps(&t, n, Q.begin(), pid.begin(), nen.data(), nodelist.data(), root, N, lefts.begin(), rights.begin(),
                                    d.begin(), &o, out.begin(), off, cap, dw, ms);
  }, N, E);
  return List::create(Named("stats") = out, Named("maps") = maps);
  END_RCPP
}
