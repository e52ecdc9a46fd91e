// phylomap_mcmc_maps_shim.cpp -- `.Call` binding of phm_maketreelistMCMC_maps (include/phylomap_hip.h) behind sumstatMCMCmaps
// in shim/R/phylomap_mcmc_maps.R: the fixed-Q MCMC drivers with the chains' sampled histories at chosen iterations, one map per
// (history, edge row), in the list shape history_tree() (shim/R/phylomap_maps.R) reads.  Kept apart from phylomap_shim.cpp and
// phylomap_maps_shim.cpp; built the same way (PKG_CPPFLAGS=-I<repo>/include PKG_LIBS=-L<repo>/phylomap_amd -lphylomap_hip).
#include <Rcpp.h>

#include <string>
#include <vector>

#include "phylomap_hip.h"

using namespace Rcpp;

namespace {

void check(int32_t st) {
  if (st != PHM_OK) stop("phylomap_hip: %s: %s", phm_status_string(st), phm_last_error());
}

// the phylomap.hip.* options phylomap_shim.cpp reads (replicas, reduce, device, devices, rescale, mapping, cap_tail), and x$sites
struct Request {
  phm_options o;
  int S = 1;
  bool summed = true;
  std::vector<int32_t> site_states;
};

Request request_from_R(List x, int n_tips) {
  Request rq;
  phm_options& o = rq.o;
  o = phm_options();
  uint64_t hi = (uint64_t)(unif_rand() * 4294967296.0), lo = (uint64_t)(unif_rand() * 4294967296.0);   // inside the RNGScope
  o.seed = (hi << 32) | lo;
  Environment base("package:base");
  Function getOption = base["getOption"];
  o.device = as<int>(getOption("phylomap.hip.device", -1));
  IntegerVector devs = as<IntegerVector>(getOption("phylomap.hip.devices", IntegerVector(0)));
  if (devs.size() == 1 && devs[0] >= 1) {
    if (devs[0] > PHM_MAX_DEVICES) stop("phylomap.hip.devices: at most %d GPUs", (int)PHM_MAX_DEVICES);
    o.n_devices = devs[0];
    for (int d = 0; d < devs[0]; ++d) o.devices[d] = d;
  } else if (devs.size() > 1) {
    if (devs.size() > PHM_MAX_DEVICES) stop("phylomap.hip.devices: at most %d GPUs", (int)PHM_MAX_DEVICES);
    o.n_devices = (int32_t)devs.size();
    for (int d = 0; d < devs.size(); ++d) o.devices[d] = devs[d];
  }
  o.rescale_pruning = as<bool>(getOption("phylomap.hip.rescale", false)) ? 1 : 0;
  o.cap_tail = as<double>(getOption("phylomap.hip.cap_tail", 0.0));
  const std::string mp = as<std::string>(getOption("phylomap.hip.mapping", "auto"));
  if (mp == "auto") o.mapping = PHM_MAP_AUTO;
  else if (mp == "replicas") o.mapping = PHM_MAP_REPLICAS;
  else if (mp == "branches") o.mapping = PHM_MAP_BRANCHES;
  else if (mp == "tiles") o.mapping = PHM_MAP_TILES;
  else stop("phylomap.hip.mapping must be \"auto\", \"replicas\", \"branches\" or \"tiles\"");
  rq.S = as<int>(getOption("phylomap.hip.replicas", 1));
  rq.summed = as<bool>(getOption("phylomap.hip.reduce", true));
  if (x.containsElementNamed("sites")) {
    IntegerMatrix sites = as<IntegerMatrix>(x["sites"]);
    if (sites.ncol() != n_tips) stop("x$sites must have one column per tip (%d), it has %d", n_tips, sites.ncol());
    rq.S = sites.nrow();
    rq.site_states.resize((size_t)rq.S * n_tips);
    for (int s = 0; s < rq.S; ++s)
      for (int t = 0; t < n_tips; ++t) rq.site_states[(size_t)s * n_tips + t] = sites.begin()[s + (size_t)rq.S * t];
    o.tips_per_replica = 1;
  }
  if (rq.S < 1) stop("phylomap.hip.replicas must be >= 1");
  o.n_replicas = rq.S;
  o.reduce = (rq.S > 1 && rq.summed) ? 1 : 0;
  return rq;
}

}  // namespace

// z: the phylomap tree; Q: n x n rate matrix; pid: root prior; Omega; N sweeps; map_iters: 0-based recorded iterations, increasing
// (length 0: every iteration); variant: "plain", "bigtree", "sparse", "ks" or "bf".  Returns list(stats, maps): stats as the
// plain driver's (an N x cols matrix, or a list of S of them with options(phylomap.hip.reduce = FALSE)), maps = list(off, dwell,
// state, n_hist, n_edge) with history h = s * J + j (0-based) = chain s at the j-th recorded iteration.
RcppExport SEXP phylomap_hip_mcmc_maps(SEXP xSEXP, SEXP QSEXP, SEXP pidSEXP, SEXP OmegaSEXP, SEXP NSEXP, SEXP itersSEXP,
                                       SEXP variantSEXP) {
  BEGIN_RCPP
  RNGScope scope;
  List x = as<List>(xSEXP);
  IntegerMatrix e = as<IntegerMatrix>(x["edge"]);
  NumericVector el = as<NumericVector>(x["edge.length"]);
  IntegerVector st = as<IntegerVector>(x["states"]);
  List maps_in = as<List>(x["maps"]), names_in = as<List>(x["mapnames"]);
  NumericMatrix Q(QSEXP);
  NumericVector pid(pidSEXP);
  IntegerVector iters(itersSEXP);
  const double Omega = as<double>(OmegaSEXP);
  const std::string vname = as<std::string>(variantSEXP);
  const int n = Q.nrow(), N = as<int>(NSEXP), T = (int)st.size(), Nn = as<int>(x["Nnode"]), E = e.nrow();
  if (N < 1) stop("N must be >= 1");
  if (pid.size() != n) stop("pid must have %d entries", n);
  int variant = PHM_MCMC, cols = n + n * (n - 1);
  if (vname == "plain") variant = PHM_MCMC;
  else if (vname == "bigtree") variant = PHM_MCMC_BIGTREE;
  else if (vname == "sparse") variant = PHM_MCMC_SPARSE;
  else if (vname == "ks") { variant = PHM_MCMC_KS; cols = n + n * n + 2 + 3 * (n / 2 - 1) + 1; }
  else if (vname == "bf") { variant = PHM_MCMC_BF; cols = n + n * n + 3; }
  else stop("variant must be \"plain\", \"bigtree\", \"sparse\", \"ks\" or \"bf\"");
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
  Request rq = request_from_R(x, T);
  phm_tree t = phm_tree();
  t.n_tips = T; t.n_node = Nn; t.n_edge = E;
  t.edge = edge.data(); t.edge_length = len.data(); t.states = rq.site_states.empty() ? states.data() : rq.site_states.data();
  t.map_off = map_off.data(); t.maps = segs.data(); t.mapnames = mapnames.data();
  std::vector<double> B((size_t)n * n);                              // B = I + Q / Omega (R/sumstatMCMC.R:25), column-major
  for (int i = 0; i < n * n; ++i) B[i] = Q.begin()[i] / Omega + ((i % (n + 1)) == 0 ? 1.0 : 0.0);
  std::vector<int32_t> its(iters.begin(), iters.end());
  const int J = its.empty() ? N : (int)its.size();
  const int S = rq.S;
  const bool single = S == 1 || rq.summed;
  std::vector<double> buf((size_t)N * cols * (single ? 1 : S));
  auto call = [&](int64_t* off, int64_t cap, double* dw, int32_t* ms) {
    return phm_maketreelistMCMC_maps(variant, &t, n, Q.begin(), pid.begin(), B.data(), Omega, nen.data(), nodelist.data(), root, N,
                                     its.empty() ? nullptr : its.data(), (int32_t)its.size(), &rq.o, buf.data(), off, cap, dw, ms);
  };
  const size_t rows = (size_t)S * J * E;
  std::vector<int64_t> off(rows + 1, 0);
  check(call(off.data(), 0, nullptr, nullptr));                      // sizing, then filling into arrays of the size it reported
  const int64_t total = off[rows];
  std::vector<double> dwell((size_t)(total > 0 ? total : 1));
  std::vector<int32_t> state(dwell.size());
  check(call(off.data(), total, dwell.data(), state.data()));
  NumericVector o((int)off.size());
  for (size_t k = 0; k < off.size(); ++k) o[(long)k] = (double)off[k];
  NumericVector d((int)total);
  IntegerVector s((int)total);
  for (int64_t k = 0; k < total; ++k) { d[(long)k] = dwell[k]; s[(long)k] = state[k]; }
  List maps = List::create(Named("off") = o, Named("dwell") = d, Named("state") = s, Named("n_hist") = S * J, Named("n_edge") = E);
  SEXP stats;
  if (single) {
    NumericMatrix m(N, cols);
    std::copy(buf.begin(), buf.begin() + (size_t)N * cols, m.begin());
    stats = m;
  } else {
    List res(S);
    for (int r = 0; r < S; ++r) {
      NumericMatrix m(N, cols);
      std::copy(buf.begin() + (size_t)r * N * cols, buf.begin() + (size_t)(r + 1) * N * cols, m.begin());
      res[r] = m;
    }
    stats = res;
  }
  return List::create(Named("stats") = stats, Named("maps") = maps);
  END_RCPP
}
