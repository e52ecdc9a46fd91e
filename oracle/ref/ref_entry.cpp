// C entry points to the reference's own src/phylomap.cpp, compiled unchanged against the stand-in headers of oracle/ref/stub/.
// TEST INFRASTRUCTURE: built by oracle/ref_build.sh into oracle/_ref/libphm_ref.so where the reference tree is present, loaded by
// tests/ref_lib.py only.  The reference's translation unit is pulled in by the #include below (the build passes its directory
// with -I), so its file-local functions and its Branch type are in scope without restating a line of it.
//
// The wrappers take the flat arrays of orc_tree and of the orc_maketreelist* drivers (oracle/phm_oracle.h), build the R objects the
// reference reads, seed the R stream (set.seed(seed) as restated in the oracle), call the reference and copy the result out
// column-major.  A C++ exception comes back as a status: REF_SAMPLE for RcppArmadillo::sample's range_error (no positive
// probability, ...), REF_INDEX for an out-of-range element access, REF_OTHER for anything else.
#include <phylomap.cpp>

#include "../phm_oracle.h"

enum { REF_OK = 0, REF_SAMPLE = 1, REF_INDEX = 2, REF_OTHER = 3 };

namespace {

template <class F> int guarded(F f) {
  try { f(); return REF_OK; }
  catch (const std::range_error&) { return REF_SAMPLE; }
  catch (const std::out_of_range&) { return REF_INDEX; }
  catch (const std::logic_error&) { return REF_INDEX; }
  catch (...) { return REF_OTHER; }
}

NumericVector nvec(const double* p, long n) { return NumericVector(p, p + n); }
IntegerVector ivec(const int32_t* p, long n) { return IntegerVector(p, p + n); }
NumericMatrix nmat_cm(const double* p, int r, int c) { NumericMatrix m(r, c); std::copy(p, p + (size_t)r * c, m.begin()); return m; }
IntegerMatrix imat_cm(const int32_t* p, int r, int c) { IntegerMatrix m(r, c); std::copy(p, p + (size_t)r * c, m.begin()); return m; }
IntegerMatrix imat_rm(const int32_t* p, int r, int c) {
  IntegerMatrix m(r, c);
  for (int i = 0; i < r; ++i) for (int j = 0; j < c; ++j) m(i, j) = p[(size_t)i * c + j];
  return m;
}
arma::mat amat_rm(const double* p, int r, int c) {
  arma::mat m(r, c);
  for (int i = 0; i < r; ++i) for (int j = 0; j < c; ++j) m(i, j) = p[(size_t)i * c + j];
  return m;
}
void out_rm(const arma::mat& m, double* p) {
  for (arma::uword i = 0; i < m.n_rows; ++i) for (arma::uword j = 0; j < m.n_cols; ++j) p[(size_t)i * m.n_cols + j] = m(i, j);
}

// the phylomap tree object: the fields the drivers read (x$maps, x$mapnames, x$edge, x$Nnode, x$states, x$node.states, x$edge.length)
List tree_object(const orc_tree* x) {
  List maps, mapnames;
  for (int b = 0; b < x->n_edge; ++b) {
    const int o = x->map_off[b], m = x->map_off[b + 1] - o;
    maps.push_back(nvec(x->maps + o, m).sexp());
    mapnames.push_back(ivec(x->mapnames + o, m).sexp());
  }
  List z;
  z["maps"] = maps;
  z["mapnames"] = mapnames;
  z["edge"] = imat_cm(x->edge, x->n_edge, 2);
  z["Nnode"] = (int)x->n_node;
  z["states"] = ivec(x->states, x->n_tips);
  IntegerMatrix ns(x->n_edge, 2);
  std::fill(ns.begin(), ns.end(), 1);
  z["node.states"] = ns;
  if (x->edge_length) z["edge.length"] = nvec(x->edge_length, x->n_edge);
  return z;
}

int copy_out(const NumericMatrix& r, int N, int cols, double* out) {
  if (r.nrow() != N || r.ncol() != cols) return REF_OTHER;
  std::copy(r.begin(), r.end(), out);
  return REF_OK;
}

arma::mat tips_PL(const orc_tree* x, int n) {
  arma::mat PL(2 * x->n_node + 1, n);
  for (int i = 0; i < x->n_tips; ++i) PL(i, x->states[i] - 1) = 1;
  return PL;
}

}  // namespace

extern "C" {

long ref_rcout_lines(void) { return Rcpp::phm_stub_rcout_counter(); }

// driver: the ORC_MCMC_* variant (PLAIN, BIGTREE, SPARSE, KS, BF), + 16 for the DIC twin of KS / BF.  out: N x cols, column-major.
int ref_maketreelistMCMC(int driver, const orc_tree* x, int n, const double* Q_cm, const double* pid, const double* B_cm, double Omega,
                         const int32_t* nen, const int32_t* nodelist, int root, int N, const double* prior, int nprior,
                         uint32_t seed, double* out, int cols) {
  int copied = REF_OK;
  int rc = guarded([&] {
    List z = tree_object(x);
    NumericMatrix Q = nmat_cm(Q_cm, n, n), B = nmat_cm(B_cm, n, n);
    NumericVector p = nvec(pid, n), pr = nvec(prior, prior ? nprior : 0);
    IntegerVector ne = ivec(nen, 2 * x->n_node), nl = ivec(nodelist, x->n_node - 1);
    orc_r_set_seed(seed);
    NumericMatrix r;
    switch (driver) {
      case ORC_MCMC_PLAIN:   r = maketreelistMCMC(z, Q, p, B, Omega, ne, nl, root, N); break;
      case ORC_MCMC_BIGTREE: r = maketreelistMCMC_bigtree(z, Q, p, B, Omega, ne, nl, root, N); break;
      case ORC_MCMC_SPARSE:  r = SPARSEmaketreelistMCMC(z, Q, p, B, Omega, ne, nl, root, N); break;
      case ORC_MCMC_KS:      r = maketreelistMCMCks(z, Q, p, B, Omega, ne, nl, root, N, pr); break;
      case ORC_MCMC_BF:      r = maketreelistMCMCbf(z, Q, p, B, Omega, ne, nl, root, N, pr); break;
      case ORC_MCMC_KS + 16: r = maketreelistMCMCksDICt(z, Q, p, B, Omega, ne, nl, root, N, pr); break;
      case ORC_MCMC_BF + 16: r = maketreelistMCMC2sDICt(z, Q, p, B, Omega, ne, nl, root, N, pr); break;
      default: throw std::runtime_error("unknown driver");
    }
    copied = copy_out(r, N, cols, out);
  });
  return rc ? rc : copied;
}

// variant: ORC_MCMC_MT or ORC_MCMC_KSMT.  nen_m / nodelist_m: one row per tree, row-major.
int ref_maketreelistMCMCmt(int variant, const orc_tree* const* xs, int treecount, int n, const double* Q_cm, const double* pid,
                           const double* B_cm, double Omega, const int32_t* nen_m, const int32_t* nodelist_m, const int32_t* roots,
                           int N, const double* prior, int nprior, uint32_t seed, double* out, int cols) {
  int copied = REF_OK;
  int rc = guarded([&] {
    List zs;
    for (int j = 0; j < treecount; ++j) zs.push_back(tree_object(xs[j]).sexp());
    const int Nnode = xs[0]->n_node;
    NumericMatrix Q = nmat_cm(Q_cm, n, n), B = nmat_cm(B_cm, n, n);
    NumericVector p = nvec(pid, n), pr = nvec(prior, nprior);
    IntegerMatrix ne = imat_rm(nen_m, treecount, 2 * Nnode), nl = imat_rm(nodelist_m, treecount, Nnode - 1);
    IntegerVector rt = ivec(roots, treecount);
    orc_r_set_seed(seed);
    NumericMatrix r = (variant == ORC_MCMC_KSMT) ? maketreelistMCMCksmt(zs, Q, p, B, Omega, ne, nl, rt, N, pr)
                                                  : maketreelistMCMCmt(zs, Q, p, B, Omega, ne, nl, rt, N, pr);
    copied = copy_out(r, N, cols, out);
  });
  return rc ? rc : copied;
}

int ref_maketreelistEXP(const orc_tree* x, int n, const double* Q_cm, const double* pid, const int32_t* nen, const int32_t* nodelist,
                        int root, int N, const double* lefts_cm, const double* rights_cm, const double* d_cm, uint32_t seed,
                        double* out, int cols) {
  int copied = REF_OK;
  int rc = guarded([&] {
    List z = tree_object(x);
    NumericMatrix Q = nmat_cm(Q_cm, n, n), L = nmat_cm(lefts_cm, n, n), R = nmat_cm(rights_cm, n, n), D = nmat_cm(d_cm, n, n);
    NumericVector p = nvec(pid, n);
    IntegerVector ne = ivec(nen, 2 * x->n_node), nl = ivec(nodelist, x->n_node - 1);
    orc_r_set_seed(seed);
    NumericMatrix r = maketreelistEXP(z, Q, p, ne, nl, root, N, L, R, D);
    copied = copy_out(r, N, cols, out);
  });
  return rc ? rc : copied;
}

// ---- per-function entry points, mirroring orc_shortener / orc_matTospmat / orc_makePL / orc_makePLexp / orc_matexp -------------
// d, s (0-based states) of length m in and out; *m_out the new length; stats_row (n + n(n-1) values, bf: n + n*n) gets += counts
int ref_shortener(double* d, int32_t* s, int m, int n, int bf, double* stats_row, int* m_out) {
  return guarded([&] {
    std::vector<int> s1(s, s + m);
    for (int& v : s1) v += 1;                                  // makeabranch takes 1-based names
    Branch b = makeabranch(nvec(d, m), IntegerVector(s1.begin(), s1.end()));
    const int cols = bf ? n + n * n : n + n * (n - 1);
    arma::mat dw = amat_rm(stats_row, 1, cols);
    if (bf) shortenerbf(&b, &dw, n, 0); else shortener(&b, &dw, n, 0);
    int k = 0;
    std::list<int>::iterator nit = b.names.begin();
    for (std::list<double>::iterator bit = b.branch.begin(); bit != b.branch.end(); ++bit, ++nit, ++k) { d[k] = *bit; s[k] = *nit; }
    *m_out = k;
    out_rm(dw, stats_row);
  });
}

int ref_matTospmat(const double* B_rm, int n, double* out_rm_) {
  return guarded([&] {
    arma::sp_mat A = matTospmat(amat_rm(B_rm, n, n));
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) out_rm_[(size_t)i * n + j] = A(i, j);
  });
}

// kind 0 makePLrcpp, 1 makePLrcpp_bigtree, 2 SPARSEmakePLrcpp (on matTospmat(B)), 3 makePLnormalized.  B, PL row-major.
int ref_makePL(int kind, const orc_tree* x, int n, const double* B_rm, const int32_t* nen, const int32_t* seg_count, double* PL_rm) {
  return guarded([&] {
    arma::mat PL = tips_PL(x, n), B2 = amat_rm(B_rm, n, n);
    arma::imat edge = as<arma::imat>(imat_cm(x->edge, x->n_edge, 2));
    arma::irowvec edge1 = trans(edge.col(0)), edge2 = trans(edge.col(1));
    arma::irowvec ne = as<arma::irowvec>(ivec(nen, 2 * x->n_node)), bl = as<arma::irowvec>(ivec(seg_count, x->n_edge));
    arma::sp_mat B3 = matTospmat(B2);
    if (kind == 0) makePLrcpp(&edge1, &edge2, x->n_node, &PL, &ne, &B2, bl);
    else if (kind == 1) makePLrcpp_bigtree(&edge1, &edge2, x->n_node, &PL, &ne, &B2, bl);
    else if (kind == 2) SPARSEmakePLrcpp(&edge1, &edge2, x->n_node, &PL, &ne, &B3, bl);
    else makePLnormalized(&edge1, &edge2, x->n_node, &PL, &ne, &B2, bl);
    out_rm(PL, PL_rm);
  });
}

// P_rm: n_edge matrices n x n, row-major
int ref_makePLexp(const orc_tree* x, int n, const double* P_rm, const int32_t* nen, double* PL_rm) {
  return guarded([&] {
    arma::mat PL = tips_PL(x, n);
    arma::imat edge = as<arma::imat>(imat_cm(x->edge, x->n_edge, 2));
    arma::irowvec edge1 = trans(edge.col(0)), edge2 = trans(edge.col(1));
    arma::irowvec states = as<arma::irowvec>(ivec(x->states, x->n_tips));
    IntegerVector ne = ivec(nen, 2 * x->n_node);
    arma::cube TP(n, n, x->n_edge);
    for (int b = 0; b < x->n_edge; ++b) TP.slice(b) = amat_rm(P_rm + (size_t)b * n * n, n, n);
    makePLexp(&states, x->n_node, &edge1, &edge2, &ne, &TP, &PL);
    out_rm(PL, PL_rm);
  });
}

// abs(matexp(left, right, diag(dvals), t)) as the drivers use it (:2980, :3042); row-major in and out
int ref_matexp(const double* L_rm, const double* R_rm, const double* dvals, int n, double t, double* P_rm) {
  return guarded([&] {
    arma::mat D(n, n);
    for (int i = 0; i < n; ++i) D(i, i) = dvals[i];
    out_rm(abs(matexp(amat_rm(L_rm, n, n), amat_rm(R_rm, n, n), D, t)), P_rm);
  });
}

int ref_sampleOnce(const double* w, int n, double u, int* index) {
  return guarded([&] { *index = sampleOnce(as<arma::colvec>(nvec(w, n)), u); });
}

// set.seed(seed); sample(0:(n-1), 1, TRUE, p)
int ref_sample(const double* p, int n, uint32_t seed, int* index) {
  return guarded([&] {
    IntegerVector sts(n);
    for (int i = 0; i < n; ++i) sts[i] = i;
    orc_r_set_seed(seed);
    *index = as<int>(RcppArmadillo::sample(sts, 1, 1, nvec(p, n)));
  });
}

// set.seed(seed); runif(nu); rexp(ne, rate): the sugar's call semantics on top of the oracle's generators
int ref_runif_rexp(uint32_t seed, int nu, int ne, double rate, double* u_out, double* e_out) {
  return guarded([&] {
    orc_r_set_seed(seed);
    NumericVector u = runif(nu), e = rexp(ne, rate);
    std::copy(u.begin(), u.end(), u_out);
    std::copy(e.begin(), e.end(), e_out);
  });
}

}  // extern "C"
