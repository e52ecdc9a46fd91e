// Stand-in for <RcppArmadillo.h>: the part of Armadillo's surface that the reference's src/phylomap.cpp uses, as eager value types
// with column-major storage and plain loops, plus the as<> / wrap glue between them and the Rcpp stand-in.  Written from scratch.
// TEST INFRASTRUCTURE; oracle/ref/README.md lists every summation order and conversion chosen here and where it comes from.
//
// Every expression is evaluated at once into a Mat (no expression templates), element access is bounds-checked and throws
// std::logic_error as Armadillo's checked accessors do, and products accumulate left to right starting from the first term
// (what Armadillo's gemv_emul_tinysq / gemm_emul_tinysq do for square matrices up to 4 x 4; beyond that Armadillo calls BLAS,
// whose order is not knowable, and this stand-in keeps the plain order).
#ifndef PHM_STUB_RCPPARMADILLO_H
#define PHM_STUB_RCPPARMADILLO_H

#include "Rcpp.h"

extern "C" int orc_expmat_pade(const double* A_rm, int n, double* out_rm);

namespace arma {

typedef unsigned int uword;      // RcppArmadillo builds Armadillo with 32-bit words
typedef int sword;

inline void phm_check(bool bad, const char* what) { if (bad) throw std::logic_error(what); }

template <class T> class subview;
template <class T> class Col;
template <class T> class Row;

template <class T> class Mat {
  std::vector<T> own_;
  T* aux_ = nullptr;             // memory of somebody else (the copy_aux_mem = false constructor)
 protected:
  void init(uword r, uword c) { own_.assign((size_t)r * c, T(0)); aux_ = nullptr; n_rows = r; n_cols = c; n_elem = r * c; }
 public:
  typedef T elem_type;
  uword n_rows = 0, n_cols = 0, n_elem = 0;
  Mat() {}
  Mat(uword r, uword c) { init(r, c); }
  Mat(T* aux, uword r, uword c, bool copy_aux_mem = true, bool = false) {
    if (copy_aux_mem) { init(r, c); std::copy(aux, aux + (size_t)r * c, own_.begin()); }
    else { aux_ = aux; n_rows = r; n_cols = c; n_elem = r * c; }
  }
  Mat(const Mat& o) : own_(o.memptr(), o.memptr() + o.n_elem), n_rows(o.n_rows), n_cols(o.n_cols), n_elem(o.n_elem) {}
  Mat& operator=(const Mat& o) {
    if (this == &o) return *this;
    if (aux_ && o.n_rows == n_rows && o.n_cols == n_cols) { std::copy(o.memptr(), o.memptr() + n_elem, aux_); return *this; }
    std::vector<T> tmp(o.memptr(), o.memptr() + o.n_elem);      // o may be a view of *this
    own_.swap(tmp); aux_ = nullptr; n_rows = o.n_rows; n_cols = o.n_cols; n_elem = o.n_elem;
    return *this;
  }
  virtual ~Mat() {}
  T* memptr() { return aux_ ? aux_ : own_.data(); }
  const T* memptr() const { return aux_ ? aux_ : own_.data(); }
  T* begin() { return memptr(); }
  T* end() { return memptr() + n_elem; }
  uword size() const { return n_elem; }
  T& at(uword i, uword j) { return memptr()[(size_t)i + (size_t)j * n_rows]; }
  const T& at(uword i, uword j) const { return memptr()[(size_t)i + (size_t)j * n_rows]; }
  T& operator()(uword i, uword j) { phm_check(i >= n_rows || j >= n_cols, "Mat::operator(): index out of bounds"); return at(i, j); }
  const T& operator()(uword i, uword j) const { phm_check(i >= n_rows || j >= n_cols, "Mat::operator(): index out of bounds"); return at(i, j); }
  T& operator()(uword i) { phm_check(i >= n_elem, "Mat::operator(): index out of bounds"); return memptr()[i]; }
  const T& operator()(uword i) const { phm_check(i >= n_elem, "Mat::operator(): index out of bounds"); return memptr()[i]; }
  T& operator[](uword i) { return (*this)(i); }
  const T& operator[](uword i) const { return (*this)(i); }
  Mat& zeros() { std::fill(memptr(), memptr() + n_elem, T(0)); return *this; }
  Mat& ones() { std::fill(memptr(), memptr() + n_elem, T(1)); return *this; }
  Mat& eye() { zeros(); for (uword i = 0; i < n_rows && i < n_cols; ++i) at(i, i) = T(1); return *this; }
  subview<T> row(uword i) { phm_check(i >= n_rows, "Mat::row(): index out of bounds"); return subview<T>(*this, i, 0, 1, n_cols); }
  subview<T> col(uword j) { phm_check(j >= n_cols, "Mat::col(): index out of bounds"); return subview<T>(*this, 0, j, n_rows, 1); }
  Mat row(uword i) const { return const_cast<Mat*>(this)->row(i); }
  Mat col(uword j) const { return const_cast<Mat*>(this)->col(j); }
  Col<T> diag() const;
  Mat t() const { Mat o(n_cols, n_rows); for (uword j = 0; j < n_cols; ++j) for (uword i = 0; i < n_rows; ++i) o.at(j, i) = at(i, j); return o; }
};

// a rectangular window of a Mat that can be read (converts to Mat) and assigned to
template <class T> class subview {
  Mat<T>& m_; uword r0_, c0_;
 public:
  uword n_rows, n_cols, n_elem;
  subview(Mat<T>& m, uword r0, uword c0, uword nr, uword nc) : m_(m), r0_(r0), c0_(c0), n_rows(nr), n_cols(nc), n_elem(nr * nc) {}
  operator Mat<T>() const {
    Mat<T> o(n_rows, n_cols);
    for (uword j = 0; j < n_cols; ++j) for (uword i = 0; i < n_rows; ++i) o.at(i, j) = m_.at(r0_ + i, c0_ + j);
    return o;
  }
  subview& operator=(const Mat<T>& v) {
    phm_check(v.n_rows != n_rows || v.n_cols != n_cols, "copy into submatrix: incompatible matrix dimensions");
    Mat<T> tmp(v);                                                  // v may alias the parent
    for (uword j = 0; j < n_cols; ++j) for (uword i = 0; i < n_rows; ++i) m_.at(r0_ + i, c0_ + j) = tmp.at(i, j);
    return *this;
  }
  subview& operator=(const subview& v) { return *this = Mat<T>(v); }
  Mat<T> t() const { return Mat<T>(*this).t(); }
  uword size() const { return n_elem; }
  T& operator()(uword i) {
    phm_check(i >= n_elem, "subview::operator(): index out of bounds");
    return n_rows == 1 ? m_.at(r0_, c0_ + i) : m_.at(r0_ + i % n_rows, c0_ + i / n_rows);
  }
  T& operator()(uword i, uword j) { phm_check(i >= n_rows || j >= n_cols, "subview::operator(): index out of bounds"); return m_.at(r0_ + i, c0_ + j); }
};

template <class T> class Col : public Mat<T> {
 public:
  Col() {}
  explicit Col(uword n) : Mat<T>(n, 1) {}
  Col(const Mat<T>& m) : Mat<T>(m) { phm_check(m.n_elem > 0 && m.n_cols != 1, "Mat::init(): requested size is not compatible with column vector layout"); }
  Col(const subview<T>& s) : Col(Mat<T>(s)) {}
  Col(const Rcpp::Vector<T>& v) : Mat<T>(v.begin(), (uword)v.size(), 1, true) {}     // RcppArmadillo's Col(VectorBase) extension
  Col& operator=(const Mat<T>& m) { phm_check(m.n_elem > 0 && m.n_cols != 1, "Mat::init(): requested size is not compatible with column vector layout"); Mat<T>::operator=(m); return *this; }
};
template <class T> class Row : public Mat<T> {
 public:
  Row() {}
  explicit Row(uword n) : Mat<T>(1, n) {}
  Row(const Mat<T>& m) : Mat<T>(m) { phm_check(m.n_elem > 0 && m.n_rows != 1, "Mat::init(): requested size is not compatible with row vector layout"); }
  Row(const subview<T>& s) : Row(Mat<T>(s)) {}
  Row(const Rcpp::Vector<T>& v) : Mat<T>(v.begin(), 1, (uword)v.size(), true) {}     // RcppArmadillo's Row(VectorBase) extension
  Row& operator=(const Mat<T>& m) { phm_check(m.n_elem > 0 && m.n_rows != 1, "Mat::init(): requested size is not compatible with row vector layout"); Mat<T>::operator=(m); return *this; }
};
template <class T> Col<T> Mat<T>::diag() const {
  const uword k = n_rows < n_cols ? n_rows : n_cols;
  Col<T> o(k);
  for (uword i = 0; i < k; ++i) o.at(i, 0) = at(i, i);
  return o;
}

typedef Mat<double> mat;
typedef Col<double> vec;
typedef Col<double> colvec;
typedef Row<double> rowvec;
typedef Mat<sword> imat;
typedef Row<sword> irowvec;
typedef Col<sword> ivec;

template <class T> class Cube {
  std::vector<Mat<T> > s_;
 public:
  uword n_rows = 0, n_cols = 0, n_slices = 0;
  Cube() {}
  Cube(uword r, uword c, uword s) : s_(s, Mat<T>(r, c)), n_rows(r), n_cols(c), n_slices(s) {}
  Cube& zeros() { for (Mat<T>& m : s_) m.zeros(); return *this; }
  Mat<T>& slice(uword k) { phm_check(k >= n_slices, "Cube::slice(): index out of bounds"); return s_[k]; }
  const Mat<T>& slice(uword k) const { phm_check(k >= n_slices, "Cube::slice(): index out of bounds"); return s_[k]; }
  T& operator()(uword i, uword j, uword k) { phm_check(k >= n_slices, "Cube::operator(): index out of bounds"); return s_[k](i, j); }
  void insert_slices(uword at, uword count, bool = true) {
    phm_check(at > n_slices, "Cube::insert_slices(): index out of bounds");
    s_.insert(s_.begin() + at, count, Mat<T>(n_rows, n_cols));
    n_slices += count;
  }
};
typedef Cube<double> cube;

// sparse matrix: dense storage, but products visit the stored (non-zero) entries only, column by column, as a
// compressed-column product does
template <class T> class SpMat {
  std::vector<T> d_;
 public:
  uword n_rows = 0, n_cols = 0;
  SpMat() {}
  SpMat(uword r, uword c) : d_((size_t)r * c, T(0)), n_rows(r), n_cols(c) {}
  T& operator()(uword i, uword j) { phm_check(i >= n_rows || j >= n_cols, "SpMat::operator(): index out of bounds"); return d_[(size_t)i + (size_t)j * n_rows]; }
  const T& at(uword i, uword j) const { return d_[(size_t)i + (size_t)j * n_rows]; }
};
typedef SpMat<double> sp_mat;

template <class M> M zeros(uword n) { M m(n); m.zeros(); return m; }
template <class M> M zeros(uword r, uword c) { M m(r, c); m.zeros(); return m; }
template <class M> M ones(uword n) { M m(n); m.ones(); return m; }
template <class M> M ones(uword r, uword c) { M m(r, c); m.ones(); return m; }

inline mat trans(const mat& a) { return a.t(); }
inline imat trans(const imat& a) { return a.t(); }

// C(i,j) = ((A(i,0) B(0,j) + A(i,1) B(1,j)) + A(i,2) B(2,j)) + ...
inline mat operator*(const mat& a, const mat& b) {
  phm_check(a.n_cols != b.n_rows, "matrix multiplication: incompatible matrix dimensions");
  mat c(a.n_rows, b.n_cols);
  for (uword j = 0; j < b.n_cols; ++j)
    for (uword i = 0; i < a.n_rows; ++i) {
      if (a.n_cols == 0) continue;
      double acc = a.at(i, 0) * b.at(0, j);
      for (uword k = 1; k < a.n_cols; ++k) acc += a.at(i, k) * b.at(k, j);
      c.at(i, j) = acc;
    }
  return c;
}
inline mat operator*(const sp_mat& a, const mat& b) {
  phm_check(a.n_cols != b.n_rows, "matrix multiplication: incompatible matrix dimensions");
  mat c(a.n_rows, b.n_cols);
  for (uword j = 0; j < b.n_cols; ++j)
    for (uword k = 0; k < a.n_cols; ++k)
      for (uword i = 0; i < a.n_rows; ++i) if (a.at(i, k) != 0.0) c.at(i, j) += a.at(i, k) * b.at(k, j);
  return c;
}
inline mat operator*(const mat& a, const sp_mat& b) {
  phm_check(a.n_cols != b.n_rows, "matrix multiplication: incompatible matrix dimensions");
  mat c(a.n_rows, b.n_cols);
  for (uword j = 0; j < b.n_cols; ++j)
    for (uword k = 0; k < b.n_rows; ++k) if (b.at(k, j) != 0.0)
      for (uword i = 0; i < a.n_rows; ++i) c.at(i, j) += a.at(i, k) * b.at(k, j);
  return c;
}
inline mat operator*(const mat& a, double s) { mat c(a); for (uword i = 0; i < c.n_elem; ++i) c(i) = a(i) * s; return c; }
inline mat operator*(double s, const mat& a) { mat c(a); for (uword i = 0; i < c.n_elem; ++i) c(i) = s * a(i); return c; }
inline mat operator/(const mat& a, double s) { mat c(a); for (uword i = 0; i < c.n_elem; ++i) c(i) = a(i) / s; return c; }
inline mat operator%(const mat& a, const mat& b) {
  phm_check(a.n_rows != b.n_rows || a.n_cols != b.n_cols, "element-wise multiplication: incompatible matrix dimensions");
  mat c(a); for (uword i = 0; i < c.n_elem; ++i) c(i) = a(i) * b(i); return c;
}
inline mat operator+(const mat& a, const mat& b) {
  phm_check(a.n_rows != b.n_rows || a.n_cols != b.n_cols, "addition: incompatible matrix dimensions");
  mat c(a); for (uword i = 0; i < c.n_elem; ++i) c(i) = a(i) + b(i); return c;
}
// sum of a vector, left to right from the first element (oracle/ref/README.md: Armadillo's own accumulation order is an assumption)
inline double sum(const mat& a) {
  phm_check(a.n_rows != 1 && a.n_cols != 1, "sum(): the stand-in sums vectors only");
  if (a.n_elem == 0) return 0.0;
  double s = a(0);
  for (uword i = 1; i < a.n_elem; ++i) s += a(i);
  return s;
}
inline double min(const mat& a) {
  phm_check(a.n_elem == 0, "min(): object has no elements");
  double m = a(0);
  for (uword i = 1; i < a.n_elem; ++i) if (a(i) < m) m = a(i);
  return m;
}
inline mat abs(const mat& a) { mat c(a); for (uword i = 0; i < c.n_elem; ++i) c(i) = std::fabs(a(i)); return c; }
// expmat: not a second restatement of Armadillo's Pade routine -- it forwards to the oracle's (orc_expmat_pade), so the DIC
// drivers' log-likelihood column is pinned around expmat, not through it
inline mat expmat(const mat& a) {
  phm_check(a.n_rows != a.n_cols, "expmat(): given matrix must be square sized");
  const uword n = a.n_rows;
  std::vector<double> in((size_t)n * n), out((size_t)n * n);
  for (uword i = 0; i < n; ++i) for (uword j = 0; j < n; ++j) in[(size_t)i * n + j] = a.at(i, j);
  if (orc_expmat_pade(in.data(), (int)n, out.data())) throw std::runtime_error("expmat(): singular system");
  mat c(n, n);
  for (uword i = 0; i < n; ++i) for (uword j = 0; j < n; ++j) c.at(i, j) = out[(size_t)i * n + j];
  return c;
}

}  // namespace arma

namespace Rcpp {

template <class T> struct ArmaExport {
  static arma::Mat<T> matrix(const SEXP& s) {
    SEXP c = coerce_to<T>(s);
    if (c->nrow < 0) throw not_compatible("not a matrix");
    std::vector<T>& d = sexp_store<T>::of(*c);
    return arma::Mat<T>(d.data(), (arma::uword)c->nrow, (arma::uword)c->ncol, true);
  }
  static std::vector<T>& flat(const SEXP& c) { return sexp_store<T>::of(*c); }
};
template <class T> struct Exporter<arma::Mat<T> > { static arma::Mat<T> get(const SEXP& s) { return ArmaExport<T>::matrix(s); } };
template <class T> struct Exporter<arma::Row<T> > {
  static arma::Row<T> get(const SEXP& s) {
    SEXP c = coerce_to<T>(s);
    std::vector<T>& d = ArmaExport<T>::flat(c);
    return arma::Row<T>(arma::Mat<T>(d.data(), 1, (arma::uword)d.size(), true));
  }
};
template <class T> struct Exporter<arma::Col<T> > {
  static arma::Col<T> get(const SEXP& s) {
    SEXP c = coerce_to<T>(s);
    std::vector<T>& d = ArmaExport<T>::flat(c);
    return arma::Col<T>(arma::Mat<T>(d.data(), (arma::uword)d.size(), 1, true));
  }
};
inline SEXP wrap(const arma::mat& m) {
  NumericMatrix o((int)m.n_rows, (int)m.n_cols);
  std::copy(m.memptr(), m.memptr() + m.n_elem, o.begin());
  return o.sexp();
}

}  // namespace Rcpp

#endif
