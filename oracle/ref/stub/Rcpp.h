// Stand-in for <Rcpp.h>: the part of Rcpp's surface that the reference's src/phylomap.cpp uses, written from scratch so that the
// reference's translation unit compiles and RUNS without R.  TEST INFRASTRUCTURE; see oracle/ref/README.md for what is
// implemented, where each behaviour is taken from and which of them are assumptions.
//
// R objects are a small tagged record (real vector, integer vector, generic list, optional dim and names) behind a shared
// pointer, so that copies of a vector share storage as Rcpp's do.  Random and density calls forward to the oracle's restatement of
// R's generators (orc_r_* in oracle/phm_oracle.c); their call semantics (rejection loop of runif, scale of rexp) live here.
#ifndef PHM_STUB_RCPP_H
#define PHM_STUB_RCPP_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <list>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

extern "C" {
void   orc_r_set_seed(uint32_t seed);
double orc_r_unif_rand(void);
double orc_r_exp_rand(void);
double orc_r_norm_rand(void);
double orc_r_rgamma(double a, double scale);
double orc_r_dpois(double x, double lambda);
}

struct phm_sexprec;
typedef std::shared_ptr<phm_sexprec> SEXP;
struct phm_sexprec {
  enum Kind { NIL, REAL, INT, LIST } kind = NIL;
  std::vector<double> r;
  std::vector<int> i;
  std::vector<SEXP> l;
  std::vector<std::string> names;
  int nrow = -1, ncol = -1;          // dim attribute; -1: none
};

// ---- R's C API, as far as it is called ---------------------------------------------------------------------------------------
inline double unif_rand() { return orc_r_unif_rand(); }
inline double exp_rand() { return orc_r_exp_rand(); }
inline double norm_rand() { return orc_r_norm_rand(); }
inline double Rf_rgamma(double a, double scale) { return orc_r_rgamma(a, scale); }
// nmath/dpois.c: argument checks, then dpois_raw (restated in the oracle)
inline double Rf_dpois(double x, double lambda, int give_log) {
  if (std::isnan(x) || std::isnan(lambda)) return x + lambda;
  if (lambda < 0) return NAN;
  if (std::fabs(x - std::nearbyint(x)) > 1e-7 * std::max(1.0, std::fabs(x))) return give_log ? -INFINITY : 0.0;
  if (x < 0 || !std::isfinite(x)) return give_log ? -INFINITY : 0.0;
  const double d = orc_r_dpois(std::nearbyint(x), lambda);
  return give_log ? std::log(d) : d;
}
// Gamma density by its closed form.  The reference calls it only inside `acceptcompare` (metropolis * hastings), a value it never
// reads, so nothing observable depends on the last bits; R's own route through dpois_raw is not restated.
inline double Rf_dgamma(double x, double shape, double scale, int give_log) {
  if (std::isnan(x) || std::isnan(shape) || std::isnan(scale)) return x + shape + scale;
  if (shape < 0 || scale <= 0) return NAN;
  if (x < 0) return give_log ? -INFINITY : 0.0;
  const double l = (shape - 1) * std::log(x) - x / scale - std::lgamma(shape) - shape * std::log(scale);
  return give_log ? l : std::exp(l);
}

namespace Rcpp {

struct index_out_of_bounds : std::out_of_range {
  index_out_of_bounds() : std::out_of_range("index out of bounds") {}
};
struct not_compatible : std::runtime_error {
  explicit not_compatible(const std::string& m) : std::runtime_error(m) {}
};

struct RNGScope { RNGScope() {} ~RNGScope() {} };   // GetRNGstate / PutRNGstate: the stream here is process-wide already

// Rcout: swallowed (the reference prints one line per capped branch); phm_stub_rcout_lines() counts the std::endl's so that a
// test can tell that the message was issued
inline long& phm_stub_rcout_counter() { static long c = 0; return c; }
struct RcoutT {
  template <class T> RcoutT& operator<<(const T&) { return *this; }
  RcoutT& operator<<(std::ostream& (*)(std::ostream&)) { ++phm_stub_rcout_counter(); return *this; }
};
static RcoutT Rcout;

template <class T> struct sexp_store;
template <> struct sexp_store<double> {
  static const phm_sexprec::Kind kind = phm_sexprec::REAL;
  static std::vector<double>& of(phm_sexprec& s) { return s.r; }
};
template <> struct sexp_store<int> {
  static const phm_sexprec::Kind kind = phm_sexprec::INT;
  static std::vector<int>& of(phm_sexprec& s) { return s.i; }
};

// coercion as R's coerceVector does it between REALSXP and INTSXP (double -> int truncates toward zero)
template <class T> SEXP coerce_to(const SEXP& s) {
  if (!s) throw not_compatible("NULL where a vector is expected");
  if (s->kind == sexp_store<T>::kind) return s;
  SEXP o = std::make_shared<phm_sexprec>();
  o->kind = sexp_store<T>::kind; o->nrow = s->nrow; o->ncol = s->ncol; o->names = s->names;
  std::vector<T>& d = sexp_store<T>::of(*o);
  if (s->kind == phm_sexprec::REAL) for (double v : s->r) d.push_back((T)v);
  else if (s->kind == phm_sexprec::INT) for (int v : s->i) d.push_back((T)v);
  else if (s->kind == phm_sexprec::NIL) {}
  else throw not_compatible("a list where an atomic vector is expected");
  return o;
}

template <class T> class Vector {
 protected:
  SEXP s_;
  std::vector<T>& d() const { return sexp_store<T>::of(*s_); }
  static SEXP fresh(size_t n) {
    SEXP o = std::make_shared<phm_sexprec>();
    o->kind = sexp_store<T>::kind;
    sexp_store<T>::of(*o).assign(n, T(0));
    return o;
  }
 public:
  typedef T* iterator;
  typedef const T* const_iterator;
  Vector() : s_(fresh(0)) {}
  explicit Vector(int n) : s_(fresh(n < 0 ? 0 : (size_t)n)) {}          // zero-filled, as Rcpp's Vector(n)
  explicit Vector(unsigned n) : s_(fresh(n)) {}
  explicit Vector(long n) : s_(fresh(n < 0 ? 0 : (size_t)n)) {}
  explicit Vector(unsigned long n) : s_(fresh(n)) {}
  Vector(const SEXP& s) : s_(coerce_to<T>(s)) {}
  template <class It> Vector(It first, It last) : s_(fresh(0)) { for (; first != last; ++first) d().push_back((T)*first); }
  long size() const { return (long)d().size(); }
  long length() const { return size(); }
  T* begin() const { return d().data(); }
  T* end() const { return d().data() + d().size(); }
  T& operator()(long i) const { if (i < 0 || i >= size()) throw index_out_of_bounds(); return d()[(size_t)i]; }
  T& operator[](long i) const { if (i < 0 || i >= size()) throw index_out_of_bounds(); return d()[(size_t)i]; }
  const SEXP& sexp() const { return s_; }
  template <class A, class B> static Vector create(const A& a, const B& b) {
    Vector v(2); v[0] = (T)a; v[1] = (T)b; return v;
  }
  template <class A, class B, class C> static Vector create(const A& a, const B& b, const C& c) {
    Vector v(3); v[0] = (T)a; v[1] = (T)b; v[2] = (T)c; return v;
  }
};
typedef Vector<double> NumericVector;
typedef Vector<int> IntegerVector;

template <class T> class Matrix : public Vector<T> {
 public:
  Matrix() : Vector<T>() { this->s_->nrow = 0; this->s_->ncol = 0; }
  Matrix(int r, int c) : Vector<T>(r * c) { this->s_->nrow = r; this->s_->ncol = c; }
  Matrix(const SEXP& s) : Vector<T>(s) { if (this->s_->nrow < 0) throw not_compatible("not a matrix"); }
  int nrow() const { return this->s_->nrow; }
  int ncol() const { return this->s_->ncol; }
  T& operator()(int i, int j) const {
    if (i < 0 || j < 0 || i >= nrow() || j >= ncol()) throw index_out_of_bounds();
    return this->d()[(size_t)i + (size_t)j * nrow()];
  }
  struct RowView {
    const Matrix* m; int r;
    int size() const { return m->ncol(); }
    T& operator[](int j) const { return (*m)(r, j); }
    T& operator()(int j) const { return (*m)(r, j); }
  };
  RowView row(int i) const { if (i < 0 || i >= nrow()) throw index_out_of_bounds(); return RowView{this, i}; }
};
typedef Matrix<double> NumericMatrix;
typedef Matrix<int> IntegerMatrix;

class List;
inline SEXP wrap(const SEXP& s) { return s; }
inline SEXP wrap(double v) { SEXP o = std::make_shared<phm_sexprec>(); o->kind = phm_sexprec::REAL; o->r.push_back(v); return o; }
inline SEXP wrap(int v) { SEXP o = std::make_shared<phm_sexprec>(); o->kind = phm_sexprec::INT; o->i.push_back(v); return o; }
inline SEXP wrap(long v) { return v == 0 ? SEXP(std::make_shared<phm_sexprec>()) : wrap((double)v); }   // NULL arrives as (long)0
inline SEXP wrap(std::nullptr_t) { return std::make_shared<phm_sexprec>(); }
template <class T> SEXP wrap(const Vector<T>& v) { return v.sexp(); }
SEXP wrap(const List& l);

template <class T> struct Exporter;                         // Exporter<T>::get(SEXP): what as<T> does
template <> struct Exporter<SEXP> { static SEXP get(const SEXP& s) { return s; } };
template <> struct Exporter<double> {
  static double get(const SEXP& s) {
    SEXP c = coerce_to<double>(s);
    if (c->r.size() != 1) throw not_compatible("expecting a single value");
    return c->r[0];
  }
};
template <> struct Exporter<int> {
  static int get(const SEXP& s) {
    SEXP c = coerce_to<int>(s);
    if (c->i.size() != 1) throw not_compatible("expecting a single value");
    return c->i[0];
  }
};
template <class T> struct Exporter<Vector<T> > { static Vector<T> get(const SEXP& s) { return Vector<T>(s); } };
template <class T> struct Exporter<Matrix<T> > { static Matrix<T> get(const SEXP& s) { return Matrix<T>(s); } };

struct NamedArg { std::string name; SEXP value; };
struct Named {
  std::string name;
  explicit Named(const std::string& n) : name(n) {}
  template <class T> NamedArg operator=(const T& v) const { return NamedArg{name, wrap(v)}; }
};

class List {
  SEXP s_;
 public:
  List() : s_(std::make_shared<phm_sexprec>()) { s_->kind = phm_sexprec::LIST; }
  explicit List(int n) : List() { s_->l.assign((size_t)n, SEXP(std::make_shared<phm_sexprec>())); }
  List(const SEXP& s) : s_(s) { if (!s || s->kind != phm_sexprec::LIST) throw not_compatible("not a list"); }
  const SEXP& sexp() const { return s_; }
  long size() const { return (long)s_->l.size(); }
  class Proxy {
    SEXP owner_; long idx_; std::string name_;
   public:
    Proxy(const SEXP& o, long i, const std::string& n) : owner_(o), idx_(i), name_(n) {}
    SEXP get() const {
      if (idx_ < 0) throw index_out_of_bounds();        // Rcpp: "no such name" is an index error as well
      return owner_->l[(size_t)idx_];
    }
    void set(const SEXP& v) {
      if (idx_ < 0) {                                    // assigning to a new name appends
        if (owner_->names.size() < owner_->l.size()) owner_->names.resize(owner_->l.size());
        owner_->l.push_back(v); owner_->names.push_back(name_); idx_ = (long)owner_->l.size() - 1;
      } else owner_->l[(size_t)idx_] = v;
    }
    template <class T> operator T() const { return Exporter<T>::get(get()); }
    template <class T> Proxy& operator=(const T& v) { set(wrap(v)); return *this; }
  };
  Proxy operator[](int i) const { if (i < 0 || i >= size()) throw index_out_of_bounds(); return Proxy(s_, i, ""); }
  Proxy operator()(int i) const { return (*this)[i]; }
  Proxy operator[](const std::string& n) const {
    for (size_t k = 0; k < s_->names.size(); ++k) if (s_->names[k] == n) return Proxy(s_, (long)k, n);
    return Proxy(s_, -1, n);
  }
  Proxy operator[](const char* n) const { return (*this)[std::string(n)]; }
  void push_back(const SEXP& v) { s_->l.push_back(v); }
  static List create(const NamedArg& a, const NamedArg& b) {
    List l; l[a.name] = a.value; l[b.name] = b.value; return l;
  }
};
inline SEXP wrap(const List& l) { return l.sexp(); }
template <> struct Exporter<List> { static List get(const SEXP& s) { return List(s); } };

namespace detail {
inline SEXP to_sexp(const SEXP& s) { return s; }
inline SEXP to_sexp(const List::Proxy& p) { return p.get(); }
inline SEXP to_sexp(const List& l) { return l.sexp(); }
template <class T> SEXP to_sexp(const Vector<T>& v) { return v.sexp(); }
}  // namespace detail

template <class T, class U> T as(const U& u) { return Exporter<T>::get(detail::to_sexp(u)); }

// ---- sugar -------------------------------------------------------------------------------------------------------------------
// runif(n): Rcpp fills element 0 first, each element by stats::UnifGenerator__0__1: redraw while u <= 0 or u >= 1
inline NumericVector runif(int n) {
  NumericVector v(n);
  for (int i = 0; i < n; ++i) { double u; do { u = unif_rand(); } while (u <= 0.0 || u >= 1.0); v[i] = u; }
  return v;
}
// rexp(n, rate): stats::ExpGenerator(scale = 1 / rate), each element scale * exp_rand()
inline NumericVector rexp(int n, double rate) {
  const double scale = 1.0 / rate;
  NumericVector v(n);
  for (int i = 0; i < n; ++i) v[i] = scale * exp_rand();
  return v;
}
inline NumericVector operator*(double a, const NumericVector& x) {
  NumericVector v((int)x.size());
  for (long i = 0; i < x.size(); ++i) v[i] = a * x[i];
  return v;
}

}  // namespace Rcpp

// The reference reports progress with printf("%i \r", i) once per sweep.  Every standard header it uses is included above, so
// from here on the name can be made a no-op without touching a declaration.
#define printf(...) ((void)0)

#endif
