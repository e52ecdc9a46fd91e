// Stand-in for <RcppArmadilloExtensions/sample.h>: RcppArmadillo::sample(x, size, replace, prob) for the one way the reference
// calls it -- with replacement and with a probability vector.  Written from scratch after RcppArmadillo's documented algorithm
// (FixProb, then ProbSampleReplace); oracle/ref/README.md says which details are recalled and which are assumptions.
// TEST INFRASTRUCTURE.
#ifndef PHM_STUB_SAMPLE_H
#define PHM_STUB_SAMPLE_H

#include "../RcppArmadillo.h"

namespace Rcpp {
namespace RcppArmadillo {

// FixProb: reject non-finite and negative entries, sum the positive ones in index order, divide every entry by that sum
inline void FixProb(std::vector<double>& p, int size, bool replace) {
  double sum = 0.0;
  int npos = 0;
  for (double v : p) {
    if (!std::isfinite(v)) throw std::range_error("NAs not allowed in probability");
    if (v < 0.0) throw std::range_error("Negative probabilities not allowed");
    if (v > 0.0) { npos++; sum += v; }
  }
  if (npos == 0 || (!replace && size > npos)) throw std::range_error("Not enough positive probabilities");
  for (double& v : p) v = v / sum;
}

template <class T> T sample(const T& x, const int size, const bool replace, NumericVector prob_ = NumericVector()) {
  const int n = (int)x.size();
  if (!replace) throw std::range_error("sample(): the stand-in draws with replacement only");
  if ((int)prob_.size() != n) throw std::range_error("Number of probabilities must equal input vector length");
  if (n > 200) throw std::range_error("sample(): Walker's alias method (more than 200 values) is not in the stand-in");
  std::vector<double> p(prob_.begin(), prob_.end());
  FixProb(p, size, replace);
  // ProbSampleReplace: order by descending probability (sort_index is an std::sort of (value, index) packets on value alone, so
  // the order of exactly equal values is the library's), accumulate, take the first jj < n - 1 with u <= cum[jj], else the last
  struct packet { double val; int index; };
  std::vector<packet> q((size_t)n);
  for (int i = 0; i < n; ++i) { q[(size_t)i].val = p[(size_t)i]; q[(size_t)i].index = i; }
  std::sort(q.begin(), q.end(), [](const packet& a, const packet& b) { return a.val > b.val; });
  double cum = 0.0;
  for (packet& e : q) { cum += e.val; e.val = cum; }
  T ret(size);
  for (int ii = 0; ii < size; ++ii) {
    const double rU = unif_rand();
    int jj;
    for (jj = 0; jj < n - 1; ++jj) if (rU <= q[(size_t)jj].val) break;
    ret[ii] = x[q[(size_t)jj].index];
  }
  return ret;
}

}  // namespace RcppArmadillo
}  // namespace Rcpp

#endif
