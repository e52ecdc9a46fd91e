// Stand-alone check of the integer form of the categorical draw (phm_draw_tab.h) against sample_cat and u01 of phm_device.h, restated
// here for the host.  Built with the host compiler, -ffp-contract=off and -fsanitize=address,undefined by
// tests/test_draw_thresholds_cpu.py, which writes the models: a text file of `n` followed by the n*n entries of B (row-major, C99 hex
// floats), one model after the other.  For every model, chain row kk = 0 .. 40 and pair (cs, s_prev) the entry's index must be
// sample_cat's at the words 0, 1, 2^32-2, 2^32-1, T_j - 1 .. T_j + 2 and 1 000 random words, and its fallback bit must be set
// exactly where sample_cat raises its zero-probability flag.  Prints per model the thresholds that no word satisfies, the ones
// every word satisfies and the entries with the fallback bit.  With a row count as second argument it prints the tables instead, an
// entry per line in the device table's order (tests/test_gpu_draw_thresholds.py compares the table the device built with them).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "phm_draw_tab.h"

namespace {

constexpr uint32_t ZERO_PROB = 1u;
constexpr int ROWS = 41;

// phm_device.h u01
double u01(uint32_t x) { return ((double)x + 0.5) * 2.3283064365386962890625e-10; }

// phm_device.h sample_cat
template <int NS>
int sample_cat(const double (&p)[NS], double u, uint32_t& err) {
  double total = p[0];
  for (int j = 1; j < NS; ++j) total += p[j];
  if (!(total > 0.0) || std::isinf(total)) err |= ZERO_PROB;
  double thr = u * total;
  double cum = p[0];
  int idx = (thr <= cum) ? 0 : 1;
  for (int j = 1; j < NS - 1; ++j) { cum += p[j]; idx += (thr <= cum) ? 0 : 1; }
  return idx;
}

struct Tally { long draws = 0, none = 0, every = 0, fallback = 0, bad = 0; };

// col[kk][cs][:] = B^kk e_cs, unfused left-to-right sums (the host's chain tables for 2 to 4 states)
template <int NS>
std::vector<double> chain_rows(const std::vector<double>& B, int rows) {
  std::vector<double> col((size_t)rows * NS * NS, 0.0);
  for (int j = 0; j < NS; ++j) col[(size_t)j * NS + j] = 1.0;
  for (int k = 1; k < rows; ++k)
    for (int j = 0; j < NS; ++j) {
      const double* x = &col[((size_t)(k - 1) * NS + j) * NS];
      double* y = &col[((size_t)k * NS + j) * NS];
      for (int i = 0; i < NS; ++i) {
        double acc = B[i * NS] * x[0];
        for (int c = 1; c < NS; ++c) acc += B[i * NS + c] * x[c];
        y[i] = acc;
      }
    }
  return col;
}

// `rows` rows of the table of one model, a line of four hex words per entry, in the order of the device table
template <int NS>
void dump_model(const std::vector<double>& B, int rows) {
  const std::vector<double> col = chain_rows<NS>(B, rows);
  for (int kk = 0; kk < rows; ++kk)
    for (int cs = 0; cs < NS; ++cs)
      for (int sp = 0; sp < NS; ++sp) {
        uint32_t e[4];
        phm::draw_tab_entry<NS>(&B[(size_t)sp * NS], &col[((size_t)kk * NS + cs) * NS], e);
        std::printf("%08x %08x %08x %08x\n", e[0], e[1], e[2], e[3]);
      }
}

template <int NS>
void check_model(const std::vector<double>& B, Tally& t) {
  const std::vector<double> col = chain_rows<NS>(B, ROWS);
  uint64_t rng = 0x9e3779b97f4a7c15ull;
  for (int kk = 0; kk < ROWS; ++kk)
    for (int cs = 0; cs < NS; ++cs)
      for (int sp = 0; sp < NS; ++sp) {
        const double* beta = &col[((size_t)kk * NS + cs) * NS];
        const double* b2 = &B[(size_t)sp * NS];
        uint32_t e[4];
        phm::draw_tab_entry<NS>(b2, beta, e);
        double pr[NS];
        for (int c = 0; c < NS; ++c) pr[c] = b2[c] * beta[c];
        uint32_t err0 = 0;
        (void)sample_cat<NS>(pr, u01(0u), err0);
        const bool flagged = (err0 & ZERO_PROB) != 0, fb = (e[3] & phm::DRAW_TAB_FALLBACK) != 0;
        if (flagged != fb) { ++t.bad; std::fprintf(stderr, "NS %d kk %d cs %d sp %d: fallback bit %d, sample_cat flag %d\n", NS, kk, cs, sp, (int)fb, (int)flagged); }
        if (fb) { ++t.fallback; continue; }
        for (int w = NS - 1; w < 3; ++w) if (e[w] != phm::DRAW_TAB_NEVER) { ++t.bad; std::fprintf(stderr, "NS %d: padding word %d is %08x\n", NS, w, e[w]); }
        if (e[3] > (uint32_t)(NS - 1)) { ++t.bad; std::fprintf(stderr, "NS %d: extra %u\n", NS, e[3]); }
        {   // the two edge cases, told apart by the predicate itself
          double total, cum[NS];
          phm::draw_tab_sums<NS>(b2, beta, total, cum);
          for (int j = 0; j < NS - 1; ++j) {
            if (!phm::draw_tab_below(0u, total, cum[j])) ++t.none;
            else if (phm::draw_tab_below(0xFFFFFFFFu, total, cum[j])) ++t.every;
          }
        }
        std::vector<uint32_t> words = {0u, 1u, 0xFFFFFFFEu, 0xFFFFFFFFu};
        for (int j = 0; j < NS - 1; ++j)
          for (int64_t d = -1; d <= 2; ++d) {
            const int64_t x = (int64_t)e[j] + d;
            if (x >= 0 && x <= 0xFFFFFFFFll) words.push_back((uint32_t)x);
          }
        for (int r = 0; r < 1000; ++r) {
          rng = rng * 6364136223846793005ull + 1442695040888963407ull;
          words.push_back((uint32_t)(rng >> 32));
        }
        for (uint32_t x : words) {
          uint32_t err = 0;
          const int want = sample_cat<NS>(pr, u01(x), err);
          const int got = phm::draw_tab_index<NS>(e[0], e[1], e[2], e[3], x);
          ++t.draws;
          if (want != got && ++t.bad <= 20)
            std::fprintf(stderr, "NS %d kk %d cs %d sp %d word %08x: table %d, sample_cat %d (entry %08x %08x %08x %08x)\n", NS, kk, cs, sp, x, got,
                         want, e[0], e[1], e[2], e[3]);
        }
      }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 && argc != 3) { std::fprintf(stderr, "usage: %s models.txt [rows: print the tables instead]\n", argv[0]); return 2; }
  const int dump_rows = argc == 3 ? std::atoi(argv[2]) : 0;
  if (argc == 3 && (dump_rows < 1 || dump_rows > phm::DRAW_TAB_ROWS)) { std::fprintf(stderr, "rows: 1 .. %d\n", phm::DRAW_TAB_ROWS); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  long bad = 0;
  int n = 0, model = 0;
  while (std::fscanf(f, "%d", &n) == 1) {
    if (n < 2 || n > 4) { std::fprintf(stderr, "model %d: %d states\n", model, n); std::fclose(f); return 2; }
    std::vector<double> B((size_t)n * n);
    for (double& v : B) {
      char tok[64];
      if (std::fscanf(f, "%63s", tok) != 1) { std::fprintf(stderr, "model %d: short\n", model); std::fclose(f); return 2; }
      v = std::strtod(tok, nullptr);
    }
    if (dump_rows) {
      if (n == 2) dump_model<2>(B, dump_rows); else if (n == 3) dump_model<3>(B, dump_rows); else dump_model<4>(B, dump_rows);
      ++model;
      continue;
    }
    Tally t;
    if (n == 2) check_model<2>(B, t); else if (n == 3) check_model<3>(B, t); else check_model<4>(B, t);
    std::printf("model %d states %d draws %ld none %ld every %ld fallback %ld mismatches %ld\n", model, n, t.draws, t.none, t.every, t.fallback, t.bad);
    bad += t.bad;
    ++model;
  }
  std::fclose(f);
  if (bad || model == 0) return 1;
  std::printf("ok\n");
  return 0;
}
