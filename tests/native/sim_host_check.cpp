// sim_host_check.cpp -- prints what the table builder of the two forward simulators' shared front end
// (phylomap_amd/csrc/phm_sim_host.h: model_tables) computes for a few generators: the jump weights, their row totals, the inverse
// rates, or the refusal.  It makes no HIP call and needs no device.  Built with hipcc and -fsanitize=address,undefined on the host
// side and compared with a Python transcription of the loops by tests/test_sim_host_cpu.py.
#include "phm_sim_host.h"

#include <cstdio>

// generator `which` of n states, column-major: rates (1 + (7 i + 3 j + which) % 5) / 8, the diagonal minus the row's sum
static std::vector<double> generator(int n, int which) {
  std::vector<double> Q((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) {
    double sum = 0.0;
    for (int j = 0; j < n; ++j)
      if (j != i) { const double q = (1 + (7 * i + 3 * j + which) % 5) / 8.0; Q[i + (size_t)j * n] = q; sum += q; }
    Q[i + (size_t)i * n] = -sum;
  }
  return Q;
}

static void row(const char* what, const double* v, size_t count) {
  std::printf("%s", what);
  for (size_t i = 0; i < count; ++i) std::printf(" %.17g", v[i]);
  std::printf("\n");
}

// one call of the builder on exactly n n + 2 n doubles of heap, so that a write past any table is seen
static void tables(const char* name, const std::vector<double>& Q, int n, const std::string& who) {
  std::vector<double> qoff((size_t)n * n), qtot(n), inv(n);
  const int32_t st = phm_sim::model_tables(Q.data(), n, who, qoff.data(), qtot.data(), inv.data());
  std::printf("%s n=%d status=%d\n", name, n, (int)st);
  if (st) { std::printf("refused: %s\n", g_phm_err.c_str()); return; }
  row("qoff", qoff.data(), qoff.size());
  row("qtot", qtot.data(), qtot.size());
  row("inv_rate", inv.data(), inv.size());
}

int main() {
  tables("plain", generator(2, 0), 2, "");
  tables("plain", generator(5, 1), 5, "");
  std::vector<double> Q = generator(5, 2);                         // state 3 absorbs
  for (int j = 0; j < 5; ++j) Q[2 + (size_t)j * 5] = 0.0;
  tables("absorbing", Q, 5, "");
  Q = generator(2, 0);                                             // row 1 passes the row-sum check and has no target
  Q[0] = -1e-14; Q[0 + 2] = 0.0; Q[1] = 100.0; Q[1 + 2] = -100.0;
  tables("no_target", Q, 2, "");
  tables("no_target_model", Q, 2, "model 2: ");
  // K = 1 against model k of a batch of three: the same call on the batch's k-th matrix
  std::vector<double> batch;
  for (int k = 0; k < 3; ++k) { const std::vector<double> q = generator(5, 10 + k); batch.insert(batch.end(), q.begin(), q.end()); }
  for (int k = 0; k < 3; ++k) {
    tables("single", generator(5, 10 + k), 5, "");
    tables("batch", std::vector<double>(batch.begin() + (size_t)k * 25, batch.begin() + (size_t)(k + 1) * 25), 5, "model " + std::to_string(k) + ": ");
  }
  std::printf("ok\n");
  return 0;
}
