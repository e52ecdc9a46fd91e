// many_models_host_check.cpp -- prints what the pure host pieces of the many-model core (phylomap_amd/csrc/phm_loglik_host.h)
// compute: the chunk plan over a grid of free memory, expect_chunk, model counts and caller's extras, and the staged bytes of
// models and tips.  It makes no HIP call and needs no device.  Built with hipcc and -fsanitize=address,undefined on the host
// side and compared with a Python transcription of the formulas by tests/test_many_models_host_cpu.py.
#include "phm_loglik_host.h"

#include <cinttypes>

using namespace phm_ll;

static LlInput shape(int n, bool paired, int S) {
  LlInput in;
  in.n = n; in.T = 6; in.Nn = 5; in.E = 10; in.NT = 11; in.S = S; in.K = 130;
  in.paired = paired; in.per_site = true;
  return in;
}

static void plans() {
  const size_t extras[2][3] = {{0, 0, 0}, {4096, 100, 50}};
  const size_t frees[] = {0, size_t(1) << 20, 2 * LL_WORK + (size_t(1) << 20), size_t(64) << 30};
  const int chunks[] = {0, 2, 100};
  const int64_t counts[] = {1, 64, 65, 130};
  for (int n : {3, 5})
    for (int paired = 0; paired < 2; ++paired) {
      const LlInput in = shape(n, paired != 0, 1000);
      for (const auto& x : extras)
        for (size_t free_b : frees)
          for (int chunk : chunks)
            for (int64_t count : counts) {
              const LlPlan pl = ll_plan(free_b, in, count, chunk, x[0], x[1], x[2]);
              std::printf("plan n=%d paired=%d extra=%zu,%zu,%zu free=%zu chunk=%d count=%" PRId64 " -> Kc_max=%" PRId64 " Sc_max=%" PRId64
                          " ne_max=%d\n", n, paired, x[0], x[1], x[2], free_b, chunk, count, pl.Kc_max, pl.Sc_max, pl.ne_max);
            }
    }
}

static void bytes(const char* what, const std::vector<uint8_t>& v, size_t row) {
  std::printf("%s %zu", what, v.size());
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i % row == 0 ? " | " : "", (int)v[i]);
  std::printf("\n");
}

static void staging() {
  const int K = 70, T = 5, S = 5, n = 3, nn = 9;
  std::vector<int32_t> tips((size_t)S * T), owner(K);
  for (int s = 0; s < S; ++s)
    for (int t = 0; t < T; ++t) tips[(size_t)s * T + t] = (s * 7 + t * 3) % 4;
  for (int k = 0; k < K; ++k) owner[k] = (k * 37 + 11) % S;                // every site, in no order
  LlInput in;
  in.n = n; in.T = T; in.S = S; in.K = K; in.per_site = true;
  in.states = tips.data();
  in.Qr.resize((size_t)K * nn);
  for (size_t i = 0; i < in.Qr.size(); ++i) in.Qr[i] = (double)(i / nn * 100 + i % nn);

  // the two chunks of 70 models at Kc_max = 64, and all of them in one
  const int64_t chunks[3][2] = {{0, 64}, {64, 6}, {0, 70}};
  std::vector<double> rows;
  std::vector<uint8_t> th;
  in.paired = true; in.site_of_model = owner.data();
  for (const auto& c : chunks) {
    const int Kp = (int)((c[1] + 63) / 64 * 64);
    ll_stage_rows(in.Qr.data() + (size_t)c[0] * nn, nn, c[1], Kp, rows);
    std::printf("models m0=%" PRId64 " Kc=%" PRId64 " Kp=%d %zu", c[0], c[1], Kp, rows.size());
    for (size_t i = 0; i < rows.size(); ++i) std::printf("%s%.0f", i % Kp == 0 ? " | " : " ", rows[i]);
    std::printf("\n");
    ll_stage_tips_paired(in, c[0], c[1], Kp, th);
    std::printf("paired m0=%" PRId64 " Kc=%" PRId64 " ", c[0], c[1]);
    bytes("tips", th, (size_t)Kp);
  }
  in.paired = false; in.site_of_model = nullptr;
  th.assign(1000, (uint8_t)9);                                             // a longer buffer from an earlier chunk
  ll_stage_tips_sites(in, 2, 3, th);
  bytes("cross s0=2 Sc=3 tips", th, (size_t)T);
}

int main() {
  plans();
  staging();
  std::printf("ok\n");
  return 0;
}
