// sample_host_check.cpp -- prints what the pure host pieces of the exact samplers and of the wide tree passes compute
// (phylomap_amd/csrc/phm_ancestral_wide_host.h: aw_plan; phm_sample_host.h: sm_tile_bytes, sm_tiles_max, sm_tile_of,
// sm_scatter): the wide chunk plan over a grid of free memory, expect_chunk, model counts and both callers' extras, the tiles of
// an evaluation, and the scatter of a flushed batch.  It makes no HIP call and needs no device.  Built with hipcc and
// -fsanitize=address,undefined on the host side and compared with a Python transcription of the drivers' earlier formulas by
// tests/test_sample_host_cpu.py.
#include "phm_ancestral_wide_host.h"
#include "phm_sample_host.h"

#include <cinttypes>

using namespace phm_ll;

static const size_t FREES[] = {0, size_t(1) << 20, 4190288, 21157808, size_t(1) << 28, size_t(64) << 30};
static const int CHUNKS[] = {0, 1, 100};
static const int64_t COUNTS[] = {1, 3, 130};
constexpr int S = 1000, J = 5, D = 70, DEPTH = 20;

static LlInput shape(int n, bool paired) {
  LlInput in;
  in.n = n; in.T = 6; in.Nn = 5; in.E = 10; in.NT = 11; in.S = S; in.K = 130;
  in.paired = paired; in.per_site = true;
  return in;
}

static void show(const char* who, int n, int paired, size_t free_b, int chunk, int64_t count, const AwPlan& pl) {
  std::printf("%s n=%d paired=%d free=%zu chunk=%d count=%" PRId64 " -> Kc_max=%" PRId64 " Sc_max=%" PRId64 " step_max=%d\n", who, n, paired,
              free_b, chunk, count, pl.Kc_max, pl.Sc_max, pl.step_max);
}

static void plans() {
  for (int n : {9, 64})
    for (int paired = 0; paired < 2; ++paired) {
      const LlInput in = shape(n, paired != 0);
      const size_t NP = (size_t)phm::aw_lanes(n), nn = (size_t)n * n;
      const int cols = n + n * (n - 1);
      for (size_t free_b : FREES)
        for (int chunk : CHUNKS)
          for (int64_t count : COUNTS) {
            // phm_ancestral_models_wide, marginal and joint with J reported nodes
            const size_t per_eval = (sizeof(double) * NP + sizeof(int32_t)) * (size_t)in.NT + sizeof(double) * (size_t)J * n +
                                    (sizeof(double) * NP + sizeof(int32_t)) * (size_t)in.Nn + (size_t)in.E * NP + (size_t)in.NT + sizeof(double);
            show("ancestral", n, paired, free_b, chunk, count, aw_plan(free_b, in, count, chunk, 0, 0, per_eval));
            // phm_sample_histories_models_wide, D draws with node states, tables of DEPTH + 1 rows
            const size_t per_tile = sm_tile_bytes(n, in.NT, cols, true);
            const int64_t Tc_max = sm_tiles_max(free_b, per_tile, count * in.sites_per_model() * ((D + 63) / 64), chunk, ((int64_t)1 << 30) / in.E);
            const size_t per_model = sizeof(double) * (nn + 1) + sizeof(int32_t) + sizeof(double) * (DEPTH + 1) * nn;
            const AwPlan need = aw_plan(free_b, in, count, chunk, per_tile * (size_t)Tc_max, per_model, 0);
            std::printf("sampler per_tile=%zu Tc_max=%" PRId64 " ", per_tile, Tc_max);
            if (need.budget < need.per_model + need.per_eval) std::printf("n=%d paired=%d free=%zu chunk=%d count=%" PRId64 " -> capacity\n", n, paired, free_b, chunk, count);
            else show("plan", n, paired, free_b, chunk, count, need);
          }
    }
}

static void tiles_of_an_evaluation() {
  for (int draws : {3, 64, 70, 129}) {
    const int64_t ev = 7, h_first = 2 * (int64_t)draws;                    // the shard begins at evaluation 2
    for (int d0 = 0; d0 < draws; d0 += 64) {
      const phm::SmTile tl = sm_tile_of(5, 2, 77u, ev * draws - h_first, draws, d0);
      std::printf("tile D=%d ev=%d k=%d eval_id=%u d0=%d n_valid=%d pad=%d row0=%" PRId64 "\n", draws, tl.ev, tl.k, tl.eval_id, tl.d0, tl.n_valid,
                  tl.pad, tl.row0);
    }
  }
}

static void scatter() {
  // evaluations 1 and 3 of four, 70 draws each, on a shard that begins at evaluation 1: four tiles, two of them with 6 live lanes
  const int cols = 3, NT = 4, H = 4 * D, h_first = D;
  std::vector<phm::SmTile> tiles;
  for (int64_t ev : {1, 3})
    for (int d0 = 0; d0 < D; d0 += 64) tiles.push_back(sm_tile_of(0, 0, 0u, ev * D - h_first, D, d0));
  const int nt = (int)tiles.size();
  const size_t npad = (size_t)nt * 64;
  std::vector<double> outh((size_t)cols * npad), stats((size_t)cols * H, -1.0);
  std::vector<int32_t> nodes_h(npad * NT), nodes((size_t)H * NT, -1);
  for (size_t i = 0; i < outh.size(); ++i) outh[i] = (double)(1000 + i);
  for (size_t i = 0; i < nodes_h.size(); ++i) nodes_h[i] = (int32_t)(5000 + i);
  sm_scatter(tiles.data(), nt, cols, NT, outh.data(), nodes_h.data(), h_first, H, stats.data(), nodes.data());
  std::printf("stats");
  for (double v : stats) std::printf(" %.0f", v);
  std::printf("\nnodes");
  for (int32_t v : nodes) std::printf(" %d", v);
  std::printf("\n");
  std::vector<double> only((size_t)cols * H, -1.0);                         // no node output asked for
  sm_scatter(tiles.data(), nt, cols, NT, outh.data(), nullptr, h_first, H, only.data(), nullptr);
  std::printf("stats alone %s\n", only == stats ? "equal" : "DIFFER");
}

int main() {
  plans();
  tiles_of_an_evaluation();
  scatter();
  std::printf("ok\n");
  return 0;
}
