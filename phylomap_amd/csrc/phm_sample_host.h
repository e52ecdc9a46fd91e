// phm_sample_host.h -- what the two exact samplers of histories share on the host: phm_sample_histories_models
// (phm_sample_api.cpp, 2..8 states) and phm_sample_histories_models_wide (phm_sample_wide_api.cpp, 9..64
// states, section 24).  The checked input and the checks that follow ll_validate, the one body of both extern "C" functions
// (sm_entry) and the tile driver SmTiles (section 19b): the batch of tiles with its buffers, the fill of the kernels' shared
// parameters, the flush and the map shard.  The tile count, the tiles of an evaluation and the scatter of a batch are pure host
// code in this header (tests/native/sample_host_check.cpp runs them); whatever makes a HIP call is in phm_sample_host.cpp.
#pragma once

#include <functional>

#include "phm_loglik_host.h"
#include "phm_maps_host.h"
#include "phm_sample.h"

namespace phm_ll {

struct SmInput {
  LlInput ll;
  int cols = 0, D = 0, fx_exp = 0;
  int64_t n_eval = 0, H = 0;                            // evaluations, histories
  std::vector<int32_t> depth;                           // [K] M(mu_k max_b t_b)
  std::vector<int32_t> order, level_off;                // s.down positions by the depth of the parent
  phm_options opt;
  int32_t* nodes = nullptr;
};

// draws, the state count (outside n_lo .. n_hi: PHM_ERR_UNSUPPORTED with fn + range_msg), the 31-bit evaluation ids, the count
// of histories, max(-q_ii) t_b of every model and branch, and from them every model's table depth and the depth levels
inline int32_t sm_prepare(const std::string& fn, int n_lo, int n_hi, const char* range_msg, SmInput& sm, int32_t draws) {
  LlInput& in = sm.ll;
  const int n = in.n;
  if (draws < 1) return fail(PHM_ERR_BAD_INPUT, fn + "draws must be >= 1");
  if (n < n_lo || n > n_hi) return fail(PHM_ERR_UNSUPPORTED, fn + range_msg);
  if ((int64_t)in.S * in.K > (int64_t)INT32_MAX) return fail(PHM_ERR_BAD_INPUT, fn + "sites * models must fit in 31 bits (evaluation ids)");
  sm.cols = n + n * (n - 1);
  sm.D = draws;
  sm.n_eval = in.paired ? in.K : (int64_t)in.S * in.K;
  if (sm.n_eval > INT64_MAX / 4096 / draws) return fail(PHM_ERR_BAD_INPUT, fn + "evaluations * draws overflows");
  sm.H = sm.n_eval * draws;
  const size_t nn = (size_t)n * n;
  double t_max = 0.0, tree_len = 0.0;
  for (int b = 0; b < in.E; ++b) { t_max = std::max(t_max, in.edge_length[b]); tree_len += in.edge_length[b]; }
  (void)std::frexp(std::max(tree_len, 1.0), &sm.fx_exp);
  sm.depth.resize(in.K);
  for (int k = 0; k < in.K; ++k) {
    double mu = 0.0;
    for (int i = 0; i < n; ++i) mu = std::max(mu, -in.Qr[(size_t)k * nn + (size_t)i * n + i]);
    for (int b = 0; b < in.E; ++b)
      if (mu * in.edge_length[b] > phm::SM_MAX_JUMP_MEAN)
        return fail(PHM_ERR_UNSUPPORTED, "model " + std::to_string(k) + ", edge row " + std::to_string(b + 1) + ": max(-q_ii) * t_b above 32768");
    sm.depth[k] = phm::sm_stop_index(mu * t_max);
  }
  phm::depth_levels(in.sched, sm.order, sm.level_off);
  return PHM_OK;
}

// ---- the tiles (host only) ----
// device bytes of a tile: node states, accumulators, the output columns, the node output when asked for, and the tile itself
inline size_t sm_tile_bytes(int n, int NT, int cols, bool nodes) {
  return (size_t)NT * 64 + 64 * (sizeof(double) * (cols + n) + sizeof(uint32_t) * n * (n - 1)) +
         (nodes ? sizeof(int32_t) * 64 * (size_t)NT : 0) + sizeof(phm::SmTile);
}

// tiles of one batch: an eighth of the free memory at most, 2^20, `cap` (the launch's own bound) and, when set, expect_chunk
inline int64_t sm_tiles_max(size_t free_b, size_t per_tile, int64_t tiles_total, int chunk, int64_t cap) {
  int64_t Tc_max = std::max<int64_t>(1, std::min<int64_t>({tiles_total, (int64_t)(free_b / 8 / per_tile), (int64_t)1 << 20, cap}));
  if (chunk > 0) Tc_max = std::min<int64_t>(Tc_max, chunk);
  return Tc_max;
}

// The tile of draws d0 .. of an evaluation of D draws.  ev, k: the evaluation and the model in the launch's buffers; eval_id: the
// GLOBAL evaluation id; row_first: the evaluation's first history relative to the shard's.  d0 runs over 0, 64, .. < D.
inline phm::SmTile sm_tile_of(int32_t ev, int32_t k, uint32_t eval_id, int64_t row_first, int D, int d0) {
  phm::SmTile tl = {};
  tl.ev = ev; tl.k = k; tl.eval_id = eval_id;
  tl.d0 = d0; tl.n_valid = std::min(64, D - d0); tl.row0 = row_first + d0;
  return tl;
}

// A flushed batch of nt tiles into the caller's arrays: outh [cols][nt * 64] and nodes_h [nt * 64][NT] as the finish kernel
// leaves them; stats [cols][H] and nodes [H][NT] (NULL: not asked for) by global history, h_first the shard's first.
inline void sm_scatter(const phm::SmTile* tiles, int nt, int cols, int NT, const double* outh, const int32_t* nodes_h, int64_t h_first,
                       int64_t H, double* stats, int32_t* nodes) {
  const size_t npad = (size_t)nt * 64;
  for (int i = 0; i < nt; ++i) {
    const int64_t h0 = h_first + tiles[i].row0;
    const int nv = tiles[i].n_valid;
    for (int c = 0; c < cols; ++c) std::copy_n(outh + (size_t)c * npad + (size_t)i * 64, nv, stats + h0 + H * c);
    if (nodes) std::copy_n(nodes_h + (size_t)i * 64 * NT, (size_t)nv * NT, nodes + h0 * NT);
  }
}

// what the tree, the options and the fixed-point exponent decide of the kernels' shared parameters (the buffers are the caller's)
inline void sm_fill_core(phm::SmCore& c, const LlInput& in, const phm_options& o, int fx_exp) {
  c.n_node = in.Nn; c.n_edge = in.E; c.root_row = in.T + in.sched.root;
  c.seed_lo = (uint32_t)(o.seed & 0xFFFFFFFFull); c.seed_hi = (uint32_t)(o.seed >> 32);
  c.replica = (uint32_t)o.replica_offset;
  c.fx_scale = std::ldexp(1.0, 61 - fx_exp); c.fx_inv = std::ldexp(1.0, fx_exp - 61);
}

// ---- the tile driver of models [first, first + count) on one device ----
// The order of a driver: setup, alloc on hipMemGetInfo's free bytes, then add per evaluation, flush before L is overwritten, and
// finish_maps.  launch: the sampler's launches of the batch whose tile count alloc's block holds.  The flush and the map offsets
// are timed here (sample_ms, offsets_ms); the driver adds them to its own sums.
struct SmTiles {
  using Launch = std::function<hipError_t()>;
  const SmInput& sm;
  const std::string name, fn;                           // the entry point, and its message prefix
  double* stats;
  phm_maps::Host* mh;
  size_t shard_index, batch_b = 0;                      // batch_b: device bytes of a full batch of tiles
  int64_t h_first = 0, h_count = 0, map_pad = 0, Tc_max = 0;   // the shard's histories; tiles of a batch
  phm::SmCore* core = nullptr;                          // the driver's parameter block: n_tiles is set at every flush
  DevBuf ddown, dorder, derr, dtile, dnst, ddw, dcnt, dout, dnodes;
  std::vector<double> outh;
  std::vector<int32_t> nodes_h;
  std::vector<phm::SmTile> tiles;
  phm::MapsDev maps_dev;
  phm_maps::Shard shard;
  KernelTimer tm;
  double sample_ms = 0.0, offsets_ms = 0.0;

  SmTiles(const SmInput& input, const char* entry, double* stats_, phm_maps::Host* maps, size_t si)
      : sm(input), name(entry), fn(std::string(entry) + ": "), stats(stats_), mh(maps), shard_index(si) {}
  int32_t setup(int64_t first, int64_t count);          // down steps, depth order, error word, the map shard
  // Tc_max (cap: the launch's own bound) and batch_b from the free bytes, the tile buffers, and c's shared parameters
  int32_t alloc(size_t free_b, int64_t count, int64_t cap, phm::SmCore& c);
  int maps_mode() const { return mh ? mh->mode : phm::MAPS_OFF; }
  // evaluation ev (index into loglik) of model k and site `site` (global), at ev_local / k_local in the launch's buffers: NaN
  // rows and zero nodes when impossible, else its tiles; a full batch is flushed
  int32_t add(int64_t ev, int64_t site, int64_t k, int32_t ev_local, int32_t k_local, bool possible, const Launch& launch);
  int32_t flush(const Launch& launch);                  // upload, zero, timed launch, download, error word, scatter
  int32_t finish_maps();                                // sizing: counts -> offsets; offsets or segments home
};

using SmDevice = int32_t (*)(const SmInput& sm, int32_t device, int64_t first, int64_t count, double* stats, double* loglik,
                             phm_maps::Host* mh, size_t si);
// The body of both extern "C" functions: the argument checks, ll_validate, sm_prepare (n_lo .. n_hi, range_msg), the map
// arguments, and run over the shards of models (every draw is addressed by its global evaluation and draw index, so with
// phm_options.n_devices > 1 every output is the one-device output bit for bit).
inline int32_t sm_entry(const char* name, int n_lo, int n_hi, const char* range_msg, SmDevice run, const phm_tree* x, int32_t n_states,
                 int32_t n_models, const double* Q, const double* pid, int32_t n_pid, const int32_t* observe, const int32_t* site_of_model,
                 int32_t draws, const phm_options* opt, double* stats, double* loglik, int32_t* nodes, int64_t* map_off, int64_t map_cap,
                 double* map_dwell, int32_t* map_state) {
  const std::string fn = std::string(name) + ": ";
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid || !stats || !loglik)
    return fail(PHM_ERR_BAD_INPUT, fn + "NULL argument (only observe, site_of_model, opt, nodes and the map arrays may be NULL)");
  SmInput sm;
  int32_t st = ll_validate(fn, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, o, sm.ll);
  if (st) return st;
  sm.opt = o; sm.nodes = nodes;
  st = sm_prepare(fn, n_lo, n_hi, range_msg, sm, draws);
  if (st) return st;
  const bool want_maps = map_off || map_dwell || map_state;
  phm_maps::Host mh;
  if (want_maps) {
    st = phm_maps::validate(name, sm.H, x->n_edge, map_off, map_cap, map_dwell, map_state, mh);
    if (st) return st;
  }
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, sm.ll.K, shards);
  if (st) return st;
  mh.shard_total.assign(shards.size(), 0);
  st = run_shards(shards, [&](const phm_shard& sh, size_t i) {
    return run(sm, sh.device, sh.first, sh.count, stats, loglik, want_maps ? &mh : nullptr, i);
  });
  if (st) return st;
  if (want_maps) {
    // finish_sizing works in units of histories: a shard of models is histories [e(first) D, e(first + count) D)
    std::vector<phm_shard> hs = shards;
    const int64_t per_model = (sm.ll.paired ? 1 : (int64_t)sm.ll.S) * sm.D;
    for (phm_shard& s : hs) { s.first *= per_model; s.count *= per_model; }
    phm_maps::finish_sizing(mh, hs);
  }
  return PHM_OK;
}

}  // namespace phm_ll
