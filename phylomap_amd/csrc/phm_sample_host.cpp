// phm_sample_host.cpp -- the tile driver of the two exact samplers of histories (phm_sample_host.h):
// SmTiles' buffers, its flush and its map shard.
#include "phm_sample_host.h"

#include <limits>

namespace phm_ll {

using namespace phm_ex;

int32_t SmTiles::setup(int64_t first, int64_t count) {
  const LlInput& in = sm.ll;
  h_first = ll_eval_of(in, 0, first) * sm.D;
  h_count = count * in.sites_per_model() * sm.D;
  map_pad = (h_count + 63) / 64 * 64;
  HIPCHK(upload(ddown, in.sched.down)); HIPCHK(upload(dorder, sm.order));
  HIPCHK(derr.alloc(sizeof(uint32_t)));
  HIPCHK(hipMemset(derr.p, 0, sizeof(uint32_t)));
  if (!mh) return PHM_OK;
  if (h_count > (int64_t)INT32_MAX) return fail(PHM_ERR_UNSUPPORTED, fn + "maps of more than 2^31 - 1 histories on one device");
  return shard.setup(*mh, h_first, h_count, map_pad, maps_dev);
}

int32_t SmTiles::alloc(size_t free_b, int64_t count, int64_t cap, phm::SmCore& c) {
  const LlInput& in = sm.ll;
  const size_t per_tile = sm_tile_bytes(in.n, in.NT, sm.cols, sm.nodes != nullptr);
  Tc_max = sm_tiles_max(free_b, per_tile, count * in.sites_per_model() * ((sm.D + 63) / 64), g_phm_debug.expect_chunk, cap);
  batch_b = per_tile * (size_t)Tc_max;
  const size_t n = (size_t)in.n, NT = (size_t)in.NT, cols = (size_t)sm.cols, npad_max = (size_t)Tc_max * 64;
  HIPCHK(dtile.alloc(sizeof(phm::SmTile) * (size_t)Tc_max)); HIPCHK(dnst.alloc(NT * npad_max));
  HIPCHK(ddw.alloc(sizeof(unsigned long long) * n * npad_max)); HIPCHK(dcnt.alloc(sizeof(uint32_t) * n * (n - 1) * npad_max));
  HIPCHK(dout.alloc(sizeof(double) * cols * npad_max));
  if (sm.nodes) HIPCHK(dnodes.alloc(sizeof(int32_t) * NT * npad_max));
  outh.resize(cols * npad_max);
  nodes_h.resize(sm.nodes ? NT * npad_max : 0);
  tiles.reserve((size_t)Tc_max);
  core = &c;
  sm_fill_core(c, sm.ll, sm.opt, sm.fx_exp);
  c.tiles = dtile.as<phm::SmTile>(); c.down = ddown.as<phm::DownStep>(); c.order = dorder.as<int32_t>();
  c.nstate = dnst.as<uint8_t>(); c.dwfx = ddw.as<unsigned long long>(); c.cnt = dcnt.as<uint32_t>();
  c.out = dout.as<double>(); c.nodes = sm.nodes ? dnodes.as<int32_t>() : nullptr; c.err = derr.as<uint32_t>();
  c.maps = maps_dev; c.map_pad = map_pad;
  return PHM_OK;
}

int32_t SmTiles::add(int64_t ev, int64_t site, int64_t k, int32_t ev_local, int32_t k_local, bool possible, const Launch& launch) {
  const int D = sm.D, NT = sm.ll.NT;
  if (!possible) {                                       // not drawn: NaN rows, zero nodes, empty map rows
    for (int64_t h = ev * D; h < (ev + 1) * D; ++h) {
      for (int c = 0; c < sm.cols; ++c) stats[h + sm.H * c] = std::numeric_limits<double>::quiet_NaN();
      if (sm.nodes) std::fill_n(sm.nodes + h * NT, NT, 0);
    }
    return PHM_OK;
  }
  for (int d0 = 0; d0 < D; d0 += 64) {
    tiles.push_back(sm_tile_of(ev_local, k_local, (uint32_t)(site * sm.ll.K + k), ev * D - h_first, D, d0));
    if ((int64_t)tiles.size() == Tc_max) {
      const int32_t st = flush(launch);
      if (st) return st;
    }
  }
  return PHM_OK;
}

int32_t SmTiles::flush(const Launch& launch) {
  if (tiles.empty()) return PHM_OK;
  const int n = sm.ll.n, NT = sm.ll.NT, cols = sm.cols, nt = (int)tiles.size();
  const size_t npad = (size_t)nt * 64;
  core->n_tiles = nt;
  HIPCHK(hipMemcpy(dtile.p, tiles.data(), sizeof(phm::SmTile) * nt, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(ddw.p, 0, sizeof(unsigned long long) * n * npad));
  HIPCHK(hipMemset(dcnt.p, 0, sizeof(uint32_t) * (size_t)n * (n - 1) * npad));
  HIPCHK(tm.start());
  HIPCHK(launch());
  HIPCHK(tm.stop());
  HIPCHK(hipMemcpy(outh.data(), dout.p, sizeof(double) * cols * npad, hipMemcpyDeviceToHost));
  if (sm.nodes) HIPCHK(hipMemcpy(nodes_h.data(), dnodes.p, sizeof(int32_t) * (size_t)NT * npad, hipMemcpyDeviceToHost));
  uint32_t derrh = 0;
  HIPCHK(hipMemcpy(&derrh, derr.p, sizeof derrh, hipMemcpyDeviceToHost));
  HIPCHK(tm.add_to(sample_ms));
  if (derrh & phm::DERR_CAPACITY) return fail(PHM_ERR_CAPACITY, fn + "a branch's jump-count series outgrew the table of its model");
  const int32_t ds = device_status(derrh);
  if (ds) return ds;
  sm_scatter(tiles.data(), nt, cols, NT, outh.data(), nodes_h.data(), h_first, sm.H, stats, sm.nodes);
  tiles.clear();
  return PHM_OK;
}

int32_t SmTiles::finish_maps() {
  if (!mh) return PHM_OK;
  HIPCHK(tm.start());
  HIPCHK(shard.after_kernel(*mh, map_pad, nullptr));    // sizing: counts -> offsets
  HIPCHK(tm.stop());
  HIPCHK(tm.elapsed(offsets_ms));
  return shard.copy_home(*mh, shard_index, name.c_str());
}

}  // namespace phm_ll
