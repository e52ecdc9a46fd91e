// phm_maps_host.h -- host side of the stochastic-map entry points: argument checks that run before any
// device call, the per-shard buffers of the sizing and filling phases, and the fix-up of the shards' offsets.
#pragma once

#include "phm_internal.h"
#include "phm_maps.h"

namespace phm_maps {

// The caller's side of one call.  Sizing: off is written.  Filling: off is read, dwell / state are written.
struct Host {
  int mode = phm::MAPS_OFF;
  int64_t E = 0, R = 0;
  int64_t* off = nullptr;
  double* dwell = nullptr;
  int32_t* state = nullptr;
  std::vector<int64_t> shard_total;      // sizing: the segments of each shard, in shard order
};

// Every check on map_off / map_cap / the segment arrays; `who` names the entry point in the messages.
inline int32_t validate(const char* who, int64_t R, int64_t E, int64_t* map_off, int64_t map_cap, double* dwell, int32_t* state,
                        Host& h) {
  const std::string w(who);
  if (!map_off) return fail(PHM_ERR_BAD_INPUT, w + ": map_off is NULL (it holds R*E + 1 offsets in both phases)");
  if (E < 1 || R < 1) return fail(PHM_ERR_BAD_INPUT, w + ": no rows (R and n_edge must be >= 1)");
  if (R > (INT64_MAX / 16 - 1) / E) return fail(PHM_ERR_BAD_INPUT, w + ": R * n_edge overflows the offsets");
  h.R = R; h.E = E; h.off = map_off;
  if (!dwell && !state) { h.mode = phm::MAPS_COUNT; return PHM_OK; }
  if (!dwell || !state) return fail(PHM_ERR_BAD_INPUT, w + ": filling needs both map_dwell and map_state");
  const int64_t rows = R * E;
  if (map_off[0] != 0) return fail(PHM_ERR_BAD_INPUT, w + ": map_off[0] must be 0");
  for (int64_t k = 0; k < rows; ++k)
    if (map_off[k + 1] < map_off[k])
      return fail(PHM_ERR_BAD_INPUT, w + ": map_off decreases at row " + std::to_string(k) + " (offsets come from a sizing call)");
  if (map_off[rows] > map_cap)
    return fail(PHM_ERR_BAD_INPUT, w + ": map_cap " + std::to_string(map_cap) + " is below map_off[R*E] = " + std::to_string(map_off[rows]));
  h.mode = phm::MAPS_WRITE; h.dwell = dwell; h.state = state;
  return PHM_OK;
}

// Device buffers of one shard: rows [first*E, (first+count)*E) of the call.  pad: the producer's replica padding (count buffer).
struct Shard {
  DevBuf cnt, off, work, dwell, state, bad;
  int64_t first = 0, count = 0, base = 0, total = 0;

  int32_t setup(const Host& h, int64_t first_, int64_t count_, int64_t pad, phm::MapsDev& m) {
    first = first_; count = count_;
    const int64_t rows = count * h.E;
    if (h.mode == phm::MAPS_COUNT) {
      HIPCHK(cnt.alloc(sizeof(uint16_t) * (size_t)h.E * pad));
      HIPCHK(hipMemset(cnt.p, 0, cnt.bytes));
      HIPCHK(off.alloc(sizeof(int64_t) * (size_t)(rows + 1)));
      HIPCHK(work.alloc(phm::maps_offsets_work_bytes((int)count, (int)h.E)));
      m.seg_cnt = cnt.as<uint16_t>();
    } else if (h.mode == phm::MAPS_WRITE) {
      const int64_t* o = h.off + first * h.E;
      base = o[0]; total = o[rows] - base;
      size_t free_b = 0, total_b = 0;
      HIPCHK(hipMemGetInfo(&free_b, &total_b));
      const double need = 12.0 * (double)total + 8.0 * (double)(rows + 1);
      if (need > 0.9 * (double)free_b)
        return fail(PHM_ERR_OOM, "maps: " + std::to_string(total) + " segments (" + std::to_string((int64_t)(need / 1048576.0)) +
                                     " MiB with the offsets) do not fit in the free HBM (" + std::to_string(free_b >> 20) + " MiB)");
      HIPCHK(off.alloc(sizeof(int64_t) * (size_t)(rows + 1)));
      HIPCHK(hipMemcpy(off.p, o, off.bytes, hipMemcpyHostToDevice));
      HIPCHK(dwell.alloc(sizeof(double) * (size_t)total)); HIPCHK(state.alloc(sizeof(int32_t) * (size_t)total));
      HIPCHK(bad.alloc(sizeof(unsigned long long)));
      HIPCHK(hipMemset(bad.p, 0xFF, bad.bytes));
      m.off = off.as<int64_t>(); m.base = base; m.dwell = dwell.as<double>(); m.state = state.as<int32_t>();
      m.bad_row = bad.as<unsigned long long>();
    }
    return PHM_OK;
  }

  // after the producer kernel, on the same stream: the offsets of a sizing launch
  hipError_t after_kernel(const Host& h, int64_t pad, hipStream_t stream) {
    if (h.mode != phm::MAPS_COUNT) return hipSuccess;
    return phm::launch_maps_offsets(cnt.as<uint16_t>(), (int)count, (int)h.E, (int)pad, off.as<int64_t>(), work.p, stream);
  }

  // after the device error word was checked: offsets (sizing) or segments (filling) home
  int32_t copy_home(Host& h, size_t shard_index, const char* who) {
    const int64_t rows = count * h.E;
    if (h.mode == phm::MAPS_COUNT) {
      HIPCHK(hipMemcpy(h.off + first * h.E, off.p, sizeof(int64_t) * (size_t)rows, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(&h.shard_total[shard_index], off.as<int64_t>() + rows, sizeof(int64_t), hipMemcpyDeviceToHost));
    } else if (h.mode == phm::MAPS_WRITE) {
      unsigned long long badh = 0;
      HIPCHK(hipMemcpy(&badh, bad.p, sizeof badh, hipMemcpyDeviceToHost));
      if (badh != ~0ull) {
        const int64_t k = first * h.E + (int64_t)badh;
        return fail(PHM_ERR_BAD_INPUT, std::string(who) + ": the segment count of row " + std::to_string(k) + " (history " +
                                           std::to_string(k / h.E) + ", edge row " + std::to_string(k % h.E + 1) +
                                           ") differs from map_off; the offsets must come from a sizing call with the same inputs and seed");
      }
      if (total > 0) {
        HIPCHK(hipMemcpy(h.dwell + base, dwell.p, dwell.bytes, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(h.state + base, state.p, state.bytes, hipMemcpyDeviceToHost));
      }
    }
    return PHM_OK;
  }
};

// sizing: the shards' relative offsets -> global offsets, and the grand total at map_off[R*E]
inline void finish_sizing(Host& h, const std::vector<phm_shard>& shards) {
  if (h.mode != phm::MAPS_COUNT) return;
  int64_t base = 0;
  for (size_t i = 0; i < shards.size(); ++i) {
    if (base) {
      int64_t* o = h.off + shards[i].first * h.E;
      for (int64_t k = 0; k < shards[i].count * h.E; ++k) o[k] += base;
    }
    base += h.shard_total[i];
  }
  h.off[h.R * h.E] = base;
}

}  // namespace phm_maps
