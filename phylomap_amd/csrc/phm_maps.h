// phm_maps.h -- stochastic maps out of the producers of character histories: the device side of the sizing /
// filling contract of the six producer kernels, written once (MapRow): sim_kernel (phm_sim.hip), simm_level_kernel (phm_simm.hip),
// sm_branch_kernel (phm_sample.hip), mcmc_maps_tiles_kernel and mcmc_maps_wtiles_kernel (phm_mcmc_maps.hip); exp_tiles_branch_kernel
// (phm_exp.hip) has the same rule in a copy of its own (see there).
//
// Row k = r * E + b holds history r's segments on edge row b.  A sizing launch stores every row's segment count into a
// [edge][replica_pad] uint16 buffer (one coalesced row per wave and branch); launch_maps_offsets turns it into replica-major
// int64 exclusive offsets.  A filling launch walks the same draws with a write cursor per lane that starts at the row's offset,
// stores (dwell, 1-based state) per segment while it stays below the row's end, and reports the first row whose count differs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>
#include <vector>

namespace phm {

enum MapMode { MAPS_OFF = 0, MAPS_COUNT = 1, MAPS_WRITE = 2 };

// what a producer kernel needs for its maps (pointers are device buffers of one shard; unused ones NULL)
struct MapsDev {
  uint16_t* seg_cnt = nullptr;            // MAPS_COUNT: [edge][replica_pad] segments per (branch, replica)
  const int64_t* off = nullptr;           // MAPS_WRITE: the R*E + 1 caller offsets of the shard's rows
  int64_t base = 0;                       // MAPS_WRITE: off[0], the shard's first segment in the caller's arrays
  double* dwell = nullptr;                // MAPS_WRITE: segment dwell times
  int32_t* state = nullptr;               // MAPS_WRITE: segment states, 1-based
  unsigned long long* bad_row = nullptr;  // MAPS_WRITE: lowest shard row whose count differs from `off` (~0 = none)
};

// One lane's sink for one row of the maps.  MAPS_COUNT: counts the segments; end() stores the count at seg_cnt[cnt_at] (a replayed
// launch overwrites).  MAPS_WRITE: a cursor from off[row] - base; emit() stores while the cursor is below the row's end and end()
// reports a row whose count differs (the lowest row of the launch wins).  A lane that is not live gets an empty row: it stores no
// segment and reports nothing; whether it stores its count is the caller's (it guards end()).  MAPS_OFF compiles to nothing.
template <int MODE>
struct MapRow {
  const MapsDev* m;
  int64_t row, cur, stop;
  bool live;

  __device__ __forceinline__ void begin(const MapsDev& maps, int64_t shard_row, bool is_live = true) {
    m = &maps; row = shard_row; live = is_live; cur = 0; stop = 0;
    if constexpr (MODE == MAPS_WRITE) {
      if (live) { cur = maps.off[row] - maps.base; stop = maps.off[row + 1] - maps.base; }
    }
  }
  __device__ __forceinline__ void emit(double dwell, int state0) {
    if constexpr (MODE == MAPS_WRITE) {
      if (cur < stop) { m->dwell[cur] = dwell; m->state[cur] = state0 + 1; }
    }
    if constexpr (MODE != MAPS_OFF) ++cur;
  }
  __device__ __forceinline__ void end(size_t cnt_at) {
    if constexpr (MODE == MAPS_COUNT) m->seg_cnt[cnt_at] = (uint16_t)cur;
    if constexpr (MODE == MAPS_WRITE) {
      if (live && cur != stop) atomicMin(m->bad_row, (unsigned long long)row);
    }
  }
};

// A launcher's way from the run-time mode to the kernel instantiation: f(std::integral_constant<int, mode>).  with_producer_form:
// f(mode, ns), ns the state count of the kernel's form: n for 2..4 states (compile-time accumulators), 0 for the run-time form.
template <class F>
inline void with_map_mode(int maps_mode, F&& f) {
  if (maps_mode == MAPS_COUNT) f(std::integral_constant<int, MAPS_COUNT>{});
  else if (maps_mode == MAPS_WRITE) f(std::integral_constant<int, MAPS_WRITE>{});
  else f(std::integral_constant<int, MAPS_OFF>{});
}

template <class F>
inline void with_producer_form(int maps_mode, int n_states, F&& f) {
  with_map_mode(maps_mode, [&](auto mode) {
    if (n_states == 2) f(mode, std::integral_constant<int, 2>{});
    else if (n_states == 3) f(mode, std::integral_constant<int, 3>{});
    else if (n_states == 4) f(mode, std::integral_constant<int, 4>{});
    else f(mode, std::integral_constant<int, 0>{});
  });
}

// off[r * E + b] = sum of cnt over rows before (r, b) in replica-major order, off[R * E] = the total; cnt is [edge][pad] with
// pad >= R.  `work` must hold maps_offsets_work_bytes(R, E) bytes.
size_t maps_offsets_work_bytes(int R, int E);
hipError_t launch_maps_offsets(const uint16_t* cnt, int R, int E, int pad, int64_t* off, void* work, hipStream_t stream);

}  // namespace phm
