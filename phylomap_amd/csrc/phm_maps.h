// phm_maps.h -- stochastic maps out of the samplers: the device side of the sizing / filling contract of
// phm_simulate_histories_maps and phm_maketreelistEXP_maps, shared by both producers.
//
// Row k = r * E + b holds history r's segments on edge row b.  A sizing launch stores every row's segment count into a
// [edge][replica_pad] uint16 buffer (one coalesced row per wave and branch); launch_maps_offsets turns it into replica-major
// int64 exclusive offsets.  A filling launch walks the same draws with a write cursor per lane that starts at the row's offset,
// stores (dwell, 1-based state) per segment while it stays below the row's end, and reports the first row whose count differs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
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

// off[r * E + b] = sum of cnt over rows before (r, b) in replica-major order, off[R * E] = the total; cnt is [edge][pad] with
// pad >= R.  `work` must hold maps_offsets_work_bytes(R, E) bytes.
size_t maps_offsets_work_bytes(int R, int E);
hipError_t launch_maps_offsets(const uint16_t* cnt, int R, int E, int pad, int64_t* off, void* work, hipStream_t stream);

}  // namespace phm
