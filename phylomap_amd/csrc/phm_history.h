// phm_history.h -- the per-lane statistics accumulators of the producers whose waves share a history (simm_level_kernel and
// sm_branch_kernel; exp_tiles_branch_kernel keeps a copy of its own; DESIGN.md sections 14, 19 and 22): dwell sums in 64-bit fixed point (exact in any
// order, so the same bits under any grouping, chunking and device count) and uint32 counts, in cells [col][pad] of the launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace phm {

// One lane's statistics over the branches of one wave item.  NS > 0 (2..4 states, compile-time): NS dwell sums and NC_ counters in
// registers (selects, no dynamic register indexing) that reach the cells once per item (flush); NS = 0 (run-time n up to 64): one
// atomic per segment.  The count-column formula is the caller's.  A lane that is not live adds to no cell.
template <int NS, int NC_>
struct StatLanes {
  static constexpr int NA = NS > 0 ? NS : 1, NC = NS > 0 ? NC_ : 1;
  unsigned long long acc_dw[NA] = {};
  uint32_t acc_ct[NC] = {};
  unsigned long long* dw;                 // the lane's cell of dwell column 0; column c at dw[c * pad]
  uint32_t* ct;                           // the lane's cell of count column 0
  size_t pad;
  double fx_scale;                        // dwell -> fixed point (a power of two)
  bool live;

  __device__ __forceinline__ void begin(unsigned long long* dwfx, uint32_t* cnt, size_t cell_pad, size_t cell, double scale,
                                        bool is_live = true) {
    dw = dwfx + cell; ct = cnt + cell; pad = cell_pad; fx_scale = scale; live = is_live;
  }
  __device__ __forceinline__ void dwell(int col, double x) {
    const unsigned long long fx = (unsigned long long)__double2ll_rn(x * fx_scale);
    if constexpr (NS > 0) {
#pragma unroll
      for (int c = 0; c < NA; ++c) acc_dw[c] += (col == c) ? fx : 0ull;
    } else {
      if (live) atomicAdd(dw + (size_t)col * pad, fx);
    }
  }
  __device__ __forceinline__ void count(int col) {
    if constexpr (NS > 0) {
#pragma unroll
      for (int c = 0; c < NC; ++c) acc_ct[c] += (col == c) ? 1u : 0u;
    } else {
      if (live) atomicAdd(ct + (size_t)col * pad, 1u);
    }
  }
  __device__ __forceinline__ void flush() {
    if constexpr (NS > 0) {
      if (live) {
#pragma unroll
        for (int c = 0; c < NA; ++c) if (acc_dw[c]) atomicAdd(dw + (size_t)c * pad, acc_dw[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) if (acc_ct[c]) atomicAdd(ct + (size_t)c * pad, acc_ct[c]);
      }
    }
  }
};

// column c < n + counts of a history's statistics out of its accumulator cells: a dwell sum back from fixed point, or a count
__device__ __forceinline__ double stat_cell_value(const unsigned long long* dwfx, const uint32_t* cnt, int n, int c, size_t pad,
                                                  size_t cell, double fx_inv) {
  return c < n ? (double)(long long)dwfx[(size_t)c * pad + cell] * fx_inv : (double)cnt[(size_t)(c - n) * pad + cell];
}

}  // namespace phm
