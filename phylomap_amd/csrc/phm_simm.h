// phm_simm.h -- kernel parameter block and launcher of the forward simulation under many rate matrices (phm_simm.hip), behind
// phm_simulate_histories_models (phm_sim_models_api.cpp).  DESIGN.md section 22.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "phm_maps.h"
#include "phm_sched.h"
#include "phm_sim.h"

namespace phm {

constexpr int SIMM_BLOCK = 256;                // 4 wavefronts, each on an item of its own

// One chunk of histories on one device.  History i of the chunk is global history h = h0 + i (lane i & 63 of tile i >> 6): its
// model is h / n_rep_model, its Philox replica word replica_offset + h.  Passed by value.
struct SimmParams {
  int32_t n_states, n_tips, n_node, n_edge;
  int32_t root;                                // internal index of the root (node id n_tips + 1 + root)
  int32_t n_hist, n_hist_pad;                  // histories of the chunk; rows of the per-history buffers (multiple of 64)
  uint32_t h0;                                 // global index of history 0 of the chunk
  uint32_t n_rep_model;                        // R: histories per model
  uint32_t k0;                                 // global index of the model in lane 0 of the tables
  int32_t Kp;                                  // models in the tables, padded to a multiple of 64
  uint32_t replica_offset;                     // phm_options.replica_offset
  uint32_t seed_lo, seed_hi;
  int64_t map_row0;                            // maps: history 0 of the chunk relative to the shard's first history
  int64_t map_pad;                             // MAPS_COUNT: row length of maps.seg_cnt (histories of the shard, padded)
  double fx_scale, fx_inv;                     // fixed-point scale of the dwell accumulators (powers of two)
  const DownStep* down;                        // pre-order of the branches (phm_sched.h)
  const int32_t* order;                        // positions into down[], grouped by the depth of the parent
  const double* edge_length;                   // by edge row
  const double* qoff;                          // [n n][Kp] jump weights, row-major (from, to), diagonal 0
  const double* qtot;                          // [n][Kp] row totals of qoff, summed left to right
  const double* inv_rate;                      // [n][Kp] 1 / (-q_ss), 0 for an absorbing state
  const double* pid;                           // [n][Kp] root prior
  const double* ptot;                          // [Kp] its total, summed left to right
  uint8_t* nstate;                             // [node id - 1][n_hist_pad] 0-based true states (launch_sim_transpose's layout)
  unsigned long long* dwfx;                    // [n][n_hist_pad] dwell sums, fixed point
  uint32_t* cnt;                               // [n n][n_hist_pad] jump counts, row-major (from, to)
  double* out;                                 // [n + n n + 1][n_hist_pad]: the simulator's columns
  uint32_t* err;                               // device error bits
  unsigned long long* cap;                     // lowest (global model << 32 | edge row) past SIM_MAX_JUMPS (~0: none)
  MapsDev maps;                                // stochastic maps (maps_mode != MAPS_OFF), rows (map_row0 + i) * n_edge + edge row
};

// root, one launch per depth level and the finish; level_off: boundaries of the depth levels in p.order (host); max_group > 0
// caps the edges of one wave item.  Returns the number of launches in *launches when it is not NULL.
hipError_t launch_simulate_models(const SimmParams& p, const std::vector<int32_t>& level_off, int max_group, int maps_mode,
                                  hipStream_t stream, int* launches = nullptr);

}  // namespace phm
