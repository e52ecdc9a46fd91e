// phm_sim.h -- kernel parameter block and launchers of the forward simulation of character histories (phm_sim.hip),
// behind phm_simulate_histories (phm_sim_api.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "phm_device.h"
#include "phm_maps.h"
#include "phm_sched.h"

namespace phm {

constexpr int SIM_BLOCK = 256;                 // 4 wavefronts (4 tiles of 64 replicas) share one LDS copy of Q
constexpr int SIM_MAX_STATES = 64;
constexpr int SIM_MAX_JUMPS = 9999;            // samplethebranch stops after 10 000 draws (R/sourceme.R:356): 9 999 jumps + the last piece
constexpr uint32_t SIM_ITER = 0xFFFFFFFFu;     // Philox iteration word of every simulation stream (an MCMC sweep never reaches it)

// Passed by value (kernarg segment): the schedule and the tables are read through scalar loads / LDS.
struct SimParams {
  int32_t n_states, n_tips, n_node, n_edge;
  int32_t root;                                // internal index of the root (node id n_tips + 1 + root)
  int32_t n_rep, n_rep_pad;                    // replicas of this launch; rows of the per-replica buffers (multiple of 64)
  uint32_t replica_offset;                     // global id of replica 0 (Philox replica word)
  uint32_t seed_lo, seed_hi;
  const DownStep* down;                        // pre-order of the branches (phm_sched.h)
  const double* qoff;                          // n x n row-major, diagonal 0: the jump weights of row s
  const double* inv_rate;                      // 1 / (-q_ss), 0 for an absorbing state
  const double* pid;                           // root prior
  const double* edge_length;                   // by edge row
  uint8_t* nstate;                             // [node id - 1][n_rep_pad] 0-based true states
  double* stats;                               // [col][n_rep_pad]: dwell (n), counts (n x n, row-major from,to), root state
  uint32_t* err;                               // [0] device error bits; [1] lowest edge row (0-based) past SIM_MAX_JUMPS
  MapsDev maps;                                // stochastic maps (maps_mode != MAPS_OFF), rows r * n_edge + edge row
};

// maps_mode: MapMode (phm_maps.h); MAPS_OFF is the plain simulation
hipError_t launch_simulate(const SimParams& p, hipStream_t stream, int maps_mode = MAPS_OFF);
// out[r * rows + i] = map[nstate[i][r]] for i < rows, r < n_rep (replica-major int32; map: n 1-based states)
hipError_t launch_sim_transpose(const uint8_t* nstate, int rows, int n_rep, int n_rep_pad, const int32_t* map, int32_t* out,
                                hipStream_t stream);

}  // namespace phm
