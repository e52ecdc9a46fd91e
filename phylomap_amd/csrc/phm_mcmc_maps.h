// phm_mcmc_maps.h -- stochastic maps out of the MCMC samplers: a read-only replay of the branch step's
// state resampling on the iterations a caller records, enqueued by the (tile, branch) launchers between the node draws and the
// branch kernel.
//
// History h = s * J + j is chain s at the j-th recorded iteration; row k = h * E + b its map on edge row b.  The replay reads what
// the branch kernel is about to read (end states, segment counts, the current dwell slot, the chain tables), redraws state i of
// every branch from word i - 1 of the ENT_BSTATE | b stream -- the very draw the branch kernel makes -- merges equal neighbours,
// and stores the row's segment count (MAPS_COUNT) or its (dwell, 1-based state) segments (MAPS_WRITE).  It writes nothing the
// sweep reads.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "phm_maps.h"
#include "phm_tiles.h"
#include "phm_wtiles.h"

namespace phm {

// one recorded sweep
struct McmcMapsLaunch {
  int32_t mode = MAPS_OFF;     // MAPS_COUNT or MAPS_WRITE
  int32_t j = 0, J = 1;        // this sweep's place among the recorded iterations; their number
  MapsDev dev;                 // seg_cnt: [J][edge][n_rep_pad] (coalesced stores); off: the S*J*E + 1 offsets of the engine's histories
};

template <int NS>
hipError_t launch_mcmc_maps_tiles(const TileParams<NS>& p, const McmcMapsLaunch& m, int it, hipStream_t stream);
hipError_t launch_mcmc_maps_wtiles(const WtParams& p, const McmcMapsLaunch& m, int it, hipStream_t stream);

// [J][edge][pad] counts -> [edge][S*J] by history (h = s*J + j), the layout launch_maps_offsets reads
hipError_t launch_mcmc_maps_transpose(const uint16_t* cnt, int S, int J, int E, int pad, uint16_t* out, hipStream_t stream);

}  // namespace phm
