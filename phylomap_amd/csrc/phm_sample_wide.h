// phm_sample_wide.h -- kernel parameter block and launchers of the exact sampler of histories over many rate matrices and sites at
// 9..64 states (phm_sample_wide.hip), behind phm_sample_histories_models_wide (phm_sample_wide_api.cpp).  DESIGN.md section 24.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "phm_ancestral_wide_host.h"
#include "phm_maps.h"
#include "phm_sample.h"
#include "phm_sched.h"

namespace phm {

constexpr int SW_TABLE_BLOCK = 256;            // lanes of the workgroup that owns a model's table
constexpr int SW_NODE_BLOCK = 256;             // four waves, one (tile, edge of the level) each
constexpr int SW_BRANCH_BLOCK = 64;            // a workgroup is ONE wave: its LDS copy of B belongs to the item's model
constexpr int64_t SW_ITEMS_MAX = (int64_t)1 << 30;   // (tile, branch) items of one launch: a grid dimension

// row stride (doubles) of B in LDS: odd, so lanes on different rows of one column fall on different bank pairs
__host__ __device__ inline int sw_row_stride(int n) { return n | 1; }

// doubles of a model's table: rows m = 0 .. depth of n * n
inline size_t sw_table_doubles(int n, int depth) { return ((size_t)depth + 1) * (size_t)n * n; }
// dynamic LDS of the table kernel: B (padded rows) and the two ping-pong rows beta_m, beta_{m+1}
inline size_t sw_table_lds_bytes(int n) { return sizeof(double) * ((size_t)n * sw_row_stride(n) + 2 * (size_t)n * n); }
// dynamic LDS of the branch kernel: B (padded rows); the neglog table is static
inline size_t sw_branch_lds_bytes(int n) { return sizeof(double) * (size_t)n * sw_row_stride(n); }

// A tile is phm_sample.h's SmTile: 64 consecutive draws of one evaluation; ev is section 23's index model * Sc + site of the
// launch and k the model in the chunk.
struct SwParams {
  SmCore core;                                 // phm_sample.h: tiles, streams, accumulators and outputs
  int32_t n, NP, n_tips;
  int32_t Kc;
  size_t Ev;                                   // evaluations of the launch (Kc * Sc): row length of L
  const double* Q;                             // [model][n][n] row-major
  const double* P;                             // [model][edge][n][n] row-major (section 23)
  const double* pid;                           // [model][n] normalised
  const double* L;                             // [node row][Ev][NP] rescaled partial likelihoods (section 23)
  const double* t;                             // [n_edge]
  double* mu;                                  // [model]
  double* B;                                   // [model][n][n] row-major: I + Q / mu (I when mu = 0)
  const int32_t* depth_of;                     // [model] M(mu_k max_b t_b): the last row of the model's table
  size_t tab_stride;                           // doubles between the tables of two models in `beta`
  double* beta;                                // model k, row m: [e][c] = (B_k^m)[c, e], the n weights of a state draw contiguous
  // sites form only (section 25): a tile is 64 consecutive SITES of one chain, ev its first evaluation, eval_id that site's id
  const double* ll;                            // [Ev] log-likelihoods of the evaluations: a lane whose own is not finite idles
  uint32_t lane_stride;                        // the evaluation id of lane l is tile.eval_id + l * lane_stride (the chains of the call)
};

// mu, B and the table of models [0, Kc) of the chunk, a workgroup per model
hipError_t launch_sw_table(const SwParams& p, hipStream_t stream);
// root, node levels, branches and the finish of the tiles of p; level_off: boundaries of the depth levels in p.order (host)
hipError_t launch_sw_sample(const SwParams& p, const std::vector<int32_t>& level_off, int maps_mode, hipStream_t stream);
// Sites form, one iteration of phm_gibbs_rates_wide: root, node levels and branches of the tiles of p, one draw per evaluation
// (p.core.replica is every lane's replica word), then the finish and the reduction: red [Kc][cols + 1] (every chain's columns and
// its log-likelihood summed over its `sites` evaluations, one after the other, sites ascending) and one more value, the error
// word.  The accumulators are left zeroed for the next iteration.  Chain k owns tiles [k, k + 1) * tiles_per_chain.
hipError_t launch_sw_sample_sites(const SwParams& p, const std::vector<int32_t>& level_off, int sites, int tiles_per_chain, double* red,
                                  hipStream_t stream);

}  // namespace phm

namespace phm_ll {

// The sampler's device state per model of a chunk (mu, B, the depths and the table), next to AwLanes' (the drivers of
// phm_sample_wide_api.cpp and phm_gibbs_wide_api.cpp).
struct SwModels {
  DevBuf dmu, dB, dbeta, ddepth;
  size_t tab_stride = 0;                       // doubles of a model's table

  int32_t alloc(int n, size_t Km, size_t tab_doubles) {
    tab_stride = tab_doubles;
    HIPCHK(dmu.alloc(sizeof(double) * Km)); HIPCHK(dB.alloc(sizeof(double) * (size_t)n * n * Km));
    HIPCHK(dbeta.alloc(sizeof(double) * tab_stride * Km)); HIPCHK(ddepth.alloc(sizeof(int32_t) * Km));
    return PHM_OK;
  }
  // what every chunk shares of sp: the state count and section 23's buffers of ln, and this state
  void fill(phm::SwParams& sp, const AwLanes& ln) const {
    sp.n = ln.in.n; sp.NP = phm::aw_lanes(ln.in.n); sp.n_tips = ln.in.T;
    sp.Q = ln.dQ.as<double>(); sp.P = ln.dP.as<double>(); sp.pid = ln.dpid.as<double>(); sp.L = ln.dL.as<double>(); sp.t = ln.dt.as<double>();
    sp.mu = dmu.as<double>(); sp.B = dB.as<double>(); sp.depth_of = ddepth.as<int32_t>(); sp.tab_stride = tab_stride; sp.beta = dbeta.as<double>();
  }
};

}  // namespace phm_ll
