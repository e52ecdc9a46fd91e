// phm_sample.h -- kernel parameter block and launchers of the exact sampler of histories over many rate matrices and sites
// (phm_sample.hip), behind phm_sample_histories_models (phm_sample_api.cpp).  DESIGN.md section 19.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "phm_loglik.h"
#include "phm_maps.h"
#include "phm_sched.h"

namespace phm {

constexpr int SM_BLOCK = 256;
constexpr double SM_MAX_JUMP_MEAN = 32768.0;   // max(-q_ii) t_b: bounds the loops, the table and a row's uint16 segment count
constexpr int SM_M_CAP = 1 << 17;              // hard end of the stopping rule's loop (M(32768) is about 34 000)

constexpr uint32_t SM_LANE_IDLE = 0xFFFFFFFFu;  // packed form: lane_id of a lane without a chain (evaluation ids keep to 31 bits)

// A tile: 64 consecutive draws of ONE evaluation (lane = draw d0 + lane; lanes >= n_valid idle).
// Packed form (SmParams.packed, section 20): 64 consecutive chains of one site, ONE draw each: lane's evaluation is ev + lane, its
// model k + lane, its evaluation id lane_id[tile * 64 + lane]; d0 = 0 and n_valid, row0 are not read.
struct SmTile {
  int32_t ev;            // evaluation in section 17's buffers of this launch: site_local * Kp + k
  int32_t k;             // model in the chunk (lane of the per-model buffers)
  uint32_t eval_id;      // GLOBAL evaluation id site * K + model: the iteration word of every stream
  int32_t d0;            // first draw of the tile
  int32_t n_valid;       // draws of the tile (1..64)
  int32_t pad;
  int64_t row0;          // history of lane 0, relative to the shard's first history (maps rows, (row0 + lane) * n_edge + b)
};

// the jump-count series ends at M(x): the last index kept by section 18's rule, as a function of x = mu t alone.
// r_0 = 1, r_m = r_{m-1} (x / m), S_M = r_0 + .. + r_M (all divided by 2^512 whenever r passes 2^512);
// M = the first m >= 1 with x < m + 1 and r_{m+1} <= 2^-60 S_m (1 - x / (m + 2)); M(0) = 0.
__host__ __device__ inline int sm_stop_index(double x) {
  if (!(x > 0.0)) return 0;
  double r = x, S = 1.0 + x;
  for (int m = 1; m < SM_M_CAP; ++m) {
    const double rn = r * (x / (double)(m + 1));
    if (x < (double)(m + 1) && rn <= 0x1p-60 * S * (1.0 - x / (double)(m + 2))) return m;
    r = rn;
    S += r;
    if (r > 0x1p512) { r *= 0x1p-512; S *= 0x1p-512; }
  }
  return SM_M_CAP;
}

// What the narrow and the wide sampler's parameter blocks share: the tiles of a launch, the streams, the accumulators and the
// outputs (filled on the host by SmTiles::fill_core, phm_sample_host.h).
struct SmCore {
  int32_t n_node, n_edge, root_row;            // root_row: n_tips + internal index of the root
  int32_t n_tiles;
  int64_t map_pad;                             // MAPS_COUNT: row length of maps.seg_cnt (histories of the shard, padded)
  uint32_t seed_lo, seed_hi, replica;          // replica: phm_options.replica_offset, added to the draw index
  double fx_scale, fx_inv;                     // fixed-point scale of the dwell accumulators (powers of two)
  const SmTile* tiles;                         // [n_tiles]
  const DownStep* down;                        // [n_edge] pre-order
  const int32_t* order;                        // positions into down[], grouped by the depth of the parent
  uint8_t* nstate;                             // [tile][n_tips + n_node][64] 0-based states by ape row
  unsigned long long* dwfx;                    // [n][n_tiles * 64] dwell sums, fixed point
  uint32_t* cnt;                               // [n (n-1)][n_tiles * 64]
  double* out;                                 // [cols][n_tiles * 64]; packed: one more column (the lanes' ll) and one more value, the error word
  int32_t* nodes;                              // NULL or [n_tiles * 64][n_tips + n_node] 1-based states
  uint32_t* err;
  MapsDev maps;
};

struct SmParams {
  LlParams ll;                                 // section 17's buffers, read in place: P [edge][n n][Kp], L [row][n][Ev], pid [n][Kp]
  SmCore core;
  int32_t depth;                               // rows of beta: m = 0 .. depth
  int32_t* depth_of;                           // [Kp] every model's own depth M(mu_k max_b t_b) <= depth (packed: written by the table kernel)
  int32_t packed;                              // 1: lane = chain (phm_gibbs_rates); a lane whose ll is not finite, or whose id is SM_LANE_IDLE, idles
  double t_max;                                // packed: max_b t_b, from which the table kernel takes depth_of (DERR_CAPACITY above depth)
  const uint32_t* lane_id;                     // packed: [n_tiles * 64] GLOBAL evaluation ids
  double* mu;                                  // [Kp]
  double* B;                                   // [n n][Kp] I + Q / mu (I when mu = 0)
  double* beta;                                // [depth + 1][n n][Kp]: entry c n + e of row m is (B^m)[c, e]
};

// fixed point -> double, counters -> double, node bytes -> 1-based int32 of the tiles of c (n states, n_tips tips), for both
// samplers.  packed_ll non-NULL (the narrow packed form only): the accumulators are zeroed for the next iteration, and the lanes'
// ll (packed_ll[tile.ev + lane]) and the error word ride along in c.out.
hipError_t launch_sm_finish(const SmCore& c, int n, int n_tips, const double* packed_ll, hipStream_t stream);

// mu, B and beta of the models of the chunk (a lane owns a model), each to its own depth
hipError_t launch_sm_table(const SmParams& p, hipStream_t stream);
// root, node levels, branches and the finish of the tiles of p (packed: maps_mode MAPS_OFF only; the finish also clears the
// accumulators for the next iteration); level_off: boundaries of the depth levels in p.order (host)
hipError_t launch_sm_sample(const SmParams& p, const std::vector<int32_t>& level_off, int branch_blocks, int maps_mode,
                            hipStream_t stream);

}  // namespace phm
