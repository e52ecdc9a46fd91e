// phm_expect.h -- kernel parameter blocks and launchers of the exact conditional expectations (phm_expect.hip), behind
// phm_expected_stats (phm_expect_api.cpp).  DESIGN.md section 13.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "phm_sched.h"

namespace phm {

constexpr int EX_MAX_STATES = 64;
constexpr int EX_LANE_MAX = 8;                 // n <= 8: one lane per (branch, site); 9..64: one lane per (branch, site, state)

struct ExDown {        // one branch of the down pass, grouped by the depth of its child
  int32_t edge;        // edge row (0-based)
  int32_t parent;      // node row of the parent (node id - 1)
  int32_t child;       // node row of the child
  int32_t sib_edge;    // the sibling branch (same parent)
  int32_t sib_child;   // its child's node row
  int32_t pad[3];
};

// Every per-site buffer is [row][state][site] or [row][site] with Sp sites (a multiple of 64) per row.
struct ExPassParams {
  int32_t n, n_tips, Sp;
  const double* P;                             // [n_edge][n][n] row-major: expm(Q t_b)
  double* L;                                   // [node row][n][Sp] rescaled partial likelihoods (tips filled first)
  double* sL;                                  // [node row][Sp] their base-2 exponents (integer-valued)
  double* O;                                   // [node row][n][Sp] rescaled outside vectors
  double* sO;                                  // [node row][Sp]
  double* F;                                   // [edge row][n][Sp] F_b = O_parent (.) P(t_sib) L_sib
  double* sF;                                  // [edge row][Sp]
  double* ll;                                  // [Sp] log p(tips | Q)
  double* lam;                                 // [Sp] pid . L_root (rescaled): p(tips | Q) = lam 2^sL[root]
};

struct ExBranchParams {
  int32_t n, Sp;
  int32_t e0;                                  // first edge row of this launch (outputs are relative to it)
  double mu;                                   // max_i(-q_ii)
  const double* B;                             // [n][n] row-major, I + Q / mu
  const double* qoff;                          // [n][n] row-major, Q with a zero diagonal
  const int64_t* w_off;                        // [n_edge + 1] into w: branch b keeps w_0 .. w_{M_b}
  const double* w;                             // pois(m + 1; mu t_b) / mu
  const int32_t* child;                        // [n_edge] node row of each edge's child
  const double* L;
  const double* sL;
  const double* F;
  const double* sF;
  const double* lam;
  int32_t root;                                // node row of the root
  double* out;                                 // [col][edge - e0][Sp], cols = n + n(n-1) (man/sumstatMCMC.Rd:18 order)
  int32_t n_out_edges;                         // rows per column of `out`
};

// L rows of the tips: 1 where observe[a] == y, all ones for y = 0 (tips [T][Sp], obs [n])
hipError_t launch_ex_tips(const ExPassParams& p, const uint8_t* tips, const int32_t* obs, hipStream_t stream);
// one height level of the up pass: `steps` (device) holds `count` UpStep entries
hipError_t launch_ex_up(const ExPassParams& p, const UpStep* steps, int count, hipStream_t stream);
// O_root = pid (normalised) and ll = log(pid . L_root) + sL_root
hipError_t launch_ex_root(const ExPassParams& p, int root_row, const double* pid, hipStream_t stream);
// one depth level of the down pass
hipError_t launch_ex_down(const ExPassParams& p, const ExDown* steps, int count, hipStream_t stream);
// post[(state * rows + row) * Sp + site] = O (.) L / sum(O (.) L)  (= O (.) L exp(sO + sL - ll))
hipError_t launch_ex_post(const ExPassParams& p, int rows, double* post, hipStream_t stream);
// branch stage for edge rows [e0, e0 + count)
hipError_t launch_ex_branch(const ExBranchParams& p, int count, hipStream_t stream);
// tot[col][Sp] += out[col][e][Sp] for e = 0 .. count - 1, in edge order
hipError_t launch_ex_reduce(const double* out, int cols, int count, int Sp, double* tot, hipStream_t stream);

}  // namespace phm
