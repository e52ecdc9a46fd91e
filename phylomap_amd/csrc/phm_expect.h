// phm_expect.h -- kernel parameter blocks and launchers of the exact conditional expectations (phm_expect.hip), behind
// phm_expected_stats (phm_expect_api.cpp).  DESIGN.md section 13.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "phm_sched.h"

namespace phm {

constexpr int EX_MAX_STATES = 64;
constexpr int EX_LANE_MAX = 8;                 // n <= 8: one lane per (branch, site); 9..64: one lane per (branch, site, state)
constexpr double LN2 = 0.69314718055994530942; // a log-likelihood is log(l) + e LN2, e the sum of the passes' base-2 exponents

// the column of E[N_ij], i != j, behind the n dwell columns: row-major with the diagonal left out
__device__ __forceinline__ int count_col(int n, int i, int j) { return n + i * (n - 1) + (j < i ? j : j - 1); }

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

// Points inside branches.  Item k of a launch is the point s on edge row edge[k]; P holds P(s) at [2k] and
// P(t_b - s) at [2k + 1].  post == NULL: a = P(s)^T F_b and beta = P(t_b - s) L_c, each rescaled like the passes' vectors with its
// base-2 exponent (sF_b, sL_c included) beside it.  Otherwise the state posterior a (.) beta / sum(a (.) beta).
struct ExAlongParams {
  int32_t n, Sp;
  const double* P;                             // [2 items][n][n] row-major
  const int32_t* edge;                         // [items] edge row of each item
  const int32_t* child;                        // [n_edge] node row of each edge's child
  const double* F;                             // the passes' F, sF, L, sL (ExPassParams)
  const double* sF;
  const double* L;
  const double* sL;
  double* a;                                   // [item][n][Sp]
  double* sa;                                  // [item][Sp]
  double* beta;                                // [item][n][Sp]
  double* sbeta;                               // [item][Sp]
  double* post;                                // NULL, or [state][rows][Sp]
  int32_t rows;                                // items per state row of post
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
// along-branch vectors or posteriors of `count` items (ExAlongParams)
hipError_t launch_ex_along(const ExAlongParams& p, int count, hipStream_t stream);
// tot[col][r][Sp] += x[col][q - q0][Sp] over the items q of range r (off[r] <= q < off[r + 1]) that lie in [q0, q0 + count), in
// order, for r = r_begin .. r_end - 1; tot has n_ranges rows per column.  The occupancy per boundary and the statistics per bin.
hipError_t launch_ex_range_sum(const double* x, int cols, int count, int64_t q0, const int64_t* off, int r_begin, int r_end,
                               int n_ranges, int Sp, double* tot, hipStream_t stream);

}  // namespace phm
