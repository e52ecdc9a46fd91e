// phm_ancestral_wide.h -- kernel parameter block and launchers of the ancestral states for many rate matrices at 9..64 states
// (phm_ancestral_wide.hip), behind phm_ancestral_models_wide (phm_ancestral_wide_api.cpp).  DESIGN.md section 23.
#pragma once

#include <type_traits>

#include "phm_expect.h"

namespace phm {

constexpr int AW_MIN_STATES = 9;               // below: phm_ancestral_models (models across the lanes)
constexpr int AW_GRID_MAX = 65535;             // models, site tiles and selected rows of one launch

// lanes of one (evaluation, node) item: ex_branch_wide_kernel's classes
inline int aw_lanes(int n) { return n <= 16 ? 16 : n <= 32 ? 32 : 64; }

// f(std::integral_constant<int, NP>) of the lane class, its value returned: constexpr int NP_ = decltype(np)::value
template <class F>
inline auto aw_with_lanes(int NP, F&& f) {
  if (NP == 16) return f(std::integral_constant<int, 16>{});
  if (NP == 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

// One state per lane.  An evaluation of the chunk is ev = model * Sc + site (Ev = Kc * Sc of them); every vector is a contiguous
// row of NP doubles, the states past n zero.  Exponents are base-2 integers.  A tip's max-product vector is its row of L, so M
// and sM have rows for the internal nodes alone.
struct AwParams {
  int32_t n, NP, n_tips, n_edge;
  int32_t root;                                // node row of the root
  int32_t Kc, Sc;                              // models and sites per model of this chunk
  int32_t tip_model, tip_site;                 // tip row of (model k, site s) = k * tip_model + s * tip_site
  const double* P;                             // [model][edge][n][n] row-major
  const double* pid;                           // [model][n] normalised
  const uint8_t* tips;                         // [tip row][n_tips] observations, 0: missing
  const int32_t* obs;                          // [n] observation of each state
  double* L;                                   // [node row][Ev][NP] rescaled partial likelihoods
  int32_t* sL;                                 // [node row][Ev]
  double* ll;                                  // [Ev] log p(tips)
  double* lam;                                 // [Ev] pid . L_root (rescaled: ll before the log and the exponent); NULL: not stored
  double* O;                                   // [node row][Ev][NP] rescaled outside vectors
  int32_t* sO;                                 // [node row][Ev]
  double* F;                                   // [edge row][Ev][NP] F_b = O_parent (.) P(t_sib) L_sib, rescaled; NULL: not stored
  int32_t* sF;                                 // [edge row][Ev]
  const int32_t* sel;                          // [J] node rows to report
  int32_t J;
  double* post;                                // [Ev][J][n] O (.) L over its own sum
  double* M;                                   // [internal index][Ev][NP] rescaled max-product vectors
  int32_t* sM;                                 // [internal index][Ev]
  uint8_t* ptr;                                // [edge row][Ev][NP] back pointers, one byte per parent state
  uint8_t* x;                                  // [node row][Ev] 0-based state of the joint reconstruction
  double* jlogp;                               // [Ev] log of the joint maximum
};

// allows `fn` up to `bytes` of dynamic LDS on the current device (above the 64 KiB a launch gets unasked); once per (function, device)
hipError_t aw_allow_lds(const void* fn, int bytes);
// tip rows of L and sL
hipError_t launch_aw_tips(const AwParams& p, hipStream_t stream);
// one height level of the sum-product (joint = false: L, sL) or max-product (joint = true: M, sM, ptr) up pass: `steps` (device)
// holds `count` UpStep entries
hipError_t launch_aw_up(const AwParams& p, const UpStep* steps, int count, bool joint, hipStream_t stream);
// log p(tips) of every evaluation; with O not NULL also the root's outside vector (pid, exponent 0), with lam not NULL also lam
hipError_t launch_aw_root(const AwParams& p, hipStream_t stream);
// one depth level of the down pass: O and sO of the children of `count` ExDown entries of `steps` (device); with F not NULL
// also F and sF of their edge rows
hipError_t launch_aw_down(const AwParams& p, const ExDown* steps, int count, hipStream_t stream);
// node posteriors of selected rows [j0, j0 + count)
hipError_t launch_aw_post(const AwParams& p, int j0, int count, hipStream_t stream);
// x_root (the smallest maximal state of pid_k (.) M_root) and jlogp
hipError_t launch_aw_jroot(const AwParams& p, hipStream_t stream);
// one depth level of the traceback: x_child = ptr_b(x_parent) for the `count` ExDown entries of `steps` (device)
hipError_t launch_aw_trace(const AwParams& p, const ExDown* steps, int count, hipStream_t stream);

}  // namespace phm
