// phm_ancestral.h -- kernel parameter block and launchers of the ancestral states for many rate matrices at once
// (phm_ancestral.hip), behind phm_ancestral_models (phm_ancestral_api.cpp).  DESIGN.md section 21.
#pragma once

#include "phm_scores.h"

namespace phm {

// Section 17's buffers (ll, with the layout rules of LlParams) and what the joint reconstruction and the node posteriors add.
// Per-evaluation buffers are [row][state][Ev] or [row][Ev], the model index fastest.  A tip's max-product vector is its 0/1 tip
// vector, which ll.L holds in the tip rows (the up pass never writes them), so M and sM have rows for the internal nodes alone.
struct AnParams {
  LlParams ll;
  int32_t root;                                // node row of the root
  double* M;                                   // [internal index][n][Ev] rescaled max-product vectors
  double* sM;                                  // [internal index][Ev] base-2 exponents
  uint32_t* ptr;                               // [edge row][Ev] back pointers: bits [3a, 3a + 3) hold ptr_b(a)
  uint8_t* x;                                  // [node row][Ev] 0-based state of the joint reconstruction
  double* jlogp;                               // [Ev] log of the joint maximum
  const double* O;                             // [node row][n][Ev] outside vectors of launch_sc_down
  const int32_t* sel;                          // [rows of post] node rows to report
  double* post;                                // [selected][n][Ev] O (.) L over its own sum
};

// one height level of the max-product up pass: `steps` (device) holds `count` UpStep entries; writes M, sM and both pointer words
hipError_t launch_an_up(const AnParams& p, const UpStep* steps, int count, hipStream_t stream);
// x_root (the first maximal state of pid_k (.) M_root) and jlogp
hipError_t launch_an_root(const AnParams& p, hipStream_t stream);
// one depth level of the traceback: x_child = ptr_b(x_parent) for the `count` ExDown entries of `steps` (device)
hipError_t launch_an_trace(const AnParams& p, const ExDown* steps, int count, hipStream_t stream);
// node posteriors of selected rows [j0, j0 + count) (after launch_sc_down)
hipError_t launch_an_post(const AnParams& p, int j0, int count, hipStream_t stream);

}  // namespace phm
