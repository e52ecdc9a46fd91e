// phm_sim_walk.h -- the branch walk of the forward simulation (samplethebranch, R/sourceme.R:346-414), written
// once for sim_kernel (phm_sim.hip: one model, tables in LDS) and simm_level_kernel (phm_simm.hip: a model per lane, model-fastest
// tables in global memory).  Device code only.
#pragma once

#include "phm_sim.h"

namespace phm {

// first j with u * total <= w_0 + .. + w_j, w_j at w[j stride], `total` summed left to right beforehand
template <int NS>
__device__ __forceinline__ int sim_categorical(const double* __restrict__ w, size_t stride, double total, int n_rt, double u,
                                               uint32_t& err) {
  const int n = NS > 0 ? NS : n_rt;
  if (!(total > 0.0) || isinf(total)) err |= DERR_ZERO_PROB;
  const double thr = u * total;
  double cum = w[0];
  int idx = (thr <= cum) ? 0 : 1;
#pragma unroll
  for (int j = 1; j < n - 1; ++j) { cum += w[(size_t)j * stride]; idx += (thr <= cum) ? 0 : 1; }
  return idx;
}

// A lane's model: entry (row, model k) of a table sits at [row * stride + k] -- stride 1 and k = 0 for one model's own tables.
struct SimModel {
  const double *qoff, *qtot, *inv;        // jump weights of (from, to) at row from * n + to, their row totals, 1 / (-q_ss) or 0
  size_t stride;
  int k, n;
  __device__ __forceinline__ double inv_rate(int s) const { return inv[(size_t)s * stride + k]; }
  __device__ __forceinline__ const double* weights(int s) const { return qoff + (size_t)(s * n) * stride + k; }
  __device__ __forceinline__ double total(int s) const { return qtot[(size_t)s * stride + k]; }
};

// The Gillespie walk of one branch of length t from state s on the opened ENT_BSTATE stream `rs`: draw 2j is the waiting time
// of jump j, draw 2j + 1 its target.  on_segment(state, dwell) per piece -- the last one is the reference's
// seg_len - (dab - branchlength), or the rest of the branch in an absorbing state, which takes no draw --, on_jump(from, to) per
// jump, on_capacity() when the branch would take more than SIM_MAX_JUMPS jumps (the walk stops there).  Returns the end state.
template <int NS, class OnSegment, class OnJump, class OnCapacity>
__device__ __forceinline__ int sim_walk_branch(int s, double t, Stream& rs, const double* ltab, const SimModel& md,
                                               OnSegment on_segment, OnJump on_jump, OnCapacity on_capacity, uint32_t& err) {
  double pos = 0.0;
  for (uint32_t j = 0;; ++j) {
    const double ir = md.inv_rate(s);
    if (ir == 0.0) { on_segment(s, t - pos); break; }             // absorbing: the rest of the branch, no draw
    const double gap = ir * neglog_u32(rs.draw_word(2u * j), ltab);
    const double dab = pos + gap;
    if (!(dab < t)) { on_segment(s, gap - (dab - t)); break; }    // seg_len - (dab - branchlength)
    on_segment(s, gap);
    if (j == (uint32_t)SIM_MAX_JUMPS) { err |= DERR_CAPACITY; on_capacity(); break; }
    const int nx = sim_categorical<NS>(md.weights(s), md.stride, md.total(s), md.n, rs.draw(2u * j + 1u), err);
    on_jump(s, nx);
    s = nx;
    pos = dab;
  }
  return s;
}

}  // namespace phm
