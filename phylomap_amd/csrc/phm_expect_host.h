// phm_expect_host.h -- host side shared by the two entry points of the exact conditional expectations: phm_expected_stats
// (phm_expect_api.cpp) and phm_expected_through_time (phm_expect_time.cpp, section 16).  The checked input,
// the per-call preparation, P(t_b) once per device and the tips / up / root / down passes of one chunk of sites.  The schedule of
// the down pass (ex_down_schedule) also serves the many-model entry points (phm_loglik_host.h).
#pragma once

#include "phm_internal.h"
#include "phm_expect.h"

namespace phm_ex {

constexpr double EX_TAIL = 0x1p-60;                    // omitted Poisson mass of a branch's truncated sum
constexpr double EX_MAX_JUMP_MEAN = 1e6;               // max(-q_ii) t_b: the branch stage runs M_b ~ this many steps
constexpr size_t EX_SCRATCH = size_t(256) << 20;       // per-(branch, site) values of one branch-stage launch

// What every device of a call shares, checked and derived once on the host.
struct ExInput {
  int n = 0, T = 0, Nn = 0, E = 0, NT = 0, S = 0, cols = 0;
  bool per_site = false;
  const int32_t* states = nullptr;
  double mu = 0.0;
  phm::Schedule sched;
  std::vector<double> Qr, B, qoff, pid, edge_length;
  std::vector<int32_t> obs, sq, child_row;
  std::vector<phm::UpStep> up;                          // grouped by height
  std::vector<int32_t> up_off;
  std::vector<phm::ExDown> down;                        // grouped by the depth of the parent
  std::vector<int32_t> down_off;
  std::vector<int64_t> w_off;
  std::vector<double> w;
};

// pmf of Poisson(x) at 0 .. M + 1 and M: the first m with sum_{k >= m + 2} pmf(k) <= 2^-60
void poisson_weights(double x, std::vector<double>& p, int& M);
// squarings of expm(Q t) so that the Pade(6) argument has norm <= 1/2
int ex_squarings(const double* Q_rm, int n, double t);
// tree, model, tips, observe and option checks (no device call); fn prefixes the messages.  The caller checks its outputs.
int32_t ex_validate(const std::string& fn, const phm_tree* x, int32_t n, const double* Q, const double* pid, const int32_t* observe,
                    const phm_options& o, ExInput& in);
// level schedules, child rows, Poisson weights and Pade squaring counts (host, once per call)
void ex_prepare(ExInput& in);

// The schedule of the down pass of a tree with T tips: every branch with the rows of its ends and of its sibling, grouped by the
// depth of the parent (down_off: the level boundaries); child_row (when asked for): [edge row] the row of the branch's child.
// Every entry point with a down pass builds it here, the many-model ones (phm_loglik_host.h) included.
inline void ex_down_schedule(const phm::Schedule& s, int T, std::vector<phm::ExDown>& down, std::vector<int32_t>& down_off,
                             std::vector<int32_t>* child_row = nullptr) {
  std::vector<int32_t> order, up_of(s.n_node, -1);
  for (int k = 0; k < s.n_node; ++k) up_of[s.up[k].parent] = k;
  auto row_of = [T](int32_t c) { return c >= 0 ? T + c : ~c; };
  phm::depth_levels(s, order, down_off);
  if (child_row) child_row->assign(s.n_edge, 0);
  for (int32_t k : order) {
    const phm::DownStep& d = s.down[k];
    const phm::UpStep& u = s.up[up_of[d.parent]];
    const int side = u.edge[0] == d.edge ? 1 : 0;                    // the sibling branch
    phm::ExDown x = {};
    x.edge = d.edge; x.parent = T + d.parent; x.child = row_of(d.child);
    x.sib_edge = u.edge[side]; x.sib_child = row_of(u.child[side]);
    down.push_back(x);
    if (child_row) (*child_row)[d.edge] = x.child;
  }
}

// What one device holds for the whole call: the model, the schedules, the branch weights and P(t_b).
struct ExDevice {
  DevBuf dQ, dt, dsq, dP, dB, dq, dpid, dobs, dup, ddown, dchild, dwoff, dw;
};
// uploads and P(t_b) (its launch timed into kernel_ms)
int32_t ex_device_setup(const std::string& fn, const ExInput& in, ExDevice& dev, KernelTimer& tm, double& kernel_ms);

// Sites per chunk: what fits in half the free HBM next to the branch-stage scratch at per_site bytes a site, a multiple of 64,
// capped by phm_debug_options.expect_chunk and by count (rounded up to 64).
int32_t ex_sites_per_chunk(size_t per_site, int64_t count, int64_t& Sc_max);

// The per-site buffers of the passes for chunks of up to Spm sites.
struct ExPasses {
  DevBuf dL, dsL, dO, dsO, dF, dsF, dll, dlam, dtips;
  std::vector<uint8_t> tips_h;
  std::vector<double> ll_h;
  int32_t alloc(const ExInput& in, size_t Spm);
  phm::ExPassParams params(const ExInput& in, const ExDevice& dev, int Sp) const;
};
// bytes per site of ExPasses
size_t ex_pass_bytes(const ExInput& in);

// Tips, up, root and down passes of sites [site0, site0 + Sc) (Sp of them with the padding); node_post (device, or NULL) gets the
// node posteriors inside the same timed region; log p(tips) goes to loglik[site0 ..] when loglik is not NULL.  A site of
// probability 0 fails the call.
int32_t ex_run_passes(const std::string& fn, const ExInput& in, const ExDevice& dev, ExPasses& ps, int64_t site0, int64_t Sc, int Sp,
                      double* node_post, double* loglik, KernelTimer& tm, double& kernel_ms);

}  // namespace phm_ex
