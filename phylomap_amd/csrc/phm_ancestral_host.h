// phm_ancestral_host.h -- what the two ancestral entry points share on the host: phm_ancestral_models (phm_ancestral_api.cpp,
// 2..8 states) and phm_ancestral_models_wide (phm_ancestral_wide_api.cpp, 9..64 states, section 23).  The
// input with the node selection and the schedule of the down pass, and the one body of both extern "C" functions.
#pragma once

#include "phm_loglik_host.h"

namespace phm_ll {

struct AnInput {
  LlInput ll;
  int J = 0;                                            // reported nodes
  std::vector<int32_t> sel;                             // their node rows (node id - 1), in the caller's order
  std::vector<phm::ExDown> down;                        // grouped by the depth of the parent
  std::vector<int32_t> down_off;
};
// models [first, first + count) on one device
using AnDevice = int32_t (*)(const AnInput& an, int32_t device, int64_t first, int64_t count, double* loglik, double* node_post,
                             int32_t* joint_states, double* joint_logp);
// The body of both: the argument checks, ll_validate, the refusal of a state count outside n_lo .. n_hi (fn + range_msg), the node
// selection, the schedule of the down pass, and run over the shards of models.
inline int32_t an_entry(const std::string& fn, int n_lo, int n_hi, const char* range_msg, AnDevice run, const phm_tree* x,
                        int32_t n_states, int32_t n_models, const double* Q, const double* pid, int32_t n_pid, const int32_t* observe,
                        const int32_t* site_of_model, const int32_t* node_sel, int32_t n_sel, const phm_options* opt, double* loglik,
                        double* node_post, int32_t* joint_states, double* joint_logp) {
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid || !loglik) return fail(PHM_ERR_BAD_INPUT, fn + "NULL argument (x, Q, pid and loglik are required)");
  if (!node_post && !joint_states) return fail(PHM_ERR_BAD_INPUT, fn + "node_post and joint_states are both NULL: nothing to compute");
  if (joint_logp && !joint_states) return fail(PHM_ERR_BAD_INPUT, fn + "joint_logp needs joint_states");
  if (n_sel < 0) return fail(PHM_ERR_BAD_INPUT, fn + "n_sel must be >= 0");
  if (n_sel > 0 && !node_sel) return fail(PHM_ERR_BAD_INPUT, fn + "node_sel is NULL with n_sel > 0");
  AnInput an;
  LlInput& in = an.ll;
  int32_t st = ll_validate(fn, x, n_states, n_models, Q, pid, n_pid, observe, site_of_model, o, in);
  if (st) return st;
  if (in.n < n_lo || in.n > n_hi) return fail(PHM_ERR_UNSUPPORTED, fn + range_msg);
  if ((int64_t)in.S * in.K > (int64_t)INT32_MAX) return fail(PHM_ERR_BAD_INPUT, fn + "sites * models must fit in 31 bits");
  if (n_sel == 0) {
    an.sel.resize(in.NT);
    for (int r = 0; r < in.NT; ++r) an.sel[r] = r;
  } else {
    an.sel.resize(n_sel);
    for (int j = 0; j < n_sel; ++j) {
      if (node_sel[j] < 1 || node_sel[j] > in.NT)
        return fail(PHM_ERR_BAD_INPUT, fn + "node_sel[" + std::to_string(j) + "] must be in 1.." + std::to_string(in.NT));
      an.sel[j] = node_sel[j] - 1;
    }
  }
  an.J = (int)an.sel.size();
  phm_ex::ex_down_schedule(in.sched, in.T, an.down, an.down_off);
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, in.K, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) {
    return run(an, sh.device, sh.first, sh.count, loglik, node_post, joint_states, joint_logp);
  });
}

}  // namespace phm_ll
