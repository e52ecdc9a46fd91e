// phm_expect_api.cpp -- C-ABI of the exact conditional expectations (phm_expected_stats): validation and
// everything that depends on the branch alone (level schedules, Poisson weights, Pade squaring counts) on the host, then per
// device P(t_b) once, and per chunk of sites the up pass, the down pass and the branch stage (phm_expect.hip).  The host pieces
// declared in phm_expect_host.h, which phm_expected_through_time shares, are defined here (ex_down_schedule, which the many-model
// entry points use too, is inline in that header).
#include "phm_expect_host.h"

namespace phm_ex {

// Computed outward from the mode with pmf(mode) = 1 and normalised by the sum, so x in the thousands keeps full relative precision
// (no lgamma cancellation).
void poisson_weights(double x, std::vector<double>& p, int& M) {
  if (!(x > 0.0)) { p.assign({1.0, 0.0}); M = 0; return; }
  const int64_t mode = (int64_t)std::floor(x), half = (int64_t)std::ceil(12.0 * std::sqrt(x)) + 40;
  const int64_t hi = mode + half, lo = std::max<int64_t>(0, mode - half);
  std::vector<double> r((size_t)hi + 1, 0.0);
  r[mode] = 1.0;
  for (int64_t k = mode; k < hi; ++k) r[k + 1] = r[k] * x / (double)(k + 1);
  for (int64_t k = mode; k > lo; --k) r[k - 1] = r[k] * (double)k / x;
  double sum = 0.0;
  for (int64_t k = hi; k >= lo; --k) sum += r[k];
  std::vector<double> tail((size_t)hi + 2, 0.0);
  for (int64_t k = hi; k >= 0; --k) tail[k] = tail[k + 1] + r[k] / sum;
  int64_t m = 0;
  while (m + 2 <= hi && tail[m + 2] > EX_TAIL) ++m;
  M = (int)m;
  p.resize((size_t)m + 2);
  for (int64_t k = 0; k <= m + 1; ++k) p[k] = r[k] / sum;
}

int32_t ex_validate(const std::string& fn, const phm_tree* x, int32_t n, const double* Q, const double* pid, const int32_t* observe,
                    const phm_options& o, ExInput& in) {
  if (!x || !Q || !pid) return fail(PHM_ERR_BAD_INPUT, fn + "NULL argument (x, Q and pid are required)");
  if (n < 2 || n > phm::EX_MAX_STATES) return fail(PHM_ERR_BAD_INPUT, fn + "n_states must be in 2..64");
  if (o.reduce != 0) return fail(PHM_ERR_BAD_INPUT, fn + "reduce must be 0 (expectations are per site)");
  if (o.n_replicas < 0 || o.n_replicas > (1 << 22)) return fail(PHM_ERR_BAD_INPUT, fn + "n_replicas must be in 0..4194304");
  if (!x->edge || !x->edge_length || !x->states) return fail(PHM_ERR_BAD_INPUT, fn + "x$edge, x$edge.length and x$states are required");
  std::string serr;
  if (!phm::build_schedule(x->n_tips, x->n_node, x->n_edge, x->edge, in.sched, serr)) return fail(PHM_ERR_BAD_INPUT, "tree: " + serr);
  in.n = n; in.T = x->n_tips; in.Nn = x->n_node; in.E = x->n_edge; in.NT = in.T + in.Nn;
  in.S = std::max(1, (int)o.n_replicas);
  in.cols = n + n * (n - 1);
  in.per_site = o.tips_per_replica != 0;
  in.states = x->states;
  int32_t st = check_edge_lengths(x);
  if (st) return st;
  in.edge_length.assign(x->edge_length, x->edge_length + in.E);
  st = check_generator(Q, n, in.Qr);
  if (st) return st;
  in.qoff = in.Qr;
  in.mu = 0.0;
  for (int i = 0; i < n; ++i) {
    in.qoff[(size_t)i * n + i] = 0.0;
    in.mu = std::max(in.mu, -in.Qr[(size_t)i * n + i]);
  }
  if (!(in.mu > 0.0)) return fail(PHM_ERR_BAD_INPUT, "Q: no state is left at a positive rate (max(-q_ii) must be > 0)");
  in.B.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) in.B[(size_t)i * n + j] = (i == j ? 1.0 : 0.0) + in.Qr[(size_t)i * n + j] / in.mu;
  double psum = 0.0;
  st = check_root_prior(pid, n, psum);
  if (st) return st;
  in.pid.resize(n);
  for (int i = 0; i < n; ++i) in.pid[i] = pid[i] / psum;
  st = check_observe(observe, n, in.obs);
  if (st) return st;
  const int64_t n_states_in = (int64_t)(in.per_site ? in.S : 1) * in.T;
  for (int64_t k = 0; k < n_states_in; ++k)
    if (in.states[k] < 0 || in.states[k] > n) return fail(PHM_ERR_BAD_INPUT, "x$states must be in 0..n (0: missing)");
  for (int b = 0; b < in.E; ++b)
    if (in.mu * in.edge_length[b] > EX_MAX_JUMP_MEAN)
      return fail(PHM_ERR_UNSUPPORTED, "edge row " + std::to_string(b + 1) + ": max(-q_ii) * t_b above 1e6");
  return PHM_OK;
}

// phm_expm_pade's own count, pade_squarings, is arma::expmat's, which leaves norms up to ~log2 of the norm and costs 1e-13 .. 1e-12
// in P on fast branches.
int ex_squarings(const double* Q_rm, int n, double t) {
  double norm = 0.0;
  for (int i = 0; i < n; ++i) {
    double r = 0.0;
    for (int j = 0; j < n; ++j) r += std::fabs(Q_rm[(size_t)i * n + j] * t);
    norm = std::max(norm, r);
  }
  int s = 0;
  while (norm > 0.5 && s < 1000) { norm *= 0.5; ++s; }
  return s;
}

void ex_prepare(ExInput& in) {
  const phm::Schedule& s = in.sched;
  std::vector<int32_t> order;
  phm::height_levels(s.up, order, in.up_off);
  for (int32_t k : order) in.up.push_back(s.up[k]);
  ex_down_schedule(s, in.T, in.down, in.down_off, &in.child_row);
  in.w_off.assign(1, 0);
  in.sq.resize(in.E);
  std::vector<double> p;
  for (int b = 0; b < in.E; ++b) {
    int M = 0;
    poisson_weights(in.mu * in.edge_length[b], p, M);
    for (int m = 0; m <= M; ++m) in.w.push_back(p[m + 1] / in.mu);     // w_m = pois(m + 1; mu t_b) / mu
    in.w_off.push_back((int64_t)in.w.size());
    in.sq[b] = ex_squarings(in.Qr.data(), in.n, in.edge_length[b]);
  }
}

int32_t ex_device_setup(const std::string& fn, const ExInput& in, ExDevice& d, KernelTimer& tm, double& kernel_ms) {
  const size_t nn = (size_t)in.n * in.n;
  const int E = in.E;
  DevBuf dwork, derr;
  HIPCHK(upload(d.dQ, in.Qr)); HIPCHK(upload(d.dt, in.edge_length)); HIPCHK(upload(d.dsq, in.sq));
  HIPCHK(dwork.alloc(sizeof(double) * nn * 5 * E)); HIPCHK(d.dP.alloc(sizeof(double) * nn * E));
  HIPCHK(derr.alloc(sizeof(uint32_t))); HIPCHK(hipMemset(derr.p, 0, sizeof(uint32_t)));
  HIPCHK(upload(d.dB, in.B)); HIPCHK(upload(d.dq, in.qoff)); HIPCHK(upload(d.dpid, in.pid)); HIPCHK(upload(d.dobs, in.obs));
  HIPCHK(upload(d.dup, in.up)); HIPCHK(upload(d.ddown, in.down)); HIPCHK(upload(d.dchild, in.child_row));
  HIPCHK(upload(d.dwoff, in.w_off)); HIPCHK(upload(d.dw, in.w));
  HIPCHK(tm.start());
  HIPCHK(phm::launch_expm_pade(in.n, d.dQ.as<double>(), d.dt.as<double>(), d.dsq.as<int32_t>(), E, dwork.as<double>(), d.dP.as<double>(),
                               derr.as<uint32_t>(), nullptr));
  HIPCHK(tm.stop());
  uint32_t derrh = 0;
  HIPCHK(hipMemcpy(&derrh, derr.p, sizeof derrh, hipMemcpyDeviceToHost));
  if (derrh) return fail(PHM_ERR_BAD_INPUT, fn + "singular Pade denominator in expm(Q t_b)");
  HIPCHK(tm.add_to(kernel_ms));
  return PHM_OK;
}

int32_t ex_sites_per_chunk(size_t per_site, int64_t count, int64_t& Sc_max) {
  const int chunk = g_phm_debug.expect_chunk;
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const size_t budget = free_b / 2 > EX_SCRATCH ? free_b / 2 - EX_SCRATCH : 0;
  Sc_max = std::max<int64_t>(64, (int64_t)(budget / per_site) / 64 * 64);
  if (chunk > 0) Sc_max = std::min<int64_t>(Sc_max, ((int64_t)chunk + 63) / 64 * 64);
  Sc_max = std::min<int64_t>(Sc_max, (count + 63) / 64 * 64);
  return PHM_OK;
}

size_t ex_pass_bytes(const ExInput& in) {
  return sizeof(double) * ((size_t)in.NT * (2 * in.n + 2) + (size_t)in.E * (in.n + 1) + 2) + in.T;
}

int32_t ExPasses::alloc(const ExInput& in, size_t Spm) {
  const size_t n = in.n, NT = in.NT, E = in.E;
  HIPCHK(dL.alloc(sizeof(double) * NT * n * Spm)); HIPCHK(dsL.alloc(sizeof(double) * NT * Spm));
  HIPCHK(dO.alloc(sizeof(double) * NT * n * Spm)); HIPCHK(dsO.alloc(sizeof(double) * NT * Spm));
  HIPCHK(dF.alloc(sizeof(double) * E * n * Spm)); HIPCHK(dsF.alloc(sizeof(double) * E * Spm));
  HIPCHK(dll.alloc(sizeof(double) * Spm)); HIPCHK(dlam.alloc(sizeof(double) * Spm)); HIPCHK(dtips.alloc((size_t)in.T * Spm));
  tips_h.assign((size_t)in.T * Spm, 0);
  ll_h.assign(Spm, 0.0);
  return PHM_OK;
}

phm::ExPassParams ExPasses::params(const ExInput& in, const ExDevice& dev, int Sp) const {
  phm::ExPassParams pp;
  pp.n = in.n; pp.n_tips = in.T; pp.Sp = Sp;
  pp.P = dev.dP.as<double>(); pp.L = dL.as<double>(); pp.sL = dsL.as<double>(); pp.O = dO.as<double>(); pp.sO = dsO.as<double>();
  pp.F = dF.as<double>(); pp.sF = dsF.as<double>(); pp.ll = dll.as<double>(); pp.lam = dlam.as<double>();
  return pp;
}

int32_t ex_run_passes(const std::string& fn, const ExInput& in, const ExDevice& dev, ExPasses& ps, int64_t site0, int64_t Sc, int Sp,
                      double* node_post, double* loglik, KernelTimer& tm, double& kernel_ms) {
  const int T = in.T;
  std::fill(ps.tips_h.begin(), ps.tips_h.end(), (uint8_t)0);     // padding sites: every tip missing
  for (int64_t k = 0; k < Sc; ++k) {
    const int32_t* y = in.states + (in.per_site ? (site0 + k) * T : 0);
    for (int t = 0; t < T; ++t) ps.tips_h[(size_t)t * Sp + k] = (uint8_t)y[t];
  }
  HIPCHK(hipMemcpy(ps.dtips.p, ps.tips_h.data(), (size_t)T * Sp, hipMemcpyHostToDevice));
  const phm::ExPassParams pp = ps.params(in, dev, Sp);
  HIPCHK(tm.start());
  HIPCHK(phm::launch_ex_tips(pp, ps.dtips.as<uint8_t>(), dev.dobs.as<int32_t>(), nullptr));
  for (size_t l = 0; l + 1 < in.up_off.size(); ++l)
    HIPCHK(phm::launch_ex_up(pp, dev.dup.as<phm::UpStep>() + in.up_off[l], in.up_off[l + 1] - in.up_off[l], nullptr));
  HIPCHK(phm::launch_ex_root(pp, T + in.sched.root, dev.dpid.as<double>(), nullptr));
  for (size_t l = 0; l + 1 < in.down_off.size(); ++l)
    HIPCHK(phm::launch_ex_down(pp, dev.ddown.as<phm::ExDown>() + in.down_off[l], in.down_off[l + 1] - in.down_off[l], nullptr));
  if (node_post) HIPCHK(phm::launch_ex_post(pp, in.NT, node_post, nullptr));
  HIPCHK(tm.stop());
  HIPCHK(hipMemcpy(ps.ll_h.data(), ps.dll.p, sizeof(double) * Sc, hipMemcpyDeviceToHost));
  for (int64_t k = 0; k < Sc; ++k)
    if (!std::isfinite(ps.ll_h[k]))
      return fail(PHM_ERR_ZERO_PROB, fn + "site " + std::to_string(site0 + k + 1) + " has probability 0 under Q (its tips are impossible)");
  if (loglik) std::memcpy(loglik + site0, ps.ll_h.data(), sizeof(double) * Sc);
  HIPCHK(tm.add_to(kernel_ms));
  return PHM_OK;
}

}  // namespace phm_ex

namespace {

using namespace phm_ex;

const std::string EX_FN = "phm_expected_stats: ";

// Sites [first, first + count) of the call on one device; outputs point at the caller's full arrays (S sites per column).
int32_t ex_one_device(const ExInput& in, int32_t device, int64_t first, int64_t count, double* stats, double* loglik,
                      double* branch_stats, double* node_post) {
  int32_t st = select_device(device);
  if (st) return st;
  const int n = in.n, E = in.E, NT = in.NT, cols = in.cols;
  const size_t S = (size_t)in.S;
  ExDevice dev;
  KernelTimer tm;
  double kernel_ms = 0.0;
  st = ex_device_setup(EX_FN, in, dev, tm, kernel_ms);
  if (st) return st;

  int64_t Sc_max = 0;
  st = ex_sites_per_chunk(ex_pass_bytes(in) + sizeof(double) * (cols + (node_post ? (size_t)NT * n : 0)), count, Sc_max);
  if (st) return st;
  const size_t Spm = (size_t)Sc_max;
  ExPasses ps;
  st = ps.alloc(in, Spm);
  if (st) return st;
  DevBuf dtot, dpost, dout;
  HIPCHK(dtot.alloc(sizeof(double) * cols * Spm));
  if (node_post) HIPCHK(dpost.alloc(sizeof(double) * NT * n * Spm));
  const int chunk = g_phm_debug.expect_chunk;
  int ne_max = (int)std::max<size_t>(1, std::min<size_t>({(size_t)E, (size_t)65535, EX_SCRATCH / (sizeof(double) * cols * Spm)}));
  if (chunk > 0) ne_max = std::min(ne_max, chunk);
  HIPCHK(dout.alloc(sizeof(double) * cols * (size_t)ne_max * Spm));

  for (int64_t c0 = 0; c0 < count; c0 += Sc_max) {
    const int64_t Sc = std::min<int64_t>(Sc_max, count - c0);
    const int Sp = (int)((Sc + 63) / 64 * 64);
    const int64_t site0 = first + c0;                              // global id of this chunk's first site
    st = ex_run_passes(EX_FN, in, dev, ps, site0, Sc, Sp, node_post ? dpost.as<double>() : nullptr, loglik, tm, kernel_ms);
    if (st) return st;
    if (node_post)                                                 // [state][row][Sp] -> site + S (row + NT state)
      HIPCHK(hipMemcpy2D(node_post + site0, sizeof(double) * S, dpost.p, sizeof(double) * Sp, sizeof(double) * Sc, (size_t)NT * n,
                         hipMemcpyDeviceToHost));

    phm::ExBranchParams bp;
    bp.n = n; bp.Sp = Sp; bp.mu = in.mu; bp.B = dev.dB.as<double>(); bp.qoff = dev.dq.as<double>(); bp.w_off = dev.dwoff.as<int64_t>();
    bp.w = dev.dw.as<double>(); bp.child = dev.dchild.as<int32_t>(); bp.L = ps.dL.as<double>(); bp.sL = ps.dsL.as<double>();
    bp.F = ps.dF.as<double>(); bp.sF = ps.dsF.as<double>(); bp.lam = ps.dlam.as<double>();
    bp.root = in.T + in.sched.root;
    bp.out = dout.as<double>();
    HIPCHK(hipMemset(dtot.p, 0, sizeof(double) * cols * Sp));
    for (int e0 = 0; e0 < E; e0 += ne_max) {
      const int ne = std::min(ne_max, E - e0);
      bp.e0 = e0; bp.n_out_edges = ne;
      HIPCHK(tm.start());
      HIPCHK(phm::launch_ex_branch(bp, ne, nullptr));
      HIPCHK(phm::launch_ex_reduce(dout.as<double>(), cols, ne, Sp, dtot.as<double>(), nullptr));
      HIPCHK(tm.stop());
      if (branch_stats)                                            // [col][e][Sp] -> site + S (edge + E col)
        for (int col = 0; col < cols; ++col)
          HIPCHK(hipMemcpy2D(branch_stats + site0 + S * ((size_t)e0 + (size_t)E * col), sizeof(double) * S,
                             dout.as<double>() + (size_t)col * ne * Sp, sizeof(double) * Sp, sizeof(double) * Sc, ne,
                             hipMemcpyDeviceToHost));
      HIPCHK(tm.add_to(kernel_ms));
    }
    HIPCHK(hipMemcpy2D(stats + site0, sizeof(double) * S, dtot.p, sizeof(double) * Sp, sizeof(double) * Sc, cols,
                       hipMemcpyDeviceToHost));
  }
  g_phm_last_kernel_ms = kernel_ms;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Sites are independent: with phm_options.n_devices > 1 device d computes a contiguous range of them (phm_plan_shards,
// run_shards); every output row is the one-device row bit for bit.
int32_t phm_expected_stats(const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const int32_t* observe,
                           const phm_options* opt, double* stats, double* loglik, double* branch_stats, double* node_post) {
  const phm_options o = resolve_options(opt);
  if (!x || !Q || !pid || !stats || !loglik) return fail(PHM_ERR_BAD_INPUT, EX_FN + "NULL argument (only observe, branch_stats and node_post may be NULL)");
  ExInput in;
  int32_t st = ex_validate(EX_FN, x, n_states, Q, pid, observe, o, in);
  if (st) return st;
  ex_prepare(in);
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, in.S, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) {
    return ex_one_device(in, sh.device, sh.first, sh.count, stats, loglik, branch_stats, node_post);
  });
}

}  // extern "C"
