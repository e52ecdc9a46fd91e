// phm_expect_time.cpp -- C-ABI of the exact expectations through time (phm_expected_through_time).  On the
// host: section 13's checks and preparation (phm_expect_host.h), the bounds and points, the node depths, the crossings of every
// boundary and the sub-branches of every bin with their Poisson weights.  Per device: P(t_b), and per chunk of sites section 13's
// passes, then per chunk of items P(s) and P(t_b - s) and the along-branch vectors (phm_expect.hip), the sub-branch integrals
// through the unchanged branch stage, and the fixed-order sums per boundary and per bin.
#include "phm_expect_host.h"

namespace {

using namespace phm_ex;

const std::string TT_FN = "phm_expected_through_time: ";

// Points on branches: the edge row and the times of the two P matrices, s1 from the parent end and t_b - s2 (s1 = s2 = s for a
// point; the ends of a sub-branch otherwise), with their Pade squaring counts.
struct TtItems {
  std::vector<int32_t> edge;
  std::vector<double> t;                       // [2 items]
  std::vector<int32_t> sq;
  int64_t size() const { return (int64_t)edge.size(); }
  void add(const ExInput& in, int32_t b, double s1, double s2) {
    const double t1 = s1, t2 = in.edge_length[b] - s2;
    edge.push_back(b);
    t.push_back(t1); t.push_back(t2);
    sq.push_back(ex_squarings(in.Qr.data(), in.n, t1)); sq.push_back(ex_squarings(in.Qr.data(), in.n, t2));
  }
};

// Planned once per call on the host, shared by every device.
struct TtPlan {
  int K = 0;                                   // boundaries
  TtItems pts;                                 // the boundaries' crossings (by boundary, then edge row), then the caller's points
  int64_t n_cross = 0;
  std::vector<int64_t> cross_off;              // [K + 1]: boundary k's crossings in pts
  TtItems sub;                                 // sub-branches by (bin, edge row)
  std::vector<int64_t> bin_off;                // [K]: bin k's sub-branches
  std::vector<int64_t> w_off;                  // [sub + 1] into w
  std::vector<double> w;                       // pois(m + 1; mu h) / mu, as section 13's w per branch
};

int32_t tt_plan(const ExInput& in, int32_t K, const double* bounds, bool occ, bool bins, int64_t P, const int32_t* pe,
                const double* pp, bool points, TtPlan& pl) {
  for (int k = 0; k < K; ++k) {
    const double tau = bounds[k];
    if (!std::isfinite(tau) || tau < 0.0)
      return fail(PHM_ERR_BAD_INPUT, TT_FN + "bounds[" + std::to_string(k) + "] must be finite and >= 0");
    if (k > 0 && !(tau > bounds[k - 1]))
      return fail(PHM_ERR_BAD_INPUT, TT_FN + "bounds[" + std::to_string(k) + "] is not above bounds[" + std::to_string(k - 1) +
                                         "] (bounds must increase strictly)");
  }
  for (int64_t i = 0; i < P; ++i) {
    const int32_t b = pe[i];
    if (b < 0 || b >= in.E)
      return fail(PHM_ERR_BAD_INPUT, TT_FN + "point " + std::to_string(i) + ": edge row " + std::to_string(b) + " is not in 0..n_edge-1");
    if (!(pp[i] >= 0.0 && pp[i] <= in.edge_length[b]))
      return fail(PHM_ERR_BAD_INPUT, TT_FN + "point " + std::to_string(i) + ": position " + std::to_string(pp[i]) +
                                         " is not in [0, t_b] of edge row " + std::to_string(b));
  }
  // depths in down-pass order: d(root) = 0, d(c) = d(p) + t_b
  const int root = in.T + in.sched.root;
  std::vector<double> d(in.NT, 0.0);
  std::vector<int32_t> par(in.E, 0);
  for (const phm::ExDown& x : in.down) {
    d[x.child] = d[x.parent] + in.edge_length[x.edge];
    par[x.edge] = x.parent;
  }
  int32_t root_edge = 0;                       // tau = 0 counts the root through the start of its lowest branch row
  while (par[root_edge] != root) ++root_edge;
  pl.K = K;
  if (occ) {
    pl.cross_off.assign(1, 0);
    for (int k = 0; k < K; ++k) {
      const double tau = bounds[k];
      if (tau == 0.0) pl.pts.add(in, root_edge, 0.0, 0.0);
      for (int b = 0; b < in.E; ++b) {
        const double dp = d[par[b]], dc = d[in.child_row[b]], tb = in.edge_length[b];
        if (dp < tau && tau <= dc) {
          const double s = tau >= dc ? tb : std::min(tau - dp, tb);
          pl.pts.add(in, b, s, s);
        }
      }
      pl.cross_off.push_back(pl.pts.size());
    }
  }
  pl.n_cross = pl.pts.size();
  if (points)
    for (int64_t i = 0; i < P; ++i) pl.pts.add(in, pe[i], pp[i], pp[i]);
  if (bins) {
    pl.bin_off.assign(1, 0);
    pl.w_off.assign(1, 0);
    std::vector<double> p;
    for (int k = 0; k + 1 < K; ++k) {
      const double lo = bounds[k], hi = bounds[k + 1];
      for (int b = 0; b < in.E; ++b) {
        const double dp = d[par[b]], dc = d[in.child_row[b]], tb = in.edge_length[b];
        if (!(dp < hi && dc > lo)) continue;
        const double s1 = lo <= dp ? 0.0 : std::min(lo - dp, tb), s2 = hi >= dc ? tb : std::min(hi - dp, tb);
        if (!(s2 > s1)) continue;
        pl.sub.add(in, b, s1, s2);
        int M = 0;
        poisson_weights(in.mu * (s2 - s1), p, M);
        for (int m = 0; m <= M; ++m) pl.w.push_back(p[m + 1] / in.mu);
        pl.w_off.push_back((int64_t)pl.w.size());
      }
      pl.bin_off.push_back(pl.sub.size());
    }
  }
  return PHM_OK;
}

// items per launch: per_item_site bytes a site plus P(s), P(t_b - s) and their Pade work (12 n^2 doubles) within the scratch
int tt_items_per_chunk(size_t per_item_site, size_t Spm, int n) {
  const size_t per_item = per_item_site * Spm + sizeof(double) * 12 * (size_t)n * n;
  int cap = (int)std::max<size_t>(1, std::min<size_t>(65535, EX_SCRATCH / per_item));
  if (g_phm_debug.expect_chunk > 0) cap = std::min(cap, (int)g_phm_debug.expect_chunk);
  return cap;
}

// the ranges [r_begin, r_end) of off (range r: items off[r] .. off[r + 1] - 1) that can meet items [q0, q1)
void tt_ranges(const std::vector<int64_t>& off, int64_t q0, int64_t q1, int& r_begin, int& r_end) {
  r_begin = std::max(0, (int)(std::upper_bound(off.begin(), off.end(), q0) - off.begin()) - 1);
  r_end = std::min((int)off.size() - 1, (int)(std::lower_bound(off.begin(), off.end(), q1) - off.begin()));
}

// Sites [first, first + count) of the call on one device; outputs point at the caller's full arrays (S sites per column).
int32_t tt_one_device(const ExInput& in, const TtPlan& pl, int32_t device, int64_t first, int64_t count, double* occupancy,
                      double* bin_stats, int64_t n_points, double* point_post, double* loglik) {
  int32_t st = select_device(device);
  if (st) return st;
  const int n = in.n, cols = in.cols, K = pl.K, NB = std::max(0, pl.K - 1);
  const size_t nn = (size_t)n * n, S = (size_t)in.S;
  ExDevice dev;
  KernelTimer tm;
  double kernel_ms = 0.0, t_along = 0.0, t_branch = 0.0, t_reduce = 0.0;
  st = ex_device_setup(TT_FN, in, dev, tm, kernel_ms);
  if (st) return st;
  int64_t Sc_max = 0;
  st = ex_sites_per_chunk(ex_pass_bytes(in) + sizeof(double) * ((occupancy ? (size_t)n * K : 0) + (bin_stats ? (size_t)cols * NB : 0)),
                          count, Sc_max);
  if (st) return st;
  const size_t Spm = (size_t)Sc_max;
  ExPasses ps;
  st = ps.alloc(in, Spm);
  if (st) return st;
  const int64_t NP = pl.pts.size(), NS = pl.sub.size();
  const int np_max = NP ? tt_items_per_chunk(sizeof(double) * n, Spm, n) : 0;
  const int ns_max = NS ? tt_items_per_chunk(sizeof(double) * (2 * n + 2 + cols), Spm, n) : 0;
  const size_t nm_max = (size_t)std::max(np_max, ns_max);                // items of one P launch
  DevBuf dpe, dpt, dpsq, dse, dst, dssq, dswoff, dsw, dcoff, dboff, dident, dwork, dPi, derr, dpost, docc, da, dsa, dbe, dsbe, dout, dtot;
  HIPCHK(upload(dpe, pl.pts.edge)); HIPCHK(upload(dpt, pl.pts.t)); HIPCHK(upload(dpsq, pl.pts.sq));
  HIPCHK(upload(dse, pl.sub.edge)); HIPCHK(upload(dst, pl.sub.t)); HIPCHK(upload(dssq, pl.sub.sq));
  HIPCHK(upload(dswoff, pl.w_off)); HIPCHK(upload(dsw, pl.w)); HIPCHK(upload(dcoff, pl.cross_off)); HIPCHK(upload(dboff, pl.bin_off));
  std::vector<int32_t> ident((size_t)ns_max);                             // sub-branch k's backward vector is row k
  for (int k = 0; k < ns_max; ++k) ident[k] = k;
  HIPCHK(upload(dident, ident));
  HIPCHK(dwork.alloc(sizeof(double) * 5 * nn * 2 * nm_max)); HIPCHK(dPi.alloc(sizeof(double) * nn * 2 * nm_max));
  HIPCHK(derr.alloc(sizeof(uint32_t))); HIPCHK(hipMemset(derr.p, 0, sizeof(uint32_t)));
  HIPCHK(dpost.alloc(sizeof(double) * n * (size_t)np_max * Spm));
  if (occupancy) HIPCHK(docc.alloc(sizeof(double) * n * (size_t)K * Spm));
  HIPCHK(da.alloc(sizeof(double) * (size_t)ns_max * n * Spm)); HIPCHK(dsa.alloc(sizeof(double) * (size_t)ns_max * Spm));
  HIPCHK(dbe.alloc(sizeof(double) * (size_t)ns_max * n * Spm)); HIPCHK(dsbe.alloc(sizeof(double) * (size_t)(ns_max + 1) * Spm));
  HIPCHK(dout.alloc(sizeof(double) * cols * (size_t)ns_max * Spm));
  if (bin_stats) HIPCHK(dtot.alloc(sizeof(double) * cols * (size_t)NB * Spm));

  for (int64_t c0 = 0; c0 < count; c0 += Sc_max) {
    const int64_t Sc = std::min<int64_t>(Sc_max, count - c0);
    const int Sp = (int)((Sc + 63) / 64 * 64);
    const int64_t site0 = first + c0;                              // global id of this chunk's first site
    st = ex_run_passes(TT_FN, in, dev, ps, site0, Sc, Sp, nullptr, loglik, tm, kernel_ms);
    if (st) return st;
    const phm::ExPassParams pp = ps.params(in, dev, Sp);
    phm::ExAlongParams ap = {};
    ap.n = n; ap.Sp = Sp; ap.P = dPi.as<double>(); ap.child = dev.dchild.as<int32_t>();
    ap.F = pp.F; ap.sF = pp.sF; ap.L = pp.L; ap.sL = pp.sL;

    // posteriors at the crossings (summed per boundary) and at the caller's points
    if (occupancy) HIPCHK(hipMemset(docc.p, 0, sizeof(double) * n * (size_t)K * Sp));
    ap.post = dpost.as<double>();
    for (int64_t q0 = 0; q0 < NP; q0 += np_max) {
      const int nq = (int)std::min<int64_t>(np_max, NP - q0);
      ap.edge = dpe.as<int32_t>() + q0; ap.rows = nq;
      HIPCHK(tm.start());
      HIPCHK(phm::launch_expm_pade(n, dev.dQ.as<double>(), dpt.as<double>() + 2 * q0, dpsq.as<int32_t>() + 2 * q0, 2 * nq,
                                   dwork.as<double>(), dPi.as<double>(), derr.as<uint32_t>(), nullptr));
      HIPCHK(phm::launch_ex_along(ap, nq, nullptr));
      HIPCHK(tm.stop());
      HIPCHK(tm.add_to(t_along));
      if (occupancy && q0 < pl.n_cross) {
        int r0 = 0, r1 = 0;
        tt_ranges(pl.cross_off, q0, q0 + nq, r0, r1);
        HIPCHK(tm.start());
        HIPCHK(phm::launch_ex_range_sum(dpost.as<double>(), n, nq, q0, dcoff.as<int64_t>(), r0, r1, K, Sp, docc.as<double>(), nullptr));
        HIPCHK(tm.stop());
        HIPCHK(tm.add_to(t_reduce));
      }
      if (point_post && q0 + nq > pl.n_cross) {                  // [state][q - q0][Sp] -> site + S (point + n_points state)
        const int64_t a0 = std::max(q0, pl.n_cross);
        for (int i = 0; i < n; ++i)
          HIPCHK(hipMemcpy2D(point_post + site0 + S * ((size_t)(a0 - pl.n_cross) + (size_t)n_points * i), sizeof(double) * S,
                             dpost.as<double>() + ((size_t)i * nq + (size_t)(a0 - q0)) * Sp, sizeof(double) * Sp, sizeof(double) * Sc,
                             (size_t)(q0 + nq - a0), hipMemcpyDeviceToHost));
      }
    }
    if (occupancy)                                                 // [state][bound][Sp] -> site + S (bound + K state)
      HIPCHK(hipMemcpy2D(occupancy + site0, sizeof(double) * S, docc.p, sizeof(double) * Sp, sizeof(double) * Sc, (size_t)n * K,
                         hipMemcpyDeviceToHost));

    // sub-branch integrals: section 13's branch stage on arrays indexed by sub-branch; the backward rows carry one more row, the
    // root's exponent, which the stage's factor reads
    if (bin_stats) {
      HIPCHK(hipMemset(dtot.p, 0, sizeof(double) * cols * (size_t)NB * Sp));
      ap.post = nullptr; ap.a = da.as<double>(); ap.sa = dsa.as<double>(); ap.beta = dbe.as<double>(); ap.sbeta = dsbe.as<double>();
      phm::ExBranchParams bp;
      bp.n = n; bp.Sp = Sp; bp.e0 = 0; bp.mu = in.mu; bp.B = dev.dB.as<double>(); bp.qoff = dev.dq.as<double>();
      bp.w = dsw.as<double>(); bp.child = dident.as<int32_t>(); bp.L = dbe.as<double>(); bp.sL = dsbe.as<double>();
      bp.F = da.as<double>(); bp.sF = dsa.as<double>(); bp.lam = pp.lam; bp.out = dout.as<double>();
      for (int64_t k0 = 0; k0 < NS; k0 += ns_max) {
        const int nk = (int)std::min<int64_t>(ns_max, NS - k0);
        ap.edge = dse.as<int32_t>() + k0;
        HIPCHK(tm.start());
        HIPCHK(phm::launch_expm_pade(n, dev.dQ.as<double>(), dst.as<double>() + 2 * k0, dssq.as<int32_t>() + 2 * k0, 2 * nk,
                                     dwork.as<double>(), dPi.as<double>(), derr.as<uint32_t>(), nullptr));
        HIPCHK(phm::launch_ex_along(ap, nk, nullptr));
        HIPCHK(hipMemcpyAsync(dsbe.as<double>() + (size_t)nk * Sp, pp.sL + (size_t)(in.T + in.sched.root) * Sp, sizeof(double) * Sp,
                              hipMemcpyDeviceToDevice, nullptr));
        HIPCHK(tm.stop());
        HIPCHK(tm.add_to(t_along));
        bp.w_off = dswoff.as<int64_t>() + k0; bp.root = nk; bp.n_out_edges = nk;
        HIPCHK(tm.start());
        HIPCHK(phm::launch_ex_branch(bp, nk, nullptr));
        HIPCHK(tm.stop());
        HIPCHK(tm.add_to(t_branch));
        int r0 = 0, r1 = 0;
        tt_ranges(pl.bin_off, k0, k0 + nk, r0, r1);
        HIPCHK(tm.start());
        HIPCHK(phm::launch_ex_range_sum(dout.as<double>(), cols, nk, k0, dboff.as<int64_t>(), r0, r1, NB, Sp, dtot.as<double>(), nullptr));
        HIPCHK(tm.stop());
        HIPCHK(tm.add_to(t_reduce));
      }
      HIPCHK(hipMemcpy2D(bin_stats + site0, sizeof(double) * S, dtot.p, sizeof(double) * Sp, sizeof(double) * Sc, (size_t)cols * NB,
                         hipMemcpyDeviceToHost));
    }
    uint32_t derrh = 0;
    HIPCHK(hipMemcpy(&derrh, derr.p, sizeof derrh, hipMemcpyDeviceToHost));
    if (derrh) return fail(PHM_ERR_BAD_INPUT, TT_FN + "singular Pade denominator in expm(Q s)");
  }
  if (g_phm_debug.phase_timing)
    std::fprintf(stderr, "phm_expected_through_time: passes %.3f ms, along-branch vectors %.3f ms, branch stage %.3f ms, reductions %.3f ms\n",
                 kernel_ms, t_along, t_branch, t_reduce);
  g_phm_last_kernel_ms = kernel_ms + t_along + t_branch + t_reduce;
  return PHM_OK;
}

}  // namespace

extern "C" {

// Sites are independent: with phm_options.n_devices > 1 device d computes a contiguous range of them (phm_plan_shards,
// run_shards); every output row is the one-device row bit for bit.
int32_t phm_expected_through_time(const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const int32_t* observe,
                                  const phm_options* opt, int32_t n_bounds, const double* bounds, double* occupancy, double* bin_stats,
                                  int64_t n_points, const int32_t* point_edge, const double* point_pos, double* point_post,
                                  double* loglik) {
  const phm_options o = resolve_options(opt);
  if (!occupancy && !bin_stats && !point_post && !loglik)
    return fail(PHM_ERR_BAD_INPUT, TT_FN + "no output requested (occupancy, bin_stats, point_post and loglik are all NULL)");
  ExInput in;
  int32_t st = ex_validate(TT_FN, x, n_states, Q, pid, observe, o, in);
  if (st) return st;
  if (n_bounds < 0 || (n_bounds > 0 && !bounds)) return fail(PHM_ERR_BAD_INPUT, TT_FN + "bounds must hold n_bounds >= 0 values");
  if (occupancy && n_bounds < 1) return fail(PHM_ERR_BAD_INPUT, TT_FN + "occupancy needs n_bounds >= 1");
  if (bin_stats && n_bounds < 2) return fail(PHM_ERR_BAD_INPUT, TT_FN + "bin_stats needs n_bounds >= 2");
  if (n_points < 0 || (n_points > 0 && (!point_edge || !point_pos)))
    return fail(PHM_ERR_BAD_INPUT, TT_FN + "point_edge and point_pos must hold n_points >= 0 values");
  if (point_post && n_points < 1) return fail(PHM_ERR_BAD_INPUT, TT_FN + "point_post needs n_points >= 1");
  ex_prepare(in);
  TtPlan pl;
  st = tt_plan(in, n_bounds, bounds, occupancy != nullptr, bin_stats != nullptr, n_points, point_edge, point_pos, point_post != nullptr, pl);
  if (st) return st;
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, in.S, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) {
    return tt_one_device(in, pl, sh.device, sh.first, sh.count, occupancy, bin_stats, n_points, point_post, loglik);
  });
}

}  // extern "C"
