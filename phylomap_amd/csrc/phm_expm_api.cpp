// phm_expm_api.cpp -- C-ABI of the matrix-exponentiation path: batched transition matrices (eigen route, Pade route, their
// MFMA f64 variants) and the sumstatEXP driver (maketreelistEXP, src/phylomap.cpp:3001-3051).
#include "phm_internal.h"
#include "phm_maps_host.h"

extern "C" {

static int32_t expm_eigen_impl(bool mfma, int32_t n, const double* lefts, const double* rights, const double* d, const double* t,
                               int32_t n_t, int32_t device, double* out, double* kernel_ms) {
  if (n < 1 || n > 256 || !lefts || !rights || !d || !t || !out || n_t < 0) return fail(PHM_ERR_BAD_INPUT, "phm_expm_eigen: bad arguments");
  int32_t st = select_device(device);
  if (st) return st;
  if (n_t == 0) return PHM_OK;
  std::vector<double> L, R, dv(n);
  cm_to_rm(lefts, n, L); cm_to_rm(rights, n, R);
  for (int i = 0; i < n; ++i) dv[i] = d[i + (size_t)i * n];
  const size_t nn = (size_t)n * n;
  DevBuf dL, dR, dd, dt, dout;
  HIPCHK(upload(dL, L)); HIPCHK(upload(dR, R)); HIPCHK(upload(dd, dv)); HIPCHK(upload(dt, t, n_t));
  HIPCHK(dout.alloc(sizeof(double) * nn * n_t));
  KernelTimer tm;
  HIPCHK(tm.start());
  if (mfma) HIPCHK(phm::launch_expm_eigen_mfma(n, dL.as<double>(), dR.as<double>(), dd.as<double>(), dt.as<double>(), n_t, dout.as<double>(), nullptr));
  else HIPCHK(phm::launch_expm_eigen(n, dL.as<double>(), dR.as<double>(), dd.as<double>(), dt.as<double>(), n_t, dout.as<double>(), nullptr));
  HIPCHK(tm.stop());
  HIPCHK(hipMemcpy(out, dout.p, dout.bytes, hipMemcpyDeviceToHost));
  if (kernel_ms) HIPCHK(tm.elapsed(*kernel_ms));
  return PHM_OK;
}

int32_t phm_expm_eigen(int32_t n, const double* lefts, const double* rights, const double* d, const double* t,
                       int32_t n_t, int32_t device, double* out, double* kernel_ms) {
  return expm_eigen_impl(false, n, lefts, rights, d, t, n_t, device, out, kernel_ms);
}

int32_t phm_expm_eigen_mfma(int32_t n, const double* lefts, const double* rights, const double* d, const double* t,
                            int32_t n_t, int32_t device, double* out, double* kernel_ms) {
  if (n <= 16 || n > 64) return fail(PHM_ERR_UNSUPPORTED, "phm_expm_eigen_mfma: 16 < n_states <= 64 (smaller matrices do not fill an MFMA tile)");
  return expm_eigen_impl(true, n, lefts, rights, d, t, n_t, device, out, kernel_ms);
}

static int32_t expm_pade_impl(bool mfma, int32_t n, const double* Q, const double* t, int32_t n_t, int32_t device, double* out,
                              double* kernel_ms) {
  if (n < 1 || n > 128 || !Q || !t || !out || n_t < 0) return fail(PHM_ERR_BAD_INPUT, "phm_expm_pade: bad arguments (n <= 128)");
  int32_t st = select_device(device);
  if (st) return st;
  if (n_t == 0) return PHM_OK;
  std::vector<double> Qr;
  cm_to_rm(Q, n, Qr);
  std::vector<int32_t> sq(n_t);
  for (int b = 0; b < n_t; ++b) sq[b] = pade_squarings(Qr.data(), n, t[b]);
  const size_t nn = (size_t)n * n;
  DevBuf dQ, dt, ds, dwork, dout, derr, dbad;
  HIPCHK(upload(dQ, Qr)); HIPCHK(upload(dt, t, n_t)); HIPCHK(upload(ds, sq));
  HIPCHK(dwork.alloc(mfma ? 16 : sizeof(double) * nn * 5 * n_t)); HIPCHK(dout.alloc(sizeof(double) * nn * n_t)); HIPCHK(derr.alloc(sizeof(uint32_t)));
  HIPCHK(hipMemset(derr.p, 0, sizeof(uint32_t)));
  if (mfma) { HIPCHK(dbad.alloc(sizeof(int32_t) * n_t)); HIPCHK(hipMemset(dbad.p, 0, dbad.bytes)); }
  // smallest pivot the unpivoted block elimination accepts (test aid: phm_debug_options.pade_pivot_min = 1e300 sends every matrix to the pivoted kernel)
  const double piv_min = g_phm_debug.pade_pivot_min > 0.0 ? g_phm_debug.pade_pivot_min : 1e-3;
  KernelTimer tm;
  HIPCHK(tm.start());
  if (mfma) HIPCHK(phm::launch_expm_pade_mfma(n, dQ.as<double>(), dt.as<double>(), ds.as<int32_t>(), n_t, dout.as<double>(), dbad.as<int32_t>(), piv_min, nullptr));
  else HIPCHK(phm::launch_expm_pade(n, dQ.as<double>(), dt.as<double>(), ds.as<int32_t>(), n_t, dwork.as<double>(), dout.as<double>(), derr.as<uint32_t>(), nullptr));
  HIPCHK(tm.stop());
  if (mfma) {      // matrices the matrix-core kernel gave up on (a small pivot in a diagonal block of D): the pivoted kernel
    std::vector<int32_t> badh(n_t);
    HIPCHK(hipMemcpy(badh.data(), dbad.p, dbad.bytes, hipMemcpyDeviceToHost));
    std::vector<int32_t> idx;
    for (int b = 0; b < n_t; ++b) if (badh[b]) idx.push_back(b);
    if (!idx.empty()) {
      const int nb = (int)idx.size();
      std::vector<double> tb(nb); std::vector<int32_t> sb(nb);
      for (int i = 0; i < nb; ++i) { tb[i] = t[idx[i]]; sb[i] = sq[idx[i]]; }
      DevBuf dt2, ds2, dwork2, dout2;
      HIPCHK(upload(dt2, tb)); HIPCHK(upload(ds2, sb));
      HIPCHK(dwork2.alloc(sizeof(double) * nn * 5 * nb)); HIPCHK(dout2.alloc(sizeof(double) * nn * nb));
      HIPCHK(phm::launch_expm_pade(n, dQ.as<double>(), dt2.as<double>(), ds2.as<int32_t>(), nb, dwork2.as<double>(), dout2.as<double>(), derr.as<uint32_t>(), nullptr));
      for (int i = 0; i < nb; ++i)
        HIPCHK(hipMemcpy(dout.as<double>() + nn * idx[i], dout2.as<double>() + nn * i, sizeof(double) * nn, hipMemcpyDeviceToDevice));
      HIPCHK(tm.stop());
    }
  }
  HIPCHK(hipMemcpy(out, dout.p, dout.bytes, hipMemcpyDeviceToHost));
  uint32_t derrh = 0;
  HIPCHK(hipMemcpy(&derrh, derr.p, sizeof derrh, hipMemcpyDeviceToHost));
  if (kernel_ms) HIPCHK(tm.elapsed(*kernel_ms));
  if (derrh) return fail(PHM_ERR_BAD_INPUT, "phm_expm_pade: singular Pade denominator");
  return PHM_OK;
}

int32_t phm_expm_pade(int32_t n, const double* Q, const double* t, int32_t n_t, int32_t device, double* out, double* kernel_ms) {
  return expm_pade_impl(false, n, Q, t, n_t, device, out, kernel_ms);
}

int32_t phm_expm_pade_mfma(int32_t n, const double* Q, const double* t, int32_t n_t, int32_t device, double* out,
                           double* kernel_ms) {
  if (n <= 16 || n > 64) return fail(PHM_ERR_UNSUPPORTED, "phm_expm_pade_mfma: 16 < n_states <= 64 (smaller matrices do not fill an MFMA tile)");
  return expm_pade_impl(true, n, Q, t, n_t, device, out, kernel_ms);
}

}  // extern "C"

namespace {

// What every device of a sumstatEXP call shares, checked and derived once on the host (maketreelistEXP, src/phylomap.cpp:3001-3051).
struct ExpInput {
  int n = 0, fx_exp = 0;                       // fx_exp: binary exponent of max(tree length, 1)
  phm::Schedule sched;
  double rate = 0.0;                           // -min diag(Q), :3008
  std::vector<double> L, R, dv, B2, col, PL;   // row-major; col: the chain table of newunifSample (:127); PL: tips one-hot, :2883
  std::vector<uint8_t> tips;                   // 0-based
  std::vector<int32_t> up_order, up_off;       // the pruning pass: positions of sched.up by height
  std::vector<int32_t> walk, walk_off;         // the node draws of the (tile, branch) mapping: edges to an internal node by depth
  const double* edge_length = nullptr;
  const double* pid = nullptr;
};

int32_t exp_prepare(const phm_tree* x, int32_t n, const double* Q, const double* pid, const int32_t* nen, const int32_t* nodelist,
                    int32_t root, const double* lefts, const double* rights, const double* d, ExpInput& in) {
  if (!x || !Q || !pid || !lefts || !rights || !d) return fail(PHM_ERR_BAD_INPUT, "phm_maketreelistEXP: NULL argument");
  if (n < 2) return fail(PHM_ERR_BAD_INPUT, "n_states must be >= 2");
  if (n > 64) return fail(PHM_ERR_UNSUPPORTED, "this build has EXP kernels for n_states <= 64 only");
  if (!x->edge_length) return fail(PHM_ERR_BAD_INPUT, "x$edge.length is required (src/phylomap.cpp:3034)");
  int32_t st = validate_tree_paths(x, n, 1);
  if (st) return st;
  phm::Schedule& s = in.sched;
  std::string serr;
  if (!phm::build_schedule(x->n_tips, x->n_node, x->n_edge, x->edge, s, serr)) return fail(PHM_ERR_BAD_INPUT, "tree: " + serr);
  if (!phm::check_reference_orders(s, x->edge, nen, nodelist, root, serr)) return fail(PHM_ERR_BAD_INPUT, serr);
  st = check_edge_lengths(x);
  if (st) return st;
  in.n = n; in.edge_length = x->edge_length; in.pid = pid;
  cm_to_rm(lefts, n, in.L); cm_to_rm(rights, n, in.R);
  in.dv.resize(n);
  double minq = Q[0];
  for (int i = 0; i < n; ++i) { in.dv[i] = d[i + (size_t)i * n]; minq = std::min(minq, Q[i + (size_t)i * n]); }
  in.rate = -1.0 * minq;                                                        // :3008
  if (!(in.rate > 0.0)) return fail(PHM_ERR_BAD_INPUT, "Q must have a negative diagonal entry");
  in.B2.resize((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const double b = ((i == j) ? 1.0 : 0.0) + Q[i + (size_t)j * n] / in.rate;   // :3011
      if (!(b >= 0.0)) return fail(PHM_ERR_BAD_INPUT, "I + Q/poissonRate must be non-negative");
      in.B2[(size_t)i * n + j] = b;
    }
  std::vector<double> no_row;
  build_chain_tables(in.B2.data(), n, phm::UNIF_CAP + 1, in.col, no_row, false, false);      // unfused sums for every n; no row table
  const int T = s.n_tips;
  in.PL.assign((size_t)(2 * T - 1) * n, 0.0);
  in.tips.resize(T);
  for (int t = 0; t < T; ++t) { in.tips[t] = (uint8_t)(x->states[t] - 1); in.PL[(size_t)t * n + in.tips[t]] = 1.0; }
  phm::height_levels(s.up, in.up_order, in.up_off);
  phm::depth_levels(s, in.walk, in.walk_off, true);
  double tree_len = 0.0;
  for (int b = 0; b < s.n_edge; ++b) tree_len += x->edge_length[b];
  (void)std::frexp(std::max(tree_len, 1.0), &in.fx_exp);
  return PHM_OK;
}

// P(t_b) and the pruning pass are computed ONCE (the reference recomputes both every iteration although Q never changes,
// :2980-2981).  Samples [it0, it0 + N) of the call on one device; out: the caller's column-major matrix of ld_out rows, rows
// it0 .. it0 + N - 1.
int32_t exp_one_device(const ExpInput& in, const phm_options& o, int32_t device, int32_t it0, int32_t N, double* out, int64_t ld_out,
                       phm_maps::Host* mh = nullptr, size_t si = 0) {
  int32_t st = select_device(device);
  if (st) return st;
  const phm::Schedule& s = in.sched;
  const int n = in.n, T = s.n_tips, E = s.n_edge;
  const int tiles = (N + 63) / 64;
  const int cols = n + n * (n - 1);
  // Mapping (phm_options.mapping): PHM_MAP_TILES and PHM_MAP_AUTO: one wave per (tile of 64 samples, branch) (exp_tiles_*);
  // otherwise one wave per tile walks the tree (exp_sample_kernel / exp_wide_kernel).  Maps come from the (tile, branch) kernels.
  const bool use_tiles = mh || o.mapping == PHM_MAP_TILES || o.mapping == PHM_MAP_AUTO;
  DevBuf dL, dR, dd, dt, dP, dPL, dup, duord, ddown, dcol, dB2, dtips, dpid, dnst, dtimes, dout, derr;
  HIPCHK(upload(dL, in.L)); HIPCHK(upload(dR, in.R)); HIPCHK(upload(dd, in.dv)); HIPCHK(upload(dt, in.edge_length, E));
  HIPCHK(upload(dPL, in.PL)); HIPCHK(upload(dup, s.up)); HIPCHK(upload(duord, in.up_order)); HIPCHK(upload(ddown, s.down));
  HIPCHK(upload(dcol, in.col)); HIPCHK(upload(dB2, in.B2)); HIPCHK(upload(dtips, in.tips)); HIPCHK(upload(dpid, in.pid, n));
  HIPCHK(dP.alloc(sizeof(double) * n * n * E)); HIPCHK(dnst.alloc((size_t)tiles * s.n_node * 64));
  if (!use_tiles) HIPCHK(dtimes.alloc(sizeof(double) * (size_t)tiles * phm::UNIF_CAP * 64));      // the walk's jump-time scratch
  HIPCHK(dout.alloc(sizeof(double) * (size_t)N * cols)); HIPCHK(derr.alloc(sizeof(uint32_t)));
  HIPCHK(hipMemset(derr.p, 0, sizeof(uint32_t)));
  HIPCHK(hipMemset(dnst.p, 0, dnst.bytes));

  HIPCHK(phm::launch_expm_eigen(n, dL.as<double>(), dR.as<double>(), dd.as<double>(), dt.as<double>(), E, dP.as<double>(), nullptr));   // :3042
  HIPCHK(phm::launch_exp_pl_levels(n, T, dup.as<phm::UpStep>(), duord.as<int32_t>(), in.up_off, dP.as<double>(), dPL.as<double>(),
                                   o.rescale_pruning != 0, nullptr));                                                              // :3043
  HIPCHK(hipDeviceSynchronize());      // the set-up is not part of the sampler's time
  // the N x cols samples into rows it0 .. of the caller's matrix (one shard: the whole, contiguous matrix), then the error word
  auto copy_out = [&]() -> int32_t {
    if (ld_out == N) HIPCHK(hipMemcpy(out, dout.p, dout.bytes, hipMemcpyDeviceToHost));
    else HIPCHK(hipMemcpy2D(out + it0, sizeof(double) * ld_out, dout.p, sizeof(double) * N, sizeof(double) * N, cols, hipMemcpyDeviceToHost));
    uint32_t derrh = 0;
    HIPCHK(hipMemcpy(&derrh, derr.p, sizeof derrh, hipMemcpyDeviceToHost));
    return device_status(derrh);
  };
  // the parameters every sampler has under the same names
  auto fill_common = [&](auto& p) {
    p.n_tips = T; p.n_node = s.n_node; p.n_edge = E; p.root = s.root; p.N = N; p.n_tiles = tiles; p.it0 = it0;
    p.seed_lo = (uint32_t)(o.seed & 0xFFFFFFFFull); p.seed_hi = (uint32_t)(o.seed >> 32); p.replica = (uint32_t)o.replica_offset;
    p.poisson_rate = in.rate;
    p.down = ddown.as<phm::DownStep>(); p.P = dP.as<double>(); p.PL = dPL.as<double>(); p.edge_length = dt.as<double>();
    p.colpow = dcol.as<double>(); p.B2 = dB2.as<double>(); p.tips = dtips.as<uint8_t>(); p.nstate = dnst.as<uint8_t>();
    p.out = dout.as<double>(); p.err = derr.as<uint32_t>();
  };
  KernelTimer tm;      // the sampler alone (phm_last_kernel_ms)
  if (use_tiles) {
    const int64_t items = (int64_t)E * tiles;
    const int branch_blocks = (int)std::min<int64_t>((items + 3) / 4, 2048);
    const size_t npad = (size_t)tiles * 64;
    DevBuf dorder, ddw, dcnt, dtm;
    HIPCHK(upload(dorder, in.walk));
    HIPCHK(ddw.alloc(sizeof(unsigned long long) * n * npad)); HIPCHK(dcnt.alloc(sizeof(uint32_t) * (size_t)n * (n - 1) * npad));
    HIPCHK(dtm.alloc(sizeof(double) * (size_t)branch_blocks * 4 * phm::UNIF_CAP * 64));
    HIPCHK(hipMemset(ddw.p, 0, ddw.bytes)); HIPCHK(hipMemset(dcnt.p, 0, dcnt.bytes));
    phm::ExpTilesParams p;
    fill_common(p);
    p.n_states = n; p.pid = dpid.as<double>(); p.node_order = dorder.as<int32_t>(); p.times = dtm.as<double>();
    p.fx_scale = std::ldexp(1.0, 61 - in.fx_exp); p.fx_inv = std::ldexp(1.0, in.fx_exp - 61);
    p.dwfx = ddw.as<unsigned long long>(); p.cnt = dcnt.as<uint32_t>();
    phm_maps::Shard ms;
    if (mh) {
      st = ms.setup(*mh, it0, N, (int64_t)npad, p.maps);
      if (st) return st;
    }
    HIPCHK(tm.start());
    HIPCHK(phm::launch_exp_tiles(p, in.walk_off, branch_blocks, nullptr, mh ? mh->mode : phm::MAPS_OFF));
    if (mh) HIPCHK(ms.after_kernel(*mh, (int64_t)npad, nullptr));      // sizing: counts -> offsets
    HIPCHK(tm.stop());
    HIPCHK(tm.elapsed(g_phm_last_kernel_ms));
    st = copy_out();
    if (st || !mh) return st;
    return ms.copy_home(*mh, si, "phm_maketreelistEXP_maps");
  }
  auto fill_small = [&](auto& p) {
    fill_common(p);
    for (int i = 0; i < n; ++i) p.pid[i] = in.pid[i];
    p.times = dtimes.as<double>();
  };
  HIPCHK(tm.start());
  if (n == 2) { phm::ExpParams<2> p; fill_small(p); HIPCHK(phm::launch_exp_sample<2>(p, nullptr)); }
  if (n == 3) { phm::ExpParams<3> p; fill_small(p); HIPCHK(phm::launch_exp_sample<3>(p, nullptr)); }
  if (n == 4) { phm::ExpParams<4> p; fill_small(p); HIPCHK(phm::launch_exp_sample<4>(p, nullptr)); }
  if (n > 4) {
    HIPCHK(hipMemset(dout.p, 0, dout.bytes));
    phm::ExpWideParams p;
    fill_common(p);
    p.n_states = n; p.pid = dpid.as<double>(); p.times = dtimes.as<double>();
    HIPCHK(phm::launch_exp_wide(p, nullptr));
    HIPCHK(hipDeviceSynchronize());
  }
  HIPCHK(tm.stop());
  HIPCHK(tm.elapsed(g_phm_last_kernel_ms));
  return copy_out();
}

}  // namespace

extern "C" {

// The samples are i.i.d. and addressed by their index (src/phylomap.cpp:3045-3048): with phm_options.n_devices > 1 device d draws
// a contiguous range of the N samples (run_shards) into its rows of `out` -- the matrix is the one-device matrix row for row.
int32_t phm_maketreelistEXP(const phm_tree* x, int32_t n, const double* Q, const double* pid, const int32_t* nen,
                            const int32_t* nodelist, int32_t root, int32_t N, const double* lefts, const double* rights,
                            const double* d, const phm_options* opt_in, double* out) {
  if (!out) return fail(PHM_ERR_BAD_INPUT, "phm_maketreelistEXP: NULL argument");
  if (N < 1) return fail(PHM_ERR_BAD_INPUT, "N must be >= 1");
  const phm_options o = resolve_options(opt_in);
  ExpInput in;
  int32_t st = exp_prepare(x, n, Q, pid, nen, nodelist, root, lefts, rights, d, in);
  if (st) return st;
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, N, shards);
  if (st) return st;
  return run_shards(shards, [&](const phm_shard& sh, size_t) {
    return exp_one_device(in, o, sh.device, (int32_t)sh.first, (int32_t)sh.count, out, N);
  });
}

// The same call, plus the stochastic maps of the N samples, from the (tile, branch) kernels: a sizing call
// (map_dwell and map_state NULL) writes map_off, a filling call reads it and writes the segments.
int32_t phm_maketreelistEXP_maps(const phm_tree* x, int32_t n, const double* Q, const double* pid, const int32_t* nen,
                                 const int32_t* nodelist, int32_t root, int32_t N, const double* lefts, const double* rights,
                                 const double* d, const phm_options* opt_in, double* out,
                                 int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state) {
  if (!x || !out) return fail(PHM_ERR_BAD_INPUT, "phm_maketreelistEXP_maps: NULL argument");
  if (N < 1) return fail(PHM_ERR_BAD_INPUT, "N must be >= 1");
  const phm_options o = resolve_options(opt_in);
  if (o.mapping != PHM_MAP_AUTO && o.mapping != PHM_MAP_TILES)
    return fail(PHM_ERR_UNSUPPORTED, "phm_maketreelistEXP_maps: maps come from the (tile, branch) kernels (mapping PHM_MAP_AUTO or PHM_MAP_TILES)");
  phm_maps::Host mh;
  int32_t st = phm_maps::validate("phm_maketreelistEXP_maps", N, x->n_edge, map_off, map_cap, map_dwell, map_state, mh);
  if (st) return st;
  ExpInput in;
  st = exp_prepare(x, n, Q, pid, nen, nodelist, root, lefts, rights, d, in);
  if (st) return st;
  std::vector<phm_shard> shards;
  st = phm_plan_shards(o, N, shards);
  if (st) return st;
  mh.shard_total.assign(shards.size(), 0);
  st = run_shards(shards, [&](const phm_shard& sh, size_t i) {
    return exp_one_device(in, o, sh.device, (int32_t)sh.first, (int32_t)sh.count, out, N, &mh, i);
  });
  if (st) return st;
  phm_maps::finish_sizing(mh, shards);
  return PHM_OK;
}

double phm_last_kernel_ms(void) { return g_phm_last_kernel_ms; }

}  // extern "C"
