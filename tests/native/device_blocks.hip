// device_blocks.hip -- TEST INFRASTRUCTURE ONLY: one small kernel per device building block of phm_device.h, phm_coop.h,
// phm_history.h and phm_ll_device.h, each behind an extern "C" entry that uploads its inputs, launches, synchronises, copies back and returns the
// hipError_t as an int (tests/blocks_lib.py, tests/test_gpu_device_blocks.py).  Built with the library's own flags into
// build/tests/libphm_device_blocks.so; never linked into libphylomap_hip.so.
//
// Every kernel runs workgroups of 256 threads = four waves.  A wave-cooperative block gets one input vector and one 64-double
// LDS vector PER WAVE, as in the calling kernels, and every lane writes what it received.  No kernel reads or writes beyond the
// element counts its entry is given: per-item kernels return for items >= N, per-wave kernels for waves >= nw (after the
// workgroup's only barrier), state counts outside 1..64 and widths outside the staged arrays are refused on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "phm_device.h"
#include "phm_coop.h"
#include "phm_history.h"
#include "phm_ll_device.h"

using namespace phm;

namespace {

constexpr int TB = 256;              // threads per workgroup: four waves
constexpr int ELL_MAX = 8;           // widest ELLPACK row the harness stages
constexpr int PHMTB_BAD_ARG = -1;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// a device buffer that lives for one entry call
template <class T>
struct Buf {
  T* p = nullptr;
  size_t n = 0;
  ~Buf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t count) { n = count; return hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * (count ? count : 1)); }
  hipError_t up(const T* h, size_t count) {
    hipError_t e = alloc(count);
    if (e != hipSuccess || !count) return e;
    return hipMemcpy(p, h, sizeof(T) * count, hipMemcpyHostToDevice);
  }
  hipError_t zero(size_t count) {
    hipError_t e = alloc(count);
    if (e != hipSuccess) return e;
    return hipMemset(p, 0, sizeof(T) * (count ? count : 1));
  }
  hipError_t down(T* h) const { return n ? hipMemcpy(h, p, sizeof(T) * n, hipMemcpyDeviceToHost) : hipSuccess; }
};

int finish() {
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  return 0;
}

inline int blocks_for(long long items) { return (int)((items + TB - 1) / TB); }

// ---- phm_device.h: Philox, u01, streams -----------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void k_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out, int N) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= N) return;
  uint32_t o[4];
  philox4x32(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1], o);
  for (int q = 0; q < 4; ++q) out[4 * i + q] = o[q];
}

__global__ __launch_bounds__(TB) void k_u01(const uint32_t* x, double* out, int N) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= N) return;
  out[i] = u01(x[i]);
}

// One stream per lane (its own replica, iteration and entity); the draws dseq[0 .. nd) are asked for in the given order from two
// Stream objects (one through draw_word, one through draw) and afresh through stream_word and stream_u.
__global__ __launch_bounds__(TB) void k_stream(uint32_t seed_lo, uint32_t seed_hi, const uint32_t* rep, const uint32_t* iter,
                                               const uint32_t* ent, const uint32_t* dseq, int nd, uint32_t* w_kept, double* u_kept,
                                               uint32_t* w_fresh, double* u_fresh, int N) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= N) return;
  Stream sw, su;
  sw.open(ent[i], iter[i], rep[i], seed_lo, seed_hi);
  su.open(ent[i], iter[i], rep[i], seed_lo, seed_hi);
  for (int q = 0; q < nd; ++q) {
    const uint32_t d = dseq[q];
    const size_t o = (size_t)i * nd + q;
    w_kept[o] = sw.draw_word(d);
    u_kept[o] = su.draw(d);
    w_fresh[o] = stream_word(seed_lo, seed_hi, rep[i], iter[i], ent[i], d);
    u_fresh[o] = stream_u(seed_lo, seed_hi, rep[i], iter[i], ent[i], d);
  }
}

// ---- neglog_u32 with the table staged as the kernels stage it: logtab_entry into a 16-byte-aligned buffer, in LDS and in global memory
__global__ __launch_bounds__(TB) void k_logtab_fill(double* gtab) {
  for (int i = threadIdx.x; i < 2 * PHM_LOGTAB_N; i += TB) gtab[i] = logtab_entry(i);
}

__global__ __launch_bounds__(TB) void k_neglog(const uint32_t* k, const double* gtab, double* out_lds, double* out_glb, int N) {
  __shared__ __align__(16) double s_ltab[2 * PHM_LOGTAB_N];
  for (int i = threadIdx.x; i < 2 * PHM_LOGTAB_N; i += TB) s_ltab[i] = logtab_entry(i);
  __syncthreads();
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= N) return;
  out_lds[i] = neglog_u32(k[i], s_ltab);
  out_glb[i] = neglog_u32(k[i], gtab);
}

__global__ __launch_bounds__(TB) void k_log(const double* x, double* out, int N) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= N) return;
  out[i] = phm_log(x[i]);
}

__global__ __launch_bounds__(TB) void k_exp(const double* x, double* out, int N) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= N) return;
  out[i] = phm_exp(x[i]);
}

// ---- n <= 4: matvec_u and sample_cat, one problem per lane ---------------------------------------------------------------
template <int NS>
__global__ __launch_bounds__(TB) void k_matvec_u(const double* M, const double* v, double* out, int N) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= N) return;
  double x[NS];
  for (int j = 0; j < NS; ++j) x[j] = v[(size_t)i * NS + j];
  matvec_u<NS>(M + (size_t)i * NS * NS, x);
  for (int j = 0; j < NS; ++j) out[(size_t)i * NS + j] = x[j];
}

template <int NS>
__global__ __launch_bounds__(TB) void k_sample_cat(const double* p, const double* u, int32_t* idx, uint32_t* err, int N) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= N) return;
  double x[NS];
  for (int j = 0; j < NS; ++j) x[j] = p[(size_t)i * NS + j];
  uint32_t e = 0;
  idx[i] = sample_cat<NS>(x, u[i], e);
  err[i] = e;
}

// ---- phm_coop.h: the matrix-vector forms --------------------------------------------------------------------------------------
// form 0 coop_matvec, 1 coop_matvec_lds, 2 coop_matvec_regs, 3 coop_matvec_ell, 4 coop_matvec_band<1>, 5 coop_matvec_band<2>.
// The dense matrix (row stride ldn) and the ELLPACK rows are staged in LDS, the register row of form 2 and the band coefficients
// are those of row c = min(lane, n - 1), as at the call sites.  out1 = f(v), out2 = f(out1): the second product overwrites the
// LDS vector the first one read.
template <int FORM>
__global__ __launch_bounds__(TB) void k_matvec(int n, int ldn, const double* M, const int32_t* ecol, const double* eval, int w,
                                               const double* coef, const double* vin, double* out1, double* out2, int nw) {
  __shared__ __align__(16) double s_M[64 * 65];
  __shared__ __align__(16) double s_vec[TB / 64][64];
  __shared__ double s_eval[64 * ELL_MAX];
  __shared__ int32_t s_ecol[64 * ELL_MAX];
  if (FORM <= 2) for (int i = threadIdx.x; i < n * ldn; i += TB) s_M[i] = M[i];
  if (FORM == 3) for (int i = threadIdx.x; i < n * w; i += TB) { s_eval[i] = eval[i]; s_ecol[i] = ecol[i]; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gw = blockIdx.x * (TB / 64) + wave;
  if (gw >= nw) return;
  const int c = lane < n ? lane : n - 1;
  const double v = vin[(size_t)gw * 64 + lane];
  double y1, y2;
  if constexpr (FORM == 0) {
    y1 = coop_matvec(s_M, v, n, ldn, c);
    y2 = coop_matvec(s_M, y1, n, ldn, c);
  } else if constexpr (FORM == 1) {
    y1 = coop_matvec_lds(s_M, s_vec[wave], v, n, ldn, c, lane);
    y2 = coop_matvec_lds(s_M, s_vec[wave], y1, n, ldn, c, lane);
  } else if constexpr (FORM == 2) {
    double brow[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) brow[j] = (j < n) ? s_M[c * ldn + j] : 0.0;
    y1 = coop_matvec_regs(brow, s_vec[wave], v, n, lane);
    y2 = coop_matvec_regs(brow, s_vec[wave], y1, n, lane);
  } else if constexpr (FORM == 3) {
    y1 = coop_matvec_ell(s_ecol, s_eval, v, w, c);
    y2 = coop_matvec_ell(s_ecol, s_eval, y1, w, c);
  } else {
    double cf[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) cf[q] = coef[lane * 5 + q];
    y1 = coop_matvec_band<FORM - 3>(cf, v, lane);
    y2 = coop_matvec_band<FORM - 3>(cf, y1, lane);
  }
  out1[(size_t)gw * 64 + lane] = y1;
  out2[(size_t)gw * 64 + lane] = y2;
}

__global__ __launch_bounds__(TB) void k_shift(const unsigned long long* in, unsigned long long* below, unsigned long long* above, int nw) {
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
  if (gw >= nw) return;
  const double x = __longlong_as_double((long long)in[(size_t)gw * 64 + lane]);
  below[(size_t)gw * 64 + lane] = (unsigned long long)__double_as_longlong(wave_from_below(x, lane));
  above[(size_t)gw * 64 + lane] = (unsigned long long)__double_as_longlong(wave_from_above(x, lane));
}

// out[(gw * n + l) * 64 + lane] = what `lane` received from readlane_f64(v, l), l = 0 .. n - 1
__global__ __launch_bounds__(TB) void k_readlane(const unsigned long long* in, int n, unsigned long long* out, int nw) {
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
  if (gw >= nw) return;
  const double x = __longlong_as_double((long long)in[(size_t)gw * 64 + lane]);
  for (int l = 0; l < n; ++l)
    out[((size_t)gw * n + l) * 64 + lane] = (unsigned long long)__double_as_longlong(readlane_f64(x, l));
}

__global__ __launch_bounds__(TB) void k_coop_sum(const double* in, int n, double* out, int nw) {
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
  if (gw >= nw) return;
  out[(size_t)gw * 64 + lane] = coop_sum(in[(size_t)gw * 64 + lane], n);
}

// which 0: coop_sample, 1: coop_sample_lds; u is one value per wave, as at the call sites
__global__ __launch_bounds__(TB) void k_coop_sample(int which, int n, const double* p, const double* u, int32_t* idx, uint32_t* err, int nw) {
  __shared__ __align__(16) double s_pv[TB / 64][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gw = blockIdx.x * (TB / 64) + wave;
  if (gw >= nw) return;
  const double pr = p[(size_t)gw * 64 + lane];
  uint32_t e = 0;
  int r;
  if (which == 0) r = coop_sample(pr, u[gw], n, lane, e);
  else r = coop_sample_lds(pr, u[gw], n, lane, s_pv[wave], e);
  idx[(size_t)gw * 64 + lane] = r;
  err[(size_t)gw * 64 + lane] = e;
}

// which 0: wave_max_count, 1: wave_max_w, 2: the minimum idiom 65535 - wave_max_count(65535 - k)
__global__ __launch_bounds__(TB) void k_wave_max(int which, const int32_t* in, int32_t* out, int nw) {
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
  if (gw >= nw) return;
  const int v = in[(size_t)gw * 64 + lane];
  int r;
  if (which == 0) r = wave_max_count(v);
  else if (which == 1) r = wave_max_w(v);
  else r = 65535 - wave_max_count(65535 - v);
  out[(size_t)gw * 64 + lane] = r;
}

// ---- phm_history.h --------------------------------------------------------------------------------------------------------------
// One item per lane: nseg segments (dwell column, dwell, count column or -1) into the lane's cell.  NS > 0: n = NS states and
// NS * NS count columns; NS = 0: run-time n and ncount.
template <int NS>
__global__ __launch_bounds__(TB) void k_statlanes(int n, int ncount, int nseg, const int32_t* dcol, const double* dx, const int32_t* ccol,
                                                  const int32_t* cell, const uint8_t* live, size_t pad, double fx_scale,
                                                  unsigned long long* dwfx, uint32_t* cnt, int N) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= N) return;
  StatLanes<NS, NS * NS> st;
  st.begin(dwfx, cnt, pad, (size_t)cell[i], fx_scale, live[i] != 0);
  for (int s = 0; s < nseg; ++s) {
    const size_t o = (size_t)i * nseg + s;
    const int dc = dcol[o], cc = ccol[o];
    if (dc >= 0 && dc < n) st.dwell(dc, dx[o]);
    if (cc >= 0 && cc < ncount) st.count(cc);
  }
  st.flush();
}

__global__ __launch_bounds__(TB) void k_stat_value(const unsigned long long* dwfx, const uint32_t* cnt, int n, int ncol, size_t pad,
                                                   double fx_inv, double* out, int ncell) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= ncell * ncol) return;
  const int c = i / ncell, cellno = i % ncell;
  out[i] = stat_cell_value(dwfx, cnt, n, c, pad, (size_t)cellno, fx_inv);
}

// ---- phm_ll_device.h ------------------------------------------------------------------------------------------------------------
// One vector of N doubles per lane, its maximum taken as the passes take it (fmax from 0).
template <int N>
__global__ __launch_bounds__(TB) void k_ll_rescale(const double* v, double* out, int32_t* e, int cnt) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= cnt) return;
  double x[N], mx = 0.0;
  for (int j = 0; j < N; ++j) { x[j] = v[(size_t)i * N + j]; mx = fmax(mx, x[j]); }
  e[i] = ll_rescale<N>(x, mx);
  for (int j = 0; j < N; ++j) out[(size_t)i * N + j] = x[j];
}

// One model per lane in the model-fastest layout: entry e of model k at Q[e * K + k]
__global__ __launch_bounds__(TB) void k_model(int n, const double* Q, double* mu, double* B, int K) {
  const int k = blockIdx.x * TB + threadIdx.x;
  if (k >= K) return;
  const double m = model_mu(Q + k, (size_t)K, n);
  mu[k] = m;
  for (int e = 0; e < n * n; ++e) B[(size_t)e * K + k] = model_b(Q[(size_t)e * K + k], m, e / n == e % n ? 1.0 : 0.0);
}

}  // namespace

extern "C" {

int phmtb_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out, int N) {
  if (N < 0) return PHMTB_BAD_ARG;
  Buf<uint32_t> dc, dk, dout;
  CK(dc.up(ctr, 4 * (size_t)N)); CK(dk.up(key, 2 * (size_t)N)); CK(dout.zero(4 * (size_t)N));
  if (N) k_philox<<<blocks_for(N), TB>>>(dc.p, dk.p, dout.p, N);
  if (int e = finish()) return e;
  CK(dout.down(out));
  return 0;
}

int phmtb_u01(const uint32_t* x, double* out, int N) {
  if (N < 0) return PHMTB_BAD_ARG;
  Buf<uint32_t> dx; Buf<double> dout;
  CK(dx.up(x, N)); CK(dout.zero(N));
  if (N) k_u01<<<blocks_for(N), TB>>>(dx.p, dout.p, N);
  if (int e = finish()) return e;
  CK(dout.down(out));
  return 0;
}

int phmtb_stream(uint32_t seed_lo, uint32_t seed_hi, const uint32_t* rep, const uint32_t* iter, const uint32_t* ent,
                 const uint32_t* dseq, int nd, uint32_t* w_kept, double* u_kept, uint32_t* w_fresh, double* u_fresh, int N) {
  if (N < 0 || nd < 0) return PHMTB_BAD_ARG;
  Buf<uint32_t> dr, di, de, dd, dwk, dwf; Buf<double> duk, duf;
  const size_t tot = (size_t)N * nd;
  CK(dr.up(rep, N)); CK(di.up(iter, N)); CK(de.up(ent, N)); CK(dd.up(dseq, nd));
  CK(dwk.zero(tot)); CK(dwf.zero(tot)); CK(duk.zero(tot)); CK(duf.zero(tot));
  if (N) k_stream<<<blocks_for(N), TB>>>(seed_lo, seed_hi, dr.p, di.p, de.p, dd.p, nd, dwk.p, duk.p, dwf.p, duf.p, N);
  if (int e = finish()) return e;
  CK(dwk.down(w_kept)); CK(duk.down(u_kept)); CK(dwf.down(w_fresh)); CK(duf.down(u_fresh));
  return 0;
}

int phmtb_neglog(const uint32_t* k, double* out_lds, double* out_glb, int N) {
  if (N < 0) return PHMTB_BAD_ARG;
  Buf<uint32_t> dk; Buf<double> dtab, dl, dg;
  CK(dk.up(k, N)); CK(dtab.zero(2 * PHM_LOGTAB_N)); CK(dl.zero(N)); CK(dg.zero(N));     // hipMalloc aligns to 256 bytes
  k_logtab_fill<<<1, TB>>>(dtab.p);
  if (N) k_neglog<<<blocks_for(N), TB>>>(dk.p, dtab.p, dl.p, dg.p, N);
  if (int e = finish()) return e;
  CK(dl.down(out_lds)); CK(dg.down(out_glb));
  return 0;
}

int phmtb_log(const double* x, double* out, int N) {
  if (N < 0) return PHMTB_BAD_ARG;
  Buf<double> dx, dout;
  CK(dx.up(x, N)); CK(dout.zero(N));
  if (N) k_log<<<blocks_for(N), TB>>>(dx.p, dout.p, N);
  if (int e = finish()) return e;
  CK(dout.down(out));
  return 0;
}

int phmtb_exp(const double* x, double* out, int N) {
  if (N < 0) return PHMTB_BAD_ARG;
  Buf<double> dx, dout;
  CK(dx.up(x, N)); CK(dout.zero(N));
  if (N) k_exp<<<blocks_for(N), TB>>>(dx.p, dout.p, N);
  if (int e = finish()) return e;
  CK(dout.down(out));
  return 0;
}

int phmtb_matvec_u(int ns, const double* M, const double* v, double* out, int N) {
  if (N < 0 || ns < 2 || ns > 4) return PHMTB_BAD_ARG;
  Buf<double> dM, dv, dout;
  CK(dM.up(M, (size_t)N * ns * ns)); CK(dv.up(v, (size_t)N * ns)); CK(dout.zero((size_t)N * ns));
  if (N) {
    if (ns == 2) k_matvec_u<2><<<blocks_for(N), TB>>>(dM.p, dv.p, dout.p, N);
    else if (ns == 3) k_matvec_u<3><<<blocks_for(N), TB>>>(dM.p, dv.p, dout.p, N);
    else k_matvec_u<4><<<blocks_for(N), TB>>>(dM.p, dv.p, dout.p, N);
  }
  if (int e = finish()) return e;
  CK(dout.down(out));
  return 0;
}

int phmtb_sample_cat(int ns, const double* p, const double* u, int32_t* idx, uint32_t* err, int N) {
  if (N < 0 || ns < 2 || ns > 4) return PHMTB_BAD_ARG;
  Buf<double> dp, du; Buf<int32_t> di; Buf<uint32_t> de;
  CK(dp.up(p, (size_t)N * ns)); CK(du.up(u, N)); CK(di.zero(N)); CK(de.zero(N));
  if (N) {
    if (ns == 2) k_sample_cat<2><<<blocks_for(N), TB>>>(dp.p, du.p, di.p, de.p, N);
    else if (ns == 3) k_sample_cat<3><<<blocks_for(N), TB>>>(dp.p, du.p, di.p, de.p, N);
    else k_sample_cat<4><<<blocks_for(N), TB>>>(dp.p, du.p, di.p, de.p, N);
  }
  if (int e = finish()) return e;
  CK(di.down(idx)); CK(de.down(err));
  return 0;
}

// M: n rows of stride ldn (forms 0-2); ecol / eval: n rows of w entries, columns in 0 .. n - 1 (form 3); coef: 64 lanes x 5 (forms 4, 5);
// vin, out1, out2: nw waves x 64 lanes
int phmtb_matvec(int form, int n, int ldn, const double* M, const int32_t* ecol, const double* eval, int w, const double* coef,
                 const double* vin, double* out1, double* out2, int nw) {
  if (form < 0 || form > 5 || n < 1 || n > 64 || nw < 0) return PHMTB_BAD_ARG;
  if (form <= 2 && (ldn < n || ldn > 65)) return PHMTB_BAD_ARG;
  if (form == 3) {
    if (w < 1 || w > ELL_MAX) return PHMTB_BAD_ARG;
    for (int i = 0; i < n * w; ++i) if (ecol[i] < 0 || ecol[i] >= n) return PHMTB_BAD_ARG;
  }
  Buf<double> dM, dval, dcoef, dv, d1, d2; Buf<int32_t> dcol;
  CK(dM.up(M, form <= 2 ? (size_t)n * ldn : 0));
  CK(dcol.up(ecol, form == 3 ? (size_t)n * w : 0)); CK(dval.up(eval, form == 3 ? (size_t)n * w : 0));
  CK(dcoef.up(coef, form >= 4 ? 64 * 5 : 0));
  CK(dv.up(vin, (size_t)nw * 64)); CK(d1.zero((size_t)nw * 64)); CK(d2.zero((size_t)nw * 64));
  const int g = (nw + 3) / 4;
  if (nw) switch (form) {
    case 0: k_matvec<0><<<g, TB>>>(n, ldn, dM.p, dcol.p, dval.p, w, dcoef.p, dv.p, d1.p, d2.p, nw); break;
    case 1: k_matvec<1><<<g, TB>>>(n, ldn, dM.p, dcol.p, dval.p, w, dcoef.p, dv.p, d1.p, d2.p, nw); break;
    case 2: k_matvec<2><<<g, TB>>>(n, ldn, dM.p, dcol.p, dval.p, w, dcoef.p, dv.p, d1.p, d2.p, nw); break;
    case 3: k_matvec<3><<<g, TB>>>(n, ldn, dM.p, dcol.p, dval.p, w, dcoef.p, dv.p, d1.p, d2.p, nw); break;
    case 4: k_matvec<4><<<g, TB>>>(n, ldn, dM.p, dcol.p, dval.p, w, dcoef.p, dv.p, d1.p, d2.p, nw); break;
    default: k_matvec<5><<<g, TB>>>(n, ldn, dM.p, dcol.p, dval.p, w, dcoef.p, dv.p, d1.p, d2.p, nw); break;
  }
  if (int e = finish()) return e;
  CK(d1.down(out1)); CK(d2.down(out2));
  return 0;
}

int phmtb_shift(const unsigned long long* in, unsigned long long* below, unsigned long long* above, int nw) {
  if (nw < 0) return PHMTB_BAD_ARG;
  Buf<unsigned long long> di, db, da;
  CK(di.up(in, (size_t)nw * 64)); CK(db.zero((size_t)nw * 64)); CK(da.zero((size_t)nw * 64));
  if (nw) k_shift<<<(nw + 3) / 4, TB>>>(di.p, db.p, da.p, nw);
  if (int e = finish()) return e;
  CK(db.down(below)); CK(da.down(above));
  return 0;
}

int phmtb_readlane(const unsigned long long* in, int n, unsigned long long* out, int nw) {
  if (nw < 0 || n < 1 || n > 64) return PHMTB_BAD_ARG;
  Buf<unsigned long long> di, dout;
  CK(di.up(in, (size_t)nw * 64)); CK(dout.zero((size_t)nw * n * 64));
  if (nw) k_readlane<<<(nw + 3) / 4, TB>>>(di.p, n, dout.p, nw);
  if (int e = finish()) return e;
  CK(dout.down(out));
  return 0;
}

int phmtb_coop_sum(const double* in, int n, double* out, int nw) {
  if (nw < 0 || n < 1 || n > 64) return PHMTB_BAD_ARG;
  Buf<double> di, dout;
  CK(di.up(in, (size_t)nw * 64)); CK(dout.zero((size_t)nw * 64));
  if (nw) k_coop_sum<<<(nw + 3) / 4, TB>>>(di.p, n, dout.p, nw);
  if (int e = finish()) return e;
  CK(dout.down(out));
  return 0;
}

int phmtb_coop_sample(int which, int n, const double* p, const double* u, int32_t* idx, uint32_t* err, int nw) {
  if (nw < 0 || n < 1 || n > 64 || which < 0 || which > 1) return PHMTB_BAD_ARG;
  Buf<double> dp, du; Buf<int32_t> di; Buf<uint32_t> de;
  CK(dp.up(p, (size_t)nw * 64)); CK(du.up(u, nw)); CK(di.zero((size_t)nw * 64)); CK(de.zero((size_t)nw * 64));
  if (nw) k_coop_sample<<<(nw + 3) / 4, TB>>>(which, n, dp.p, du.p, di.p, de.p, nw);
  if (int e = finish()) return e;
  CK(di.down(idx)); CK(de.down(err));
  return 0;
}

int phmtb_wave_max(int which, const int32_t* in, int32_t* out, int nw) {
  if (nw < 0 || which < 0 || which > 2) return PHMTB_BAD_ARG;
  Buf<int32_t> di, dout;
  CK(di.up(in, (size_t)nw * 64)); CK(dout.zero((size_t)nw * 64));
  if (nw) k_wave_max<<<(nw + 3) / 4, TB>>>(which, di.p, dout.p, nw);
  if (int e = finish()) return e;
  CK(dout.down(out));
  return 0;
}

// N items of nseg segments each into ncell cells of n dwell and ncount count columns (column stride = ncell).  dwfx and cnt hold
// the cells' initial contents on entry and their final contents on return; values[(c * ncell) + cell] = stat_cell_value of
// column c < n + ncount.  ns = 0: StatLanes<0, 0> with run-time n, ncount; ns = 2, 3, 4: StatLanes<ns, ns * ns> (n = ns, ncount = ns * ns).
int phmtb_statlanes(int ns, int n, int ncount, int nseg, const int32_t* dcol, const double* dx, const int32_t* ccol, const int32_t* cell,
                    const uint8_t* live, int ncell, double fx_scale, double fx_inv, unsigned long long* dwfx, uint32_t* cnt,
                    double* values, int N) {
  if (N < 0 || nseg < 0 || ncell < 1 || n < 1 || n > 64 || ncount < 0) return PHMTB_BAD_ARG;
  if (ns != 0 && (ns < 2 || ns > 4 || n != ns || ncount != ns * ns)) return PHMTB_BAD_ARG;
  for (int i = 0; i < N; ++i) if (cell[i] < 0 || cell[i] >= ncell) return PHMTB_BAD_ARG;
  const size_t tot = (size_t)N * nseg, ncol = (size_t)n + ncount;
  Buf<int32_t> ddc, dcc, dcell; Buf<double> ddx, dval; Buf<uint8_t> dlive; Buf<unsigned long long> ddw; Buf<uint32_t> dcnt;
  CK(ddc.up(dcol, tot)); CK(ddx.up(dx, tot)); CK(dcc.up(ccol, tot)); CK(dcell.up(cell, N)); CK(dlive.up(live, N));
  CK(ddw.up(dwfx, (size_t)n * ncell)); CK(dcnt.up(cnt, (size_t)ncount * ncell)); CK(dval.zero(ncol * ncell));
  if (N) {
    const int g = blocks_for(N);
    if (ns == 0) k_statlanes<0><<<g, TB>>>(n, ncount, nseg, ddc.p, ddx.p, dcc.p, dcell.p, dlive.p, (size_t)ncell, fx_scale, ddw.p, dcnt.p, N);
    else if (ns == 2) k_statlanes<2><<<g, TB>>>(n, ncount, nseg, ddc.p, ddx.p, dcc.p, dcell.p, dlive.p, (size_t)ncell, fx_scale, ddw.p, dcnt.p, N);
    else if (ns == 3) k_statlanes<3><<<g, TB>>>(n, ncount, nseg, ddc.p, ddx.p, dcc.p, dcell.p, dlive.p, (size_t)ncell, fx_scale, ddw.p, dcnt.p, N);
    else k_statlanes<4><<<g, TB>>>(n, ncount, nseg, ddc.p, ddx.p, dcc.p, dcell.p, dlive.p, (size_t)ncell, fx_scale, ddw.p, dcnt.p, N);
  }
  k_stat_value<<<blocks_for((long long)ncol * ncell), TB>>>(ddw.p, dcnt.p, n, (int)ncol, (size_t)ncell, fx_inv, dval.p, ncell);
  if (int e = finish()) return e;
  CK(ddw.down(dwfx)); CK(dcnt.down(cnt)); CK(dval.down(values));
  return 0;
}

// cnt vectors of n doubles, n = 2 .. 8 through ll_with_states: out = the rescaled vectors, e = the exponents
int phmtb_ll_rescale(int n, const double* v, double* out, int32_t* e, int cnt) {
  if (cnt < 0 || n < 2 || n > LL_LANE_MAX) return PHMTB_BAD_ARG;
  Buf<double> dv, dout; Buf<int32_t> de;
  CK(dv.up(v, (size_t)cnt * n)); CK(dout.zero((size_t)cnt * n)); CK(de.zero(cnt));
  if (cnt) ll_with_states(n, [&](auto ns) { k_ll_rescale<decltype(ns)::value><<<blocks_for(cnt), TB>>>(dv.p, dout.p, de.p, cnt); });
  if (int err = finish()) return err;
  CK(dout.down(out)); CK(de.down(e));
  return 0;
}

// Q, B: [n * n][K] model-fastest; mu: [K]
int phmtb_model(int n, const double* Q, double* mu, double* B, int K) {
  if (K < 0 || n < 1 || n > 64) return PHMTB_BAD_ARG;
  Buf<double> dq, dmu, db;
  CK(dq.up(Q, (size_t)n * n * K)); CK(dmu.zero(K)); CK(db.zero((size_t)n * n * K));
  if (K) k_model<<<blocks_for(K), TB>>>(n, dq.p, dmu.p, db.p, K);
  if (int err = finish()) return err;
  CK(dmu.down(mu)); CK(db.down(B));
  return 0;
}

}  // extern "C"
