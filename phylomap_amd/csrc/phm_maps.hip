// phm_maps.hip -- segment counts -> replica-major exclusive offsets of the stochastic maps.
//
// The counts come as [edge][replica] (a wave's 64 replicas side by side) while rows are [replica][edge], so the scan reads
// transposed.  Three launches over chunks of MAPS_CH edges:
//  1. one thread per (replica, chunk) sums its chunk (reads coalesced along the replicas);
//  2. one workgroup scans the replica totals in blocks of 1 024 replicas and gives every (replica, chunk) its base;
//  3. one workgroup per (64 replicas, chunk) moves 64 x 64 count tiles through LDS, one lane per replica runs the prefix along
//     the edges, and the offsets go out along the edges of each replica (coalesced).
#include "phm_maps.h"

namespace phm {

namespace {

constexpr int MAPS_CH = 256;             // edges per chunk
constexpr int MAPS_SCAN = 1024;          // threads of the scan workgroup

__global__ __launch_bounds__(256) void maps_chunk_kernel(const uint16_t* __restrict__ cnt, int R, int E, int pad,
                                                         uint32_t* __restrict__ csum) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (r >= R) return;
  const int b0 = c * MAPS_CH, b1 = min(b0 + MAPS_CH, E);
  uint32_t s = 0;
  for (int b = b0; b < b1; ++b) s += cnt[(size_t)b * pad + r];
  csum[(size_t)c * R + r] = s;
}

__global__ __launch_bounds__(MAPS_SCAN) void maps_scan_kernel(const uint32_t* __restrict__ csum, int R, int E, int nch,
                                                              int64_t* __restrict__ cbase, int64_t* __restrict__ off) {
  __shared__ int64_t s_a[MAPS_SCAN], s_b[MAPS_SCAN];
  const int t = threadIdx.x;
  int64_t run = 0;
  for (int r0 = 0; r0 < R; r0 += MAPS_SCAN) {
    const int r = r0 + t;
    int64_t tot = 0;
    if (r < R)
      for (int c = 0; c < nch; ++c) tot += csum[(size_t)c * R + r];
    s_a[t] = tot;
    __syncthreads();
    int64_t* src = s_a;
    int64_t* dst = s_b;
    for (int d = 1; d < MAPS_SCAN; d <<= 1) {                      // inclusive scan, double-buffered
      dst[t] = src[t] + (t >= d ? src[t - d] : 0);
      __syncthreads();
      int64_t* x = src; src = dst; dst = x;
    }
    int64_t base = run + src[t] - tot;                              // exclusive
    if (r < R)
      for (int c = 0; c < nch; ++c) { cbase[(size_t)c * R + r] = base; base += csum[(size_t)c * R + r]; }
    run += src[MAPS_SCAN - 1];
    __syncthreads();                                                // src is rewritten by the next block of replicas
  }
  if (t == 0) off[(size_t)R * E] = run;
}

__global__ __launch_bounds__(256) void maps_fill_kernel(const uint16_t* __restrict__ cnt, int R, int E, int pad,
                                                        const int64_t* __restrict__ cbase, int64_t* __restrict__ off) {
  __shared__ uint16_t s_c[64][64];                                  // [edge][replica]
  __shared__ int64_t s_o[64][65];                                   // [replica][edge], padded against bank conflicts
  const int r0 = blockIdx.x * 64, c = blockIdx.y;
  const int t = threadIdx.x;
  int64_t run = 0;
  if (t < 64 && r0 + t < R) run = cbase[(size_t)c * R + r0 + t];
  const int b_end = min((c + 1) * MAPS_CH, E);
  for (int b0 = c * MAPS_CH; b0 < b_end; b0 += 64) {
    for (int i = t; i < 64 * 64; i += 256) {
      const int e = i >> 6, j = i & 63;
      s_c[e][j] = (b0 + e < E && r0 + j < R) ? cnt[(size_t)(b0 + e) * pad + r0 + j] : (uint16_t)0;
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll 8
      for (int e = 0; e < 64; ++e) { s_o[t][e] = run; run += s_c[e][t]; }
    }
    __syncthreads();
    for (int i = t; i < 64 * 64; i += 256) {
      const int j = i >> 6, e = i & 63;
      if (r0 + j < R && b0 + e < E) off[(size_t)(r0 + j) * E + b0 + e] = s_o[j][e];
    }
    __syncthreads();
  }
}

}  // namespace

size_t maps_offsets_work_bytes(int R, int E) {
  const size_t nch = (size_t)(E + MAPS_CH - 1) / MAPS_CH;
  return nch * (size_t)R * (sizeof(uint32_t) + sizeof(int64_t)) + 16;
}

hipError_t launch_maps_offsets(const uint16_t* cnt, int R, int E, int pad, int64_t* off, void* work, hipStream_t stream) {
  if (R <= 0 || E <= 0) return hipMemsetAsync(off, 0, sizeof(int64_t), stream);
  const int nch = (E + MAPS_CH - 1) / MAPS_CH;
  int64_t* cbase = static_cast<int64_t*>(work);
  uint32_t* csum = reinterpret_cast<uint32_t*>(cbase + (size_t)nch * R);
  hipLaunchKernelGGL(maps_chunk_kernel, dim3((R + 255) / 256, nch), dim3(256), 0, stream, cnt, R, E, pad, csum);
  hipLaunchKernelGGL(maps_scan_kernel, dim3(1), dim3(MAPS_SCAN), 0, stream, csum, R, E, nch, cbase, off);
  hipLaunchKernelGGL(maps_fill_kernel, dim3((R + 63) / 64, nch), dim3(256), 0, stream, cnt, R, E, pad, cbase, off);
  return hipGetLastError();
}

}  // namespace phm
