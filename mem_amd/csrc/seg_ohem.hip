// memhip_seg_ohem_select: the OHEM sampler's threshold from the stored key map, exactly and on the device.
//
// A key counts when it is >= 0.0f (memhip_seg_ohem_keys stores -1.0f elsewhere; a NaN does not count, -0.0f is 0.0f).  Such
// floats order like their bit patterns, so the element of ascending rank r is found by a radix select on the 31 value bits,
// 11 / 11 / 10 bits of the 32-bit word at a time.  (Bit 31 of a key that counts is zero, so the first pass separates 10 value bits
// and only the lower 1024 of its 2048 bins can be hit: 10 / 11 / 10 of the 31 value bits.  No bit is missing.)
//   sel_hist_kernel<pass>  every workgroup strides over the keys, counts those that match the prefix found so far into a
//                          histogram in LDS and flushes the nonzero bins with 64-bit integer atomics (integer sums do not
//                          depend on the order of arrival)
//   sel_scan_kernel<pass>  one workgroup: after pass 0 it has n and derives r (sampler 1: min(K, n - 1); sampler 2: n - min(K, n));
//                          it finds the bin that holds rank r, extends the prefix and makes r relative to the bin; after the
//                          last pass the prefix is the key itself and *threshold is written
//   sel_count_kernel       n_kept = the keys that count and pass the comparison with *threshold, an integer per workgroup
//                          added to the state; the last workgroup to arrive publishes the sum to stats[3]
// The histograms and the state live in the caller's workspace and are cleared on the stream by the call itself.
#include "common.h"
#include "seg_plan.hpp"

namespace {

using namespace memhip;
using namespace memhip::seg;

// pass p looks at bits shift_of(p) .. shift_of(p) + 10 (the last pass: 0 .. 9); the prefix before it is u >> shift_of(p - 1)
__host__ __device__ constexpr int shift_of(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__host__ __device__ constexpr uint32_t mask_of(int pass) { return pass == 2 ? 0x3ffu : 0x7ffu; }

// the value bits of a key that counts; false for the others
__device__ __forceinline__ bool key_bits(float k, uint32_t* u) {
  *u = __float_as_uint(k) & 0x7fffffffu;
  return k >= 0.f;
}

template <int PASS>
__global__ __launch_bounds__(kSelThreads) void sel_hist_kernel(const float* __restrict__ keys, long long total,
                                                               unsigned long long* __restrict__ hist, const SelState* __restrict__ st) {
  __shared__ int bins[kSelBins];
  const int t = threadIdx.x;
  for (int e = t; e < kSelBins; e += kSelThreads) bins[e] = 0;
  uint32_t prefix = 0;
  if constexpr (PASS > 0) {
    if (st->none) return;                                     // nothing to find: the whole workgroup leaves
    prefix = st->prefix;
  }
  __syncthreads();
  // a workgroup sees at most total / gridDim.x + kSelThreads < 2^31 keys (total <= 2^36, 1024 workgroups beyond 2^18 keys)
  for (long long n = (long long)blockIdx.x * kSelThreads + t; n < total; n += (long long)gridDim.x * kSelThreads) {
    uint32_t u;
    if (!key_bits(keys[n], &u)) continue;
    if constexpr (PASS > 0) {
      if ((u >> shift_of(PASS - 1)) != prefix) continue;
    }
    atomicAdd(&bins[(u >> shift_of(PASS)) & mask_of(PASS)], 1);
  }
  __syncthreads();
  unsigned long long* out = hist + PASS * kSelBins;
  for (int e = t; e < kSelBins; e += kSelThreads)
    if (bins[e]) atomicAdd(out + e, (unsigned long long)bins[e]);
}

template <int PASS>
__global__ __launch_bounds__(kSelThreads) void sel_scan_kernel(const unsigned long long* __restrict__ hist, SelState* __restrict__ st,
                                                               int sampler, long long K, float T, float* __restrict__ threshold) {
  constexpr int kPer = kSelBins / kSelThreads;                // consecutive bins per thread
  __shared__ unsigned long long part[kSelThreads];
  __shared__ unsigned long long s_r;
  const int t = threadIdx.x;
  if constexpr (PASS > 0) {
    if (st->none) return;
  }
  const unsigned long long* h = hist + PASS * kSelBins;
  unsigned long long mine[kPer], sum = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) { mine[e] = h[t * kPer + e]; sum += mine[e]; }
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    unsigned long long run = 0;
    for (int e = 0; e < kSelThreads; ++e) { const unsigned long long v = part[e]; part[e] = run; run += v; }   // exclusive
    unsigned long long r = 0;
    if (PASS == 0) {
      const unsigned long long n = run, k = (unsigned long long)K;
      st->n = n;
      const bool none = n == 0 || (sampler == 2 && k == 0);
      st->none = none ? 1u : 0u;
      if (none) {
        *threshold = sampler == 1 ? -INFINITY : INFINITY;     // key < -inf and key >= +inf hold for no key
      } else {
        r = sampler == 1 ? (k < n - 1 ? k : n - 1) : n - (k < n ? k : n);
      }
      s_r = none ? ~0ull : r;
    } else {
      s_r = st->r;
    }
  }
  __syncthreads();
  const unsigned long long r = s_r;
  if (r == ~0ull) return;
  // the one bin with below <= r < below + count
  unsigned long long below = part[t];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    if (mine[e] != 0 && r >= below && r < below + mine[e]) {
      uint32_t prefix = (uint32_t)(t * kPer + e);
      if constexpr (PASS > 0) prefix |= st->prefix << (shift_of(PASS - 1) - shift_of(PASS));
      st->prefix = prefix;
      st->r = r - below;
      if (PASS == kSelPasses - 1) {
        const float a = __uint_as_float(prefix);              // the key of rank r
        *threshold = sampler == 1 ? (a > T ? a : T) : a;
      }
    }
    below += mine[e];
  }
}

__global__ __launch_bounds__(kSelThreads) void sel_count_kernel(const float* __restrict__ keys, long long total, int sampler,
                                                                const float* __restrict__ threshold, SelState* __restrict__ st,
                                                                unsigned int* __restrict__ arrived, long long* __restrict__ n_kept) {
  __shared__ unsigned long long red[kSelThreads];
  const int t = threadIdx.x;
  const float thr = *threshold;
  unsigned long long c = 0;
  for (long long n = (long long)blockIdx.x * kSelThreads + t; n < total; n += (long long)gridDim.x * kSelThreads) {
    const float k = keys[n];
    c += k >= 0.f && (sampler == 1 ? k < thr : k >= thr);     // memhip_seg_ce_w's comparison
  }
  red[t] = c;
  __syncthreads();
  for (int s = kSelThreads / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) {
    if (red[0]) atomicAdd(&st->kept, red[0]);
    __threadfence();
    if (atomicAdd(arrived, 1u) == gridDim.x - 1) {            // the last to arrive: every sum above is visible
      __threadfence();
      *n_kept = (long long)atomicAdd(&st->kept, 0ull);
    }
  }
}

}  // namespace

extern "C" int memhip_seg_ohem_select(const memhip_segohem_args_t* a, memhip_stream_t stream) {
  memhip_segohem_plan_t p;
  if (int rc = seg_ohem_plan(a, OHEM_SELECT, &p)) return rc;
  hipStream_t s = as_stream(stream);
  unsigned char* base = static_cast<unsigned char*>(a->seg.workspace) + p.select_ws_offset;
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(base);
  SelState* st = reinterpret_cast<SelState*>(base + (size_t)kSelPasses * kSelBins * 8);
  const long long total = (long long)a->seg.B * a->seg.H * a->seg.W;
  const long long K = a->min_kept * (long long)a->seg.B;
  const dim3 grid(p.select_grid), block(p.select_block);
  MEMHIP_HIP(hipMemsetAsync(base, 0, p.select_ws_bytes, s));
  hipLaunchKernelGGL(sel_hist_kernel<0>, grid, block, 0, s, a->keys, total, hist, st);
  hipLaunchKernelGGL(sel_scan_kernel<0>, dim3(1), block, 0, s, hist, st, a->sampler, K, a->thresh, a->threshold);
  hipLaunchKernelGGL(sel_hist_kernel<1>, grid, block, 0, s, a->keys, total, hist, st);
  hipLaunchKernelGGL(sel_scan_kernel<1>, dim3(1), block, 0, s, hist, st, a->sampler, K, a->thresh, a->threshold);
  hipLaunchKernelGGL(sel_hist_kernel<2>, grid, block, 0, s, a->keys, total, hist, st);
  hipLaunchKernelGGL(sel_scan_kernel<2>, dim3(1), block, 0, s, hist, st, a->sampler, K, a->thresh, a->threshold);
  hipLaunchKernelGGL(sel_count_kernel, grid, block, 0, s, a->keys, total, a->sampler, a->threshold, st, &st->arrived,
                     reinterpret_cast<long long*>(a->seg.stats) + 3);
  return check_launch("seg_ohem_select");
}
