// Token pooling of the finetuning head (mem/modeling_finetune.py:349-354: fc_norm(t[:, 1:, :].mean(1))): the mean of a
// sample's patch-token rows of the fp32 residual stream, cls row skipped, and its backward.  Both are single streaming
// passes that move the byte floor (B*T*D*4 bytes read for B*D*4 written, and the reverse): no workspace, no atomics, a fixed
// summation order, so two runs give the same bits.  The grids are B x (D / 256) and B x (T / 8) workgroups: they fill the
// device at training / evaluation batch sizes; a feature-extraction call with a handful of samples moves a few MB with a
// few workgroups and is bound by launch latency, not bandwidth.
#include "common.h"

namespace {

using namespace memhip;

constexpr int kT = 256;
constexpr int kWaves = kT / 64;

// One workgroup per (sample, slab of 64 * VEC columns).  A wave reads 64 * VEC consecutive floats of ONE row per load
// (VEC = 4: 1 KiB, 16 bytes per lane), the four waves take the token rows t = 1 + w, 5 + w, 9 + w, ... (T is odd in every
// config: nothing is assumed about the row count), four rows in flight per lane.  Per column the order of the sum is fixed:
// the lane's rows in ascending order into four interleaved partial sums, those as (0 + 1) + (2 + 3), then the four waves
// through LDS as (0 + 1) + (2 + 3), then one IEEE division by T - 1.
template <int VEC>
__global__ __launch_bounds__(kT) void pool_tokens_kernel(const float* __restrict__ x, long long ldx, int T, int D,
                                                         float* __restrict__ out) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  __shared__ vec_t sm[kWaves][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + lane) * VEC;          // first column of this lane (D % VEC == 0: a vector is in or out)
  const bool live = c < D;
  const float* base = x + (long long)b * T * ldx + c;
  vec_t a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (live) {
    int t = 1 + wave;
    for (; t + 3 * kWaves < T; t += 4 * kWaves) {
      const vec_t v0 = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(base + (long long)t * ldx));
      const vec_t v1 = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(base + (long long)(t + kWaves) * ldx));
      const vec_t v2 = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(base + (long long)(t + 2 * kWaves) * ldx));
      const vec_t v3 = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(base + (long long)(t + 3 * kWaves) * ldx));
      a0 += v0; a1 += v1; a2 += v2; a3 += v3;
    }
    // (the ragged end: at most three more rows of this wave, into the partial sums in the same rotation)
    if (t < T) a0 += __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(base + (long long)t * ldx));
    if (t + kWaves < T) a1 += __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(base + (long long)(t + kWaves) * ldx));
    if (t + 2 * kWaves < T) a2 += __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(base + (long long)(t + 2 * kWaves) * ldx));
  }
  sm[wave][lane] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (wave == 0 && live) {
    const vec_t s = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
    const float n = (float)(T - 1);
    vec_t r;
#pragma unroll
    for (int k = 0; k < VEC; ++k) r[k] = s[k] / n;
    *reinterpret_cast<vec_t*>(out + (long long)b * D + c) = r;
  }
}

// dx[b*T + t] = dout[b] / (T - 1) for t >= 1, 0 for the cls row.  One workgroup per (sample, chunk of kRows token rows):
// the rows of a chunk are contiguous in dx (leading dimension D), so the chunk is one run of kRows * D floats written with
// 16-byte lane stores; the quotient is formed per store from the L2-resident dout row (IEEE division, as a / n on the host).
constexpr int kRows = 8;

template <int VEC>
__global__ __launch_bounds__(kT) void pool_tokens_bwd_kernel(const float* __restrict__ dout, int T, int D,
                                                             float* __restrict__ dx) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  const int b = blockIdx.y, t0 = blockIdx.x * kRows;
  const int rows = T - t0 < kRows ? T - t0 : kRows;
  const int dv = D / VEC, nq = rows * dv;
  const vec_t* g = reinterpret_cast<const vec_t*>(dout + (long long)b * D);
  vec_t* dst = reinterpret_cast<vec_t*>(dx + ((long long)b * T + t0) * D);
  const float n = (float)(T - 1);
  for (int q = threadIdx.x; q < nq; q += kT) {
    const int r = q / dv, cv = q - r * dv;
    vec_t v = 0.f;
    if (t0 + r > 0) {
      const vec_t gv = g[cv];
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = gv[k] / n;
    }
    dst[q] = v;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int memhip_pool_tokens(const float* x, int64_t ldx, int B, int T, int D, float* out, memhip_stream_t stream) {
  MEMHIP_REQUIRE(B > 0 && T >= 2 && D > 0, "pool_tokens: bad shape B=%d T=%d D=%d (T >= 2: a cls row and a token)", B, T, D);
  MEMHIP_REQUIRE(ldx >= D, "pool_tokens: ldx=%lld < D=%d", (long long)ldx, D);
  MEMHIP_REQUIRE(B <= 65535, "pool_tokens: B=%d > 65535", B);
  MEMHIP_REQUIRE(x && out, "pool_tokens: null pointer");
  const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(x) && aligned16(out);
  if (vec)
    hipLaunchKernelGGL(pool_tokens_kernel<4>, dim3(cdiv(D, 256), B), dim3(kT), 0, as_stream(stream), x, (long long)ldx, T, D, out);
  else
    hipLaunchKernelGGL(pool_tokens_kernel<1>, dim3(cdiv(D, 64), B), dim3(kT), 0, as_stream(stream), x, (long long)ldx, T, D, out);
  return check_launch("pool_tokens");
}

extern "C" int memhip_pool_tokens_bwd(const float* dout, int B, int T, int D, float* dx, memhip_stream_t stream) {
  MEMHIP_REQUIRE(B > 0 && T >= 2 && D > 0, "pool_tokens_bwd: bad shape B=%d T=%d D=%d (T >= 2: a cls row and a token)", B, T, D);
  MEMHIP_REQUIRE(B <= 65535 && (long long)kRows * D < (1ll << 31), "pool_tokens_bwd: B=%d > 65535 or D=%d too large", B, D);
  MEMHIP_REQUIRE(dout && dx, "pool_tokens_bwd: null pointer");
  const bool vec = D % 4 == 0 && aligned16(dout) && aligned16(dx);
  const dim3 grid(cdiv(T, kRows), B);
  if (vec)
    hipLaunchKernelGGL(pool_tokens_bwd_kernel<4>, grid, dim3(kT), 0, as_stream(stream), dout, T, D, dx);
  else
    hipLaunchKernelGGL(pool_tokens_bwd_kernel<1>, grid, dim3(kT), 0, as_stream(stream), dout, T, D, dx);
  return check_launch("pool_tokens_bwd");
}
