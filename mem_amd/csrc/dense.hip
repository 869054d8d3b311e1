// Dense per-block feature maps of the finetuning trunk (mem/semantic_segmentation/backbone/mem.py:439-441:
// x[:, 1:, :].permute(0, 2, 1).reshape(B, -1, Hp, Wp).contiguous(), and its autograd backward): the patch-token rows of the
// fp32 residual stream [B*T, D] as maps [B, D, L] (L = T - 1 = Hp * Wp), and the map gradients added back into the token
// gradient.  Both are batched [L, D] <-> [D, L] transposes, pure data movement at 2 * B * L * D * 4 bytes: one read and one
// write per element (the backward reads dx as well), no workspace, no atomics, every output element has one writer.
//
// One workgroup of 256 threads moves a tile of 64 tokens x 64 features through LDS.  On BOTH global sides a lane moves 16
// bytes and 8 neighbouring lanes one 128-byte line: the token side reads / writes 8 rows x 128 B per wave instruction (a
// row of the stream is D * 4 bytes, D % 64 == 0: a tile row is two whole lines; the cls offset shifts by a whole row), the map
// side 8 feature rows x 128 B (32 consecutive tokens).  The tile is stored [token][feature] with a row pitch of 65 floats,
// and BOTH LDS sides are 4-byte accesses (ds_write_b32 / ds_read_b32: 32 banks, conflicts within a 32-lane half):
//   token side: lane (r = t / 8, c = t % 8) touches tile[r][4 c + k]:  bank (r + 4 c + k) % 32, a half holds 4 rows x 8 c
//   map side:   lane (f = t / 8, q = t % 8) touches tile[4 q + k][f]:  bank (4 q + k + f) % 32, a half holds 4 f x 8 q
// -- 32 distinct banks per half in both, so neither the row-wise nor the column-wise pass conflicts.
// L is ragged against the tile (24, 196, 1200 tokens): token rows >= L are neither read nor written; the map side moves
// 16 bytes per lane when L % 4 == 0 (a vector is wholly inside or outside) and the map buffer is 16-byte aligned, single
// floats otherwise.
#include "common.h"

namespace {

using namespace memhip;

constexpr int kT = 256;
constexpr int kTile = 64;            // tokens and features per tile
constexpr int kPitch = kTile + 1;    // floats per LDS row (see above)

typedef float f4 __attribute__((ext_vector_type(4)));

// out[b, d, l] = x[(b * T + 1 + l) * ldx + d]
template <bool VECL>
__global__ __launch_bounds__(kT) void tokens_to_maps_kernel(const float* __restrict__ x, long long ldx, int b0, int T, int D,
                                                            float* __restrict__ out) {
  __shared__ float tile[kTile * kPitch];
  const int L = T - 1;
  const int t = threadIdx.x, l0 = blockIdx.x * kTile, d0 = blockIdx.y * kTile;
  const long long b = b0 + (long long)blockIdx.z;
  {
    const int r = t >> 3, c = t & 7;
    const float* src = x + (b * T + 1 + l0) * ldx + d0 + 4 * c;
    f4 v[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {                     // h & 1: feature half, h >> 1: token half
      const int l = r + 32 * (h >> 1);
      v[h] = 0.f;
      if (l0 + l < L) v[h] = *reinterpret_cast<const f4*>(src + (long long)l * ldx + 32 * (h & 1));
    }
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      float* dst = tile + (r + 32 * (h >> 1)) * kPitch + 32 * (h & 1) + 4 * c;
#pragma unroll
      for (int k = 0; k < 4; ++k) dst[k] = v[h][k];
    }
  }
  __syncthreads();
  {
    const int f = t >> 3, q = t & 7;
    float* dst = out + (b * D + d0) * L + l0;
#pragma unroll
    for (int h = 0; h < 4; ++h) {                     // h & 1: token half, h >> 1: feature half
      const int d = f + 32 * (h >> 1), l = 4 * q + 32 * (h & 1);
      f4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = tile[(l + k) * kPitch + d];
      float* p = dst + (long long)d * L + l;
      if (VECL) {
        if (l0 + l < L) *reinterpret_cast<f4*>(p) = v;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (l0 + l + k < L) p[k] = v[k];
      }
    }
  }
}

// dx[(b * T + 1 + l) * lddx + d] += dmap[b, d, l]
template <bool VECL>
__global__ __launch_bounds__(kT) void maps_to_tokens_add_kernel(const float* __restrict__ dmap, int b0, int T, int D,
                                                                float* __restrict__ dx, long long lddx) {
  __shared__ float tile[kTile * kPitch];
  const int L = T - 1;
  const int t = threadIdx.x, l0 = blockIdx.x * kTile, d0 = blockIdx.y * kTile;
  const long long b = b0 + (long long)blockIdx.z;
  {
    const int f = t >> 3, q = t & 7;
    const float* src = dmap + (b * D + d0) * L + l0;
    f4 v[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int d = f + 32 * (h >> 1), l = 4 * q + 32 * (h & 1);
      const float* p = src + (long long)d * L + l;
      v[h] = 0.f;
      if (VECL) {
        if (l0 + l < L) v[h] = *reinterpret_cast<const f4*>(p);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (l0 + l + k < L) v[h][k] = p[k];
      }
    }
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int d = f + 32 * (h >> 1), l = 4 * q + 32 * (h & 1);
#pragma unroll
      for (int k = 0; k < 4; ++k) tile[(l + k) * kPitch + d] = v[h][k];
    }
  }
  __syncthreads();
  {
    const int r = t >> 3, c = t & 7;
    float* dst = dx + (b * T + 1 + l0) * lddx + d0 + 4 * c;
    f4 g[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int l = r + 32 * (h >> 1);
      g[h] = 0.f;
      if (l0 + l < L) g[h] = *reinterpret_cast<const f4*>(dst + (long long)l * lddx + 32 * (h & 1));
    }
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int l = r + 32 * (h >> 1);
      const float* s = tile + l * kPitch + 32 * (h & 1) + 4 * c;
      f4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = g[h][k] + s[k];                  // the one fp32 add of the element
      if (l0 + l < L) *reinterpret_cast<f4*>(dst + (long long)l * lddx + 32 * (h & 1)) = v;
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int memhip_tokens_to_maps(const float* x, int64_t ldx, int b0, int b1, int T, int D, float* out,
                                     memhip_stream_t stream) {
  MEMHIP_REQUIRE(T >= 2 && D > 0 && D % kTile == 0,
                 "tokens_to_maps: bad shape T=%d D=%d (T >= 2: a cls row and a token; D a multiple of 64)", T, D);
  MEMHIP_REQUIRE(0 <= b0 && b0 < b1 && b1 - b0 <= 65535, "tokens_to_maps: bad sample range [%d, %d) (at most 65535 samples)", b0, b1);
  MEMHIP_REQUIRE(ldx >= D && ldx % 4 == 0, "tokens_to_maps: ldx=%lld < D=%d or not a multiple of 4", (long long)ldx, D);
  MEMHIP_REQUIRE(D / kTile <= 65535, "tokens_to_maps: D=%d too large", D);
  MEMHIP_REQUIRE(x && out, "tokens_to_maps: null pointer");
  MEMHIP_REQUIRE(aligned16(x), "tokens_to_maps: x is not 16-byte aligned");
  const dim3 grid(cdiv(T - 1, kTile), D / kTile, b1 - b0);
  if ((T - 1) % 4 == 0 && aligned16(out))
    hipLaunchKernelGGL(tokens_to_maps_kernel<true>, grid, dim3(kT), 0, as_stream(stream), x, (long long)ldx, b0, T, D, out);
  else
    hipLaunchKernelGGL(tokens_to_maps_kernel<false>, grid, dim3(kT), 0, as_stream(stream), x, (long long)ldx, b0, T, D, out);
  return check_launch("tokens_to_maps");
}

extern "C" int memhip_maps_to_tokens_add(const float* dmap, int b0, int b1, int T, int D, float* dx, int64_t lddx,
                                         memhip_stream_t stream) {
  MEMHIP_REQUIRE(T >= 2 && D > 0 && D % kTile == 0,
                 "maps_to_tokens_add: bad shape T=%d D=%d (T >= 2: a cls row and a token; D a multiple of 64)", T, D);
  MEMHIP_REQUIRE(0 <= b0 && b0 < b1 && b1 - b0 <= 65535, "maps_to_tokens_add: bad sample range [%d, %d) (at most 65535 samples)", b0, b1);
  MEMHIP_REQUIRE(lddx >= D && lddx % 4 == 0, "maps_to_tokens_add: lddx=%lld < D=%d or not a multiple of 4", (long long)lddx, D);
  MEMHIP_REQUIRE(D / kTile <= 65535, "maps_to_tokens_add: D=%d too large", D);
  MEMHIP_REQUIRE(dmap && dx, "maps_to_tokens_add: null pointer");
  MEMHIP_REQUIRE(aligned16(dx), "maps_to_tokens_add: dx is not 16-byte aligned");
  const dim3 grid(cdiv(T - 1, kTile), D / kTile, b1 - b0);
  if ((T - 1) % 4 == 0 && aligned16(dmap))
    hipLaunchKernelGGL(maps_to_tokens_add_kernel<true>, grid, dim3(kT), 0, as_stream(stream), dmap, b0, T, D, dx, (long long)lddx);
  else
    hipLaunchKernelGGL(maps_to_tokens_add_kernel<false>, grid, dim3(kT), 0, as_stream(stream), dmap, b0, T, D, dx, (long long)lddx);
  return check_launch("maps_to_tokens_add");
}
