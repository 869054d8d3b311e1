// The convolution weight gradient (conv_wgrad.hip): its geometry, the ONE function that turns (pixel row, channel chunk, grad
// column chunk) into the two element offsets the kernel's LDS-DMA reads, the slicing of the pixel range and the plan.
// wgrad_validate is the one reader of a memhip_conv_wgrad_args_t for the call and the plan query, wgrad_plan the one place that
// decides grid, slices and workspace.  Host arithmetic only; wgrad_gather is shared with the kernel, so the addresses the
// kernel issues can be enumerated and checked on the CPU (tests/wgrad_addr_check.cpp does, for every shape of the GPU tests).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>          // __host__ __device__ (empty for a plain host compile)
#include "../../include/memhip.h"

namespace memhip {

constexpr int kWgTile = 128;          // grad tile: 128 channels of small x 128 columns (ky, kx, c)
constexpr int kWgStageRows = 64;      // pixels per stage
constexpr int kWgThreads = 256;
constexpr int kWgLdsBytes = 2 * 2 * kWgStageRows * kWgTile * 2;      // two stages of two [64][128] bf16 tiles
constexpr int kWgMaxSplits = 256;

struct WgradGeom {
  int B, Hs, Ws, C, N, ksize, stride, pad, small_padded;
  int Hbp, Wbp;                       // padded size of big: stride * Hs + 2, stride * Ws + 2
  int K;                              // ksize * ksize * C
  int64_t M;                          // B * Hs * Ws
};

inline WgradGeom wgrad_geom(const memhip_conv_wgrad_args_t& a) {
  WgradGeom g;
  g.B = a.B; g.Hs = a.Hs; g.Ws = a.Ws; g.C = a.C; g.N = a.N; g.ksize = a.ksize; g.stride = a.stride; g.pad = a.pad;
  g.small_padded = a.small_padded;
  g.Hbp = a.stride * a.Hs + 2; g.Wbp = a.stride * a.Ws + 2;
  g.K = a.ksize * a.ksize * a.C;
  g.M = (int64_t)a.B * a.Hs * a.Ws;
  return g;
}

// Element offsets of the two 16-byte chunks (8 bf16) that pixel row m = (b, y, x) contributes: channels n .. n+7 of small, and
// grad columns col .. col+7 of big, col = (ky * ksize + kx) * C + c.  0 <= m < M, n % 8 == 0 < N, col % 8 == 0 < K.
// C % 8 == 0: the chunk lies inside one tap.  C == 4 (4x4, stride 2): the chunk is taps kx, kx+1 (kx even) of one ky, i.e. two
// neighbouring pixels x 4 channels, contiguous, and 16-byte aligned because Wbp and kx are even.
struct WgradAddr { int64_t small, big; };
__host__ __device__ inline WgradAddr wgrad_gather(const WgradGeom& g, int m, int n, int col) {
  const int hw = g.Hs * g.Ws;
  const int b = m / hw, r = m - b * hw;
  const int y = r / g.Ws, x = r - y * g.Ws;
  const int tap = col / g.C, c = col - tap * g.C;
  const int ky = tap / g.ksize, kx = tap - ky * g.ksize;
  WgradAddr a;
  a.small = g.small_padded ? (((int64_t)b * (g.Hs + 2) + y + 1) * (g.Ws + 2) + x + 1) * g.N + n : (int64_t)m * g.N + n;
  a.big = (((int64_t)b * g.Hbp + g.stride * y + ky + 1 - g.pad) * g.Wbp + g.stride * x + kx + 1 - g.pad) * g.C + c;
  return a;
}

// `wanted` slices of M > 0 rows in whole stages, at least 4 stages each; no slice is empty.
struct WgradSlices { int rows_per_split, splits; };
inline WgradSlices wgrad_slices(int64_t M, int wanted) {
  const int64_t stages = (M + kWgStageRows - 1) / kWgStageRows;
  int64_t s = wanted > kWgMaxSplits ? kWgMaxSplits : wanted;
  if (s > stages / 4) s = stages / 4;
  if (s < 1) s = 1;
  const int64_t rows = (stages + s - 1) / s * kWgStageRows;
  return {(int)rows, (int)((M + rows - 1) / rows)};
}

typedef memhip_conv_wgrad_plan_t WgradPlan;

// query: the pointers may be null and unaligned, the workspace of any size (the query dereferences nothing).
int wgrad_validate(const memhip_conv_wgrad_args_t* a, bool query, WgradGeom* g);
// tiles x slices fill the 2 x device_cus workgroup slots of the device once (two workgroups fit a CU), never more; a geometry
// wgrad_validate accepted.
WgradPlan wgrad_plan(const WgradGeom& g, int device_cus);

}  // namespace memhip
