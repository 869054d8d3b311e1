// The library's one ordered fold of per-workgroup partials (bn_tile.hpp: FoldOut, launch_fold): stage 2 of the two-stage column
// sums of necks.hip and seg_head.hip.  No float atomics: the G slots are added in ascending order, so two calls give the same bits.
#include "common.h"
#include "bn_tile.hpp"

namespace {

using namespace memhip;
using bn::kT, bn::FoldOut;

__global__ __launch_bounds__(kT) void fold_kernel(const float* __restrict__ ws, int G, int slot, FoldOut o) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i < o.n_count) o.count_out[i] = o.count;
  if (i >= slot) return;
  float s = 0.f;
  int g = 0;
  for (; g + 8 <= G; g += 8) {                       // eight loads in flight, added in the same ascending order
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ws[(long long)(g + j) * slot + i];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  for (; g < G; ++g) s += ws[(long long)g * slot + i];
  int j = i;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    if (j < o.n[q]) { o.p[q][j] = s; return; }
    j -= o.n[q];
  }
}

}  // namespace

void memhip::bn::launch_fold(const float* ws, int G, int slot, int grid, const FoldOut& o, hipStream_t stream) {
  hipLaunchKernelGGL(fold_kernel, dim3(grid), dim3(kT), 0, stream, ws, G, slot, o);
}
