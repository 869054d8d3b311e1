// The host side of the PSP head's pyramid pooling (memhip_ppm_pool / _concat_fwd / _concat_bwd_sums / _bwd_apply / _dmap, one
// memhip_ppm_args_t for the five): the validation of a call and its grids and LDS.  Host arithmetic only: memhip_ppm_plan
// runs without a device (tests/test_psp_head_cpu.py).  The constants and the bin arithmetic are read by the kernels
// (ppm.hip) and by the plan alike.
#pragma once
#include "common.h"

namespace memhip {
namespace ppm {

constexpr int kThreads = 256;
constexpr int kChunk = 64;                     // channels per tile: 8 lanes x 16 bytes of bf16
constexpr int kPixels = 64;                    // pixels per tile of _pool, _concat_fwd and _dmap
constexpr int kRows = 32;                      // (sample, bin) rows per tile of the gather and of _bwd_apply: one per 8 lanes
constexpr int kMaxC = 512;
constexpr int kLdsLimit = 64 * 1024;
constexpr int kTileLdsBytes = kPixels * (kChunk + 1) * 4;

// bin i of s over n pixels: [bin_start, bin_end)
__host__ __device__ inline int bin_start(int i, int n, int s) { return (i * n) / s; }
__host__ __device__ inline int bin_end(int i, int n, int s) { return ((i + 1) * n + s - 1) / s; }
// the bins of s over n that hold pixel y: bin_first .. bin_last (at most two when s <= n)
__host__ __device__ inline int bin_first(int y, int n, int s) { return (y * s) / n; }
__host__ __device__ inline int bin_last(int y, int n, int s) { return ((y + 1) * s - 1) / n; }

// _pool: the tile, an fp32 accumulator per (bin, channel of the tile) and the bins' rectangles (4 ints each)
inline int pool_lds_bytes(int bins) { return kTileLdsBytes + bins * (kChunk * 4 + 16); }

}  // namespace ppm

enum { PPM_QUERY, PPM_POOL, PPM_CONCAT, PPM_SUMS, PPM_APPLY, PPM_DMAP };     // who asks: the pointers that must be there
int ppm_plan(const memhip_ppm_args_t* a, int who, memhip_ppm_plan_t* p);

}  // namespace memhip
