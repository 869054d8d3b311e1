// The device pieces of a conv -> SyncBN -> activation block that necks.hip and seg_head.hip share: a tile of 64 rows (pixels)
// x 64 channels through one padded fp32 LDS tile (pitch 65 floats, 4-byte LDS accesses), 256 threads, and two-stage column
// sums without atomics.
//
//   map_side   fp32 maps [B, C, P]: lane (q = t % 16, channel t / 16 + 16 k) takes the rows z0 + 4 q .. + 3 of one channel,
//              16 bytes when P % 4 == 0 (VEC), single floats otherwise
//   row_side   bf16 rows of C channels: lane (row t / 8 + 32 k, channels 8 (t % 8)..) moves 16 bytes, 8 neighbouring lanes
//              the 128 bytes of a tile row; where a row lies is the caller's functor (plain rows: z * C)
//   sums       stage 1 is the caller's kernel: a grid of G x C / 64 workgroups, each thread a fixed-order chain over its rows;
//              fold_rows_and_store folds the workgroup's row lanes in LDS in ascending order and stores one partial per
//              workgroup plainly to the workspace, slot [.., which * C + channel]; stage 2, launch_fold, adds the G slots in
//              ascending order (one kernel for the whole library, fold.hip).  Bit-reproducible.
// Rows past the end (ragged last tile) are neither read nor written; C % 64 == 0, so channel tiles are whole.
#pragma once
#include "common.h"

namespace memhip {
namespace bn {

constexpr int kT = 256;
constexpr int kTile = 64;            // rows and channels per tile
constexpr int kPitch = kTile + 1;    // floats per LDS row
static_assert(MEMHIP_NECK_GROUPS == MEMHIP_BN_GROUPS, "one two-stage sum: the most partials per output are the same everywhere");
constexpr int kGroups = MEMHIP_BN_GROUPS;

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef unsigned short us8 __attribute__((ext_vector_type(8)));
typedef unsigned short bf16_t;       // storage

__device__ __forceinline__ float bf2f(bf16_t u) { return __uint_as_float((unsigned)u << 16); }
__device__ __forceinline__ bf16_t f2bf(float v) { return __builtin_bit_cast(bf16_t, (__bf16)v); }   // round to nearest even

struct BnParams {
  const float* mean; const float* rstd; const float* gamma; const float* beta;
};

inline bool aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(n - 1)) == 0; }

inline int check_bn(const char* what, const float* mean, const float* rstd, const float* gamma, const float* beta) {
  MEMHIP_REQUIRE(mean && rstd && gamma && beta, "%s: null pointer (mean, rstd, gamma, beta)", what);
  return MEMHIP_OK;
}

// ---------------------------------------------------------------- M side: fp32 maps [B, C, P], R = B * P rows
// LOAD: map -> tile, else tile -> map
template <bool VEC, bool LOAD>
__device__ __forceinline__ void map_side(std::conditional_t<LOAD, const float, float>* __restrict__ map, int C, int P, long long R,
                                         long long z0, int c0, std::conditional_t<LOAD, float, const float>* tile) {
  const int t = threadIdx.x, q = t & 15;
  const long long z = z0 + 4 * q;                                    // element e: row z + e
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cl = (t >> 4) + 16 * k;
    if constexpr (VEC) {                                             // P % 4 == 0: the four pixels lie in one sample
      const bool ok = z < R;
      auto* ptr = map + ((z / P) * C + c0 + cl) * P + z % P;
      if constexpr (LOAD) {
        f4 v = 0.f;
        if (ok) v = *reinterpret_cast<const f4*>(ptr);
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[(4 * q + e) * kPitch + cl] = v[e];
      } else {
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tile[(4 * q + e) * kPitch + cl];
        if (ok) *reinterpret_cast<f4*>(ptr) = v;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long ze = z + e;
        const bool ok = ze < R;
        auto* ptr = map + ((ze / P) * C + c0 + cl) * P + ze % P;
        if constexpr (LOAD) {
          tile[(4 * q + e) * kPitch + cl] = ok ? *ptr : 0.f;
        } else {
          if (ok) *ptr = tile[(4 * q + e) * kPitch + cl];
        }
      }
    }
  }
}

// ---------------------------------------------------------------- bf16 rows: off(z) = element offset of channel 0 of row z
struct PlainRows {
  int C;
  __device__ __forceinline__ long long operator()(long long z) const { return z * C; }
};

// LOAD: rows -> tile (zero past the end; both 16-byte loads are issued before the conversions), else tile -> rows
template <bool LOAD, typename Off>
__device__ __forceinline__ void row_side(std::conditional_t<LOAD, const bf16_t, bf16_t>* __restrict__ rows, long long nz,
                                         const Off& off, long long z0, int c0, std::conditional_t<LOAD, float, const float>* tile) {
  const int t = threadIdx.x, c = 8 * (t & 7);
  if constexpr (LOAD) {
    us8 v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int zl = (t >> 3) + 32 * h;
      v[h] = 0;
      if (z0 + zl < nz) v[h] = *reinterpret_cast<const us8*>(rows + off(z0 + zl) + c0 + c);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float* dst = tile + ((t >> 3) + 32 * h) * kPitch + c;
#pragma unroll
      for (int e = 0; e < 8; ++e) dst[e] = bf2f(v[h][e]);
    }
  } else {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int zl = (t >> 3) + 32 * h;
      const bool ok = z0 + zl < nz;
      bf16_t* ptr = rows + (ok ? off(z0 + zl) : 0) + c0 + c;
      const float* src = tile + zl * kPitch + c;
      us8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = f2bf(src[e]);
      if (ok) *reinterpret_cast<us8*>(ptr) = v;
    }
  }
}

// ---------------------------------------------------------------- two-stage column sums
// stage 1 tail: the workgroup's ROW_LANES row lanes (t / (64 / CH)) hold two sums for each of their CH channels (CH (t % (64 /
// CH)) ..): fold them in ascending order and store the workgroup's partial ws_slot[which * C + c0 + channel].
// red: 2 * ROW_LANES * 64 floats, red[which][lane][64]
template <int ROW_LANES, int CH>
__device__ __forceinline__ void fold_rows_and_store(const float (&a1)[CH], const float (&a2)[CH], float* red,
                                                    float* __restrict__ ws_slot, int C, int c0) {
  static_assert(ROW_LANES * (kTile / CH) == kT, "256 threads: row lanes x channel lanes");
  const int t = threadIdx.x, c = CH * (t % (kTile / CH)), j = t / (kTile / CH);
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    red[j * 64 + c + e] = a1[e];
    red[ROW_LANES * 64 + j * 64 + c + e] = a2[e];
  }
  __syncthreads();
  if (t < 128) {
    const int which = t >> 6, cc = t & 63;
    float s = red[which * ROW_LANES * 64 + cc];
#pragma unroll
    for (int k = 1; k < ROW_LANES; ++k) s += red[which * ROW_LANES * 64 + k * 64 + cc];
    ws_slot[which * C + c0 + cc] = s;
  }
}

// stage 2: s[i] = sum over g < G of ws[g * slot + i], in ascending order, i < slot; the slot is cut into up to three outputs;
// count_out[i] = count for i < n_count (n_count <= slot)
struct FoldOut {
  float* p[3];
  int n[3];
  float* count_out;
  int n_count;
  float count;
};
inline int fold_grid(int slot) { return cdiv(slot, kT); }           // one thread per output
// grid: fold_grid(slot), or the caller's plan's figure for it (fold.hip)
void launch_fold(const float* ws, int G, int slot, int grid, const FoldOut& o, hipStream_t stream);

}  // namespace bn
}  // namespace memhip
