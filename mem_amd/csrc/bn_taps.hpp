// The device pieces ppm.hip and fpn.hip share on the padded activation format bf16 [B, m+2, m'+2, channels]: where a pixel
// lies, the batch-norm vectors of 8 channels, xhat and u of 8 channels of a stored convolution output, the weight with which
// a bilinear output reads an input (memhip_seg_axis_table's tables), and the four-tap combination.  A thread owns 8 channels
// (16 bytes of bf16) of one pixel.
#pragma once
#include "bn_tile.hpp"

namespace memhip {
namespace bn {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// element offset of channel 0 of pixel (b, y, x) in a padded buffer of m x m' pixels and `pitch` channels
__device__ __forceinline__ long long pad_at(long long b, int y, int x, int m, int mm, int pitch) {
  return ((b * (m + 2) + y + 1) * (mm + 2) + x + 1) * pitch;
}

// the weight with which output (i0, i1 = min(i0 + 1, n - 1), w1) reads input i (seg_loss.hip)
__device__ __forceinline__ float weight_of(int i, int i0, int i1, float w1) {
  return (i0 == i ? 1.f - w1 : 0.f) + (i1 == i ? w1 : 0.f);
}

struct Chan8 { float m[8], rs[8], ga[8], be[8]; };

__device__ __forceinline__ void load8(const float* __restrict__ p, float (&o)[8]) {
  const f4 a = *reinterpret_cast<const f4*>(p), b = *reinterpret_cast<const f4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { o[e] = a[e]; o[4 + e] = b[e]; }
}

// the vectors of channels c .. c + 7 of row i of [rows, C] vectors
__device__ __forceinline__ Chan8 chan8(const BnParams& v, int i, int C, int c) {
  Chan8 k;
  const int o = i * C + c;
  load8(v.mean + o, k.m); load8(v.rstd + o, k.rs); load8(v.gamma + o, k.ga); load8(v.beta + o, k.be);
  return k;
}

// xhat, u = gamma xhat + beta of 8 channels of one pixel
__device__ __forceinline__ void bn8(const us8& v, const Chan8& k, float (&xh)[8], float (&u)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    xh[e] = (bf2f(v[e]) - k.m[e]) * k.rs[e];
    u[e] = fmaf(xh[e], k.ga[e], k.be[e]);
  }
}

// one axis of a bilinear output: the two inputs it reads and their weights
struct Tap { int i0, i1; float w0, w1; };
__device__ __forceinline__ Tap tap_of(const int* __restrict__ i0, const float* __restrict__ w1, int o, int n) {
  Tap t;
  t.i0 = clampi(i0[o], 0, n - 1);
  t.i1 = min(t.i0 + 1, n - 1);
  t.w1 = w1[o];
  t.w0 = 1.f - t.w1;
  return t;
}

// w0y (w0x a + w1x b) + w1y (w0x c + w1x d)
__device__ __forceinline__ float bilerp(const Tap& ty, const Tap& tx, float a, float b, float c, float d) {
  return ty.w0 * (tx.w0 * a + tx.w1 * b) + ty.w1 * (tx.w0 * c + tx.w1 * d);
}

}  // namespace bn
}  // namespace memhip
