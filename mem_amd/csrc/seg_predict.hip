// The end of a segmentation model at test time (mmseg 0.30 EncoderDecoder: slide_inference / whole_inference -> inference ->
// aug_test -> argmax) from the logits of V views, without the upsampled tensors: torch materialises one [B, C, H, W] fp32
// tensor per window and per flip, this kernel none.
//
// A workgroup owns a tile of 16 x 64 output pixels of one sample; a thread walks 4 consecutive x of one row, one after the
// other, so that the C running sums of one pixel (and, with two passes, the C probabilities) are all it holds in registers;
// the four labels leave as one dword where pred's rows allow it.  Per pass a thread walks the views in the order of the
// rectangles (kernel arguments: the walk is scalar).  Whether a view covers a pixel is decided for the whole tile where
// the tile lies inside or outside the rectangle -- the same branch in every lane -- and per pixel only where a window edge
// cuts the tile.  The pass with flip = 1 is read at the mirrored column.  Logits and tables are read through the cache: a
// window's logits are a few hundred KiB and every one is read by (H / h) (W / w) outputs.  Table indices are clamped before
// they address anything.  The confusion histogram of a workgroup lives in LDS and is flushed with 64-bit integer atomics.
#include "common.h"
#include "seg_plan.hpp"
#include "seg_predict_plan.hpp"

namespace {

using namespace memhip;
using namespace memhip::segp;
using memhip::seg::kMaxC;

struct PredK {
  const float* logits; long long sv, sb, sc, sy, sx;
  const int* y_i0; const float* y_w1; const int* x_i0; const float* x_w1;
  uint8_t* pred; float* prob; const uint8_t* labels; unsigned long long* conf;
  int V, C, h, w, hc, wc, H, W, ignore, tiles_y, tiles_x, passes, pred_dwords;
  int rect[kMaxViews][3];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// L[c] = the mean over the views of pass f that hold (y, xs) of the bilinear logit there; xs and TX0 .. TX1 (the tile's
// columns) are in the coordinates of pass f
template <int CP>
__device__ __forceinline__ void pass_logits(const PredK& k, int f, int b, int y, int xs, int Y0, int Y1, int TX0, int TX1,
                                            float (&L)[CP]) {
  const int C = k.C;
#pragma unroll
  for (int c = 0; c < CP; ++c) L[c] = 0.f;
  int n = 0;
  for (int v = 0; v < k.V; ++v) {
    const int ry = k.rect[v][0], rx = k.rect[v][1];
    if (k.rect[v][2] != f) continue;
    if (ry > Y1 || ry + k.hc <= Y0 || rx > TX1 || rx + k.wc <= TX0) continue;          // the tile lies outside: no lane reads it
    const bool whole = ry <= Y0 && ry + k.hc > Y1 && rx <= TX0 && rx + k.wc > TX1;     // the tile lies inside: every lane does
    if (!whole && !(y >= ry && y < ry + k.hc && xs >= rx && xs < rx + k.wc)) continue;
    const int ly = y - ry, lx = xs - rx;
    const int a0 = clampi(k.y_i0[ly], 0, k.h - 1), a1 = min(a0 + 1, k.h - 1);
    const int b0 = clampi(k.x_i0[lx], 0, k.w - 1), b1 = min(b0 + 1, k.w - 1);
    const float wy1 = k.y_w1[ly], wy0 = 1.f - wy1, wx1 = k.x_w1[lx], wx0 = 1.f - wx1;
    const float* src = k.logits + v * k.sv + b * k.sb;
    const float* p00 = src + a0 * k.sy + b0 * k.sx;
    const float* p01 = src + a0 * k.sy + b1 * k.sx;
    const float* p10 = src + a1 * k.sy + b0 * k.sx;
    const float* p11 = src + a1 * k.sy + b1 * k.sx;
#pragma unroll
    for (int c = 0; c < CP; ++c)
      if (c < C) {
        const long long o = c * k.sc;
        const float z = wy0 * (wx0 * p00[o] + wx1 * p01[o]) + wy1 * (wx0 * p10[o] + wx1 * p11[o]);
        L[c] += z;
      }
    n += 1;
  }
  if (n > 1) {                                               // preds / count_mat; a count of 1 divides by 1
    const float cnt = (float)n;
#pragma unroll
    for (int c = 0; c < CP; ++c) L[c] = L[c] / cnt;
  }
#pragma unroll
  for (int c = 0; c < CP; ++c)
    if (c >= C) L[c] = -INFINITY;
}

// in place: L -> softmax(L), the maximum subtracted; padded classes (-inf) give 0
template <int CP>
__device__ __forceinline__ void softmax(float (&L)[CP]) {
  float mx = L[0];
#pragma unroll
  for (int c = 1; c < CP; ++c) mx = fmaxf(mx, L[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    L[c] = expf(L[c] - mx);
    s += L[c];
  }
#pragma unroll
  for (int c = 0; c < CP; ++c) L[c] = L[c] / s;
}

template <int CP>
__device__ __forceinline__ int argmax(const float (&L)[CP]) {
  float mx = L[0];
  int am = 0;
#pragma unroll
  for (int c = 1; c < CP; ++c)
    if (L[c] > mx) { mx = L[c]; am = c; }                   // strictly greater: ties to the lowest class
  return am;
}

template <int CP>
__global__ __launch_bounds__(kThreads) void seg_predict_kernel(PredK k) {
  __shared__ int hist[kMaxC * kMaxC];
  const int t = threadIdx.x, C = k.C, H = k.H, W = k.W;
  const bool count = k.conf != nullptr;
  if (count) {
    for (int e = t; e < C * C; e += kThreads) hist[e] = 0;
    __syncthreads();
  }
  int wg = blockIdx.x;
  const int tx = wg % k.tiles_x; wg /= k.tiles_x;
  const int ty = wg % k.tiles_y;
  const int b = wg / k.tiles_y;
  const int Y0 = ty * kTileH, X0 = tx * kTileW;
  const int Y1 = min(Y0 + kTileH, H) - 1, X1 = min(X0 + kTileW, W) - 1;
  const int MX0 = W - 1 - X1, MX1 = W - 1 - X0;              // the tile's columns in the flipped pass
  const int y = Y0 + t / kLanesX, xq = X0 + (t % kLanesX) * kPx;
  const bool two = k.passes == 3;
  const int first = k.passes == 2 ? 1 : 0;                   // the only pass, or the first of two
  const long long HW = (long long)H * W;
  const long long row = (long long)b * HW + (long long)y * W;

  if (y <= Y1 && xq <= X1) {
    const int npx = min(kPx, X1 - xq + 1);
    uint32_t packed = 0;
#pragma unroll 1
    for (int p = 0; p < npx; ++p) {
      const int x = xq + p;
      float P[CP];
      int am;
      pass_logits<CP>(k, first, b, y, first ? W - 1 - x : x, Y0, Y1, first ? MX0 : X0, first ? MX1 : X1, P);
      if (two) {
        float Q[CP];
        softmax<CP>(P);
        pass_logits<CP>(k, 1, b, y, W - 1 - x, Y0, Y1, MX0, MX1, Q);
        softmax<CP>(Q);
#pragma unroll
        for (int c = 0; c < CP; ++c) P[c] = (P[c] + Q[c]) * 0.5f;      // seg_logit /= 2
        am = argmax<CP>(P);
      } else {
        am = argmax<CP>(P);
        if (k.prob) softmax<CP>(P);
      }
      if (k.prob) {
        float* out = k.prob + (long long)b * C * HW + (long long)y * W + x;
#pragma unroll
        for (int c = 0; c < CP; ++c)
          if (c < C) out[c * HW] = P[c];
      }
      if (count) {
        const int lab = k.labels[row + x];
        if (lab != k.ignore && lab < C) atomicAdd(&hist[lab * C + am], 1);
      }
      packed |= (uint32_t)am << (8 * p);
    }
    if (k.pred) {
      uint8_t* out = k.pred + row + xq;
      if (k.pred_dwords && npx == kPx) {
        *reinterpret_cast<uint32_t*>(out) = packed;           // W % 4 == 0, xq % 4 == 0, pred 4-byte aligned
      } else {
        for (int p = 0; p < npx; ++p) out[p] = (uint8_t)(packed >> (8 * p));
      }
    }
  }
  if (count) {
    __syncthreads();
    for (int e = t; e < C * C; e += kThreads)
      if (hist[e]) atomicAdd(k.conf + e, (unsigned long long)hist[e]);
  }
}

}  // namespace

extern "C" int memhip_seg_predict(const memhip_segpredict_args_t* a, memhip_stream_t stream) {
  memhip_segpredict_plan_t p;
  int passes;
  if (int rc = seg_predict_plan(a, false, &p, &passes)) return rc;
  if (a->B == 0) return MEMHIP_OK;
  PredK k{};
  k.logits = a->logits; k.sv = a->sv; k.sb = a->sb; k.sc = a->sc; k.sy = a->sy; k.sx = a->sx;
  k.y_i0 = a->y_i0; k.y_w1 = a->y_w1; k.x_i0 = a->x_i0; k.x_w1 = a->x_w1;
  k.pred = a->pred; k.prob = a->prob; k.labels = a->labels; k.conf = reinterpret_cast<unsigned long long*>(a->confusion);
  k.V = a->V; k.C = a->C; k.h = a->h; k.w = a->w; k.hc = a->hc; k.wc = a->wc; k.H = a->H; k.W = a->W;
  k.ignore = a->ignore_index; k.tiles_y = p.tiles_y; k.tiles_x = p.tiles_x; k.passes = passes; k.pred_dwords = p.pred_dwords;
  for (int v = 0; v < a->V; ++v)
    for (int e = 0; e < 3; ++e) k.rect[v][e] = a->rects[3 * v + e];
  const dim3 grid(p.grid), block(p.block);
  switch (p.padded_classes) {
    case 8: hipLaunchKernelGGL(seg_predict_kernel<8>, grid, block, 0, as_stream(stream), k); break;
    case 12: hipLaunchKernelGGL(seg_predict_kernel<12>, grid, block, 0, as_stream(stream), k); break;
    case 16: hipLaunchKernelGGL(seg_predict_kernel<16>, grid, block, 0, as_stream(stream), k); break;
    case 20: hipLaunchKernelGGL(seg_predict_kernel<20>, grid, block, 0, as_stream(stream), k); break;
    case 24: hipLaunchKernelGGL(seg_predict_kernel<24>, grid, block, 0, as_stream(stream), k); break;
    case 28: hipLaunchKernelGGL(seg_predict_kernel<28>, grid, block, 0, as_stream(stream), k); break;
    default: hipLaunchKernelGGL(seg_predict_kernel<32>, grid, block, 0, as_stream(stream), k); break;
  }
  return check_launch("seg_predict");
}
