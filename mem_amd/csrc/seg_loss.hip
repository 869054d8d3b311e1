// The end of a segmentation decode head (mmseg 0.30: resize(seg_logit, bilinear) -> cross_entropy(ignore_index) / accuracy,
// and resize -> argmax -> intersect_and_union at test time) without the upsampled [B, C, H, W] tensor.
//
// Training (seg_ce_kernel): a workgroup owns a tile of 8 x 8 low-resolution pixels.  It holds the tile and one pixel around it,
// all C channels, in LDS (row / column indices clamped at the map's border), and walks its FOOTPRINT -- the outputs
// y_lo[first] .. y_hi[last] x x_lo[first] .. x_hi[last] that read a pixel of the tile -- in row-major chunks of 256, one output
// per thread: the C interpolated logits in registers, max-subtracted log-sum-exp with expf / logf, q_c = softmax_c - [c == label]
// (0 where the label is ignored or >= C) to LDS.  Then thread (pixel p = t % 64, channels t / 64 + 4k) adds the chunk's share
// of its dz elements: over the rows y and columns x of its own range that lie in the chunk, ascending, the weight of the
// tables times q.  Chunks ascend, so every dz element is one fixed-order fp32 sum, written once; no atomics.  The outputs
// between two tiles are computed by both (up to four at a corner): ((t + 1) / t)^2 of the arithmetic.  Loss and counts are
// taken by the output's HOME, the tile of (i0[y], j0[x]): per thread in double / int32, folded through LDS in fixed order,
// one Partial per workgroup stored plainly; seg_finish_kernel (one workgroup) adds the partials in a fixed order and writes
// loss, the backward's factor and the counts.
//
// Every weight comes from the axis tables (seg_plan.cpp) in device memory, staged in LDS for the footprint when they fit:
// forward and gather read the same numbers.  Indices read from a table are clamped before they address anything.
//
// Evaluation (seg_confusion_kernel): a thread per output pixel with a counted label, logits read through the cache, running
// argmax, an LDS histogram per workgroup, nonzero cells flushed with 64-bit integer atomics.
//
// Class weights and OHEM (memhip_seg_ce_w, memhip_seg_ohem_keys; the selection between them is seg_ohem.hip): the training
// kernel's WEIGHTED instantiation multiplies q and the loss term by cw[label] * s, with cw staged in LDS once per workgroup and
// s decided on the key that seg_ohem_keys_kernel stored (a thread per output pixel, like the confusion kernel) against the
// threshold the selection left in device memory.
#include "common.h"
#include "seg_plan.hpp"

namespace {

using namespace memhip;
using namespace memhip::seg;

struct SegK {
  const float* logits; long long sb, sc, sy, sx;
  const uint8_t* labels;
  int B, C, h, w, H, W, ignore;
  const int* y_i0; const float* y_w1; const int* y_lo; const int* y_hi;
  const int* x_i0; const float* x_w1; const int* x_lo; const int* x_hi;
  float* dz; long long db, dc, dy, dx;
  Partial* ws;
  int tiles_y, tiles_x, max_fh, max_fw, tab_lds;
};

// what memhip_seg_ce_w adds: the class weights (NULL: ones) and the sampler's stored keys and threshold (sampler 0: none)
struct SegW {
  const float* cw; const float* keys; const float* threshold;
  int sampler;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the weight with which output (i0, i1 = min(i0 + 1, n - 1), w1) reads input i
__device__ __forceinline__ float weight_of(int i, int i0, int i1, float w1) {
  return (i0 == i ? 1.f - w1 : 0.f) + (i1 == i ? w1 : 0.f);
}

// WEIGHTED: memhip_seg_ce_w -- q and the loss term times f = cw[label] * s, s from the stored key and *threshold; with f = 1.0f
// every product is exact and the bits are those of the plain instantiation
template <int CP, bool WEIGHTED>
__global__ __launch_bounds__(kThreads) void seg_ce_kernel(SegK k, SegW sw) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int kPitch = CP + 1;
  float* zt = reinterpret_cast<float*>(smem);                 // [kHalo * kHalo][kPitch]
  float* qs = zt + kHalo * kHalo * kPitch;                    // [CP][kChunk]
  float* s_cw = qs + CP * kChunk;                             // [kMaxC], WEIGHTED only
  int* s_yi0 = reinterpret_cast<int*>(s_cw + (WEIGHTED ? kMaxC : 0));   // [max_fh], then w1 [max_fh], then the x axis
  float* s_yw1 = reinterpret_cast<float*>(s_yi0 + k.max_fh);
  int* s_xi0 = reinterpret_cast<int*>(s_yw1 + k.max_fh);
  float* s_xw1 = reinterpret_cast<float*>(s_xi0 + k.max_fw);

  const int t = threadIdx.x;
  int wg = blockIdx.x;
  const int tx = wg % k.tiles_x; wg /= k.tiles_x;
  const int ty = wg % k.tiles_y;
  const int b = wg / k.tiles_y;
  const int C = k.C, h = k.h, w = k.w;
  const int i_first = ty * kTile, i_last = min(i_first + kTile, h) - 1;
  const int j_first = tx * kTile, j_last = min(j_first + kTile, w) - 1;
  const int Y0 = clampi(k.y_lo[i_first], 0, k.H - 1), X0 = clampi(k.x_lo[j_first], 0, k.W - 1);
  int Y1 = clampi(k.y_hi[i_last], Y0, k.H - 1), X1 = clampi(k.x_hi[j_last], X0, k.W - 1);
  if (k.tab_lds) {                                            // never past the staged slices
    Y1 = min(Y1, Y0 + k.max_fh - 1);
    X1 = min(X1, X0 + k.max_fw - 1);
  }
  const int fh = Y1 - Y0 + 1, fw = X1 - X0 + 1;
  const int nfp = fh * fw;

  // the tables of the footprint: LDS copies indexed like the originals
  const int* yi0 = k.y_i0; const float* yw1 = k.y_w1; const int* xi0 = k.x_i0; const float* xw1 = k.x_w1;
  if (k.tab_lds) {
    for (int e = t; e < fh; e += kThreads) { s_yi0[e] = k.y_i0[Y0 + e]; s_yw1[e] = k.y_w1[Y0 + e]; }
    for (int e = t; e < fw; e += kThreads) { s_xi0[e] = k.x_i0[X0 + e]; s_xw1[e] = k.x_w1[X0 + e]; }
    yi0 = s_yi0 - Y0; yw1 = s_yw1 - Y0; xi0 = s_xi0 - X0; xw1 = s_xw1 - X0;
  }
  float thr = 0.f;
  if constexpr (WEIGHTED) {
    if (t < kMaxC) s_cw[t] = (sw.cw && t < C) ? sw.cw[t] : 1.f;
    if (sw.sampler) thr = *sw.threshold;
  }
  // the halo tile; neighbouring threads take neighbouring addresses in either layout
  {
    const float* src = k.logits + (long long)b * k.sb;
    const bool rows = k.sc == 1;
    for (int e = t; e < kHalo * kHalo * C; e += kThreads) {
      const int c = rows ? e % C : e / (kHalo * kHalo);
      const int pix = rows ? e / C : e % (kHalo * kHalo);
      const int gi = clampi(i_first - 1 + pix / kHalo, 0, h - 1), gj = clampi(j_first - 1 + pix % kHalo, 0, w - 1);
      zt[pix * kPitch + c] = src[c * k.sc + gi * k.sy + gj * k.sx];
    }
  }
  __syncthreads();

  // the dz elements of this thread: pixel (i, j), channels g + 4 m
  const int g = t >> 6, i = i_first + ((t & 63) >> 3), j = j_first + (t & 7);
  const bool owner = i <= i_last && j <= j_last;
  int ylo_i = 0, yhi_i = -1, xlo_j = 0, xhi_j = -1;
  if (owner) {
    ylo_i = max(k.y_lo[i], Y0); yhi_i = min(k.y_hi[i], Y1);
    xlo_j = max(k.x_lo[j], X0); xhi_j = min(k.x_hi[j], X1);
  }
  float acc[CP / 4];
#pragma unroll
  for (int m = 0; m < CP / 4; ++m) acc[m] = 0.f;

  double loss = 0.0;
  int n_valid = 0, n_correct = 0, n_bad = 0, n_kept = 0;
  const uint8_t* lab_b = k.labels + (long long)b * k.H * k.W;

  for (int base = 0; base < nfp; base += kChunk) {
    const int n = base + t;
    if (n < nfp) {
      const int ry = n / fw;
      const int y = Y0 + ry, x = X0 + (n - ry * fw);
      const int a0 = clampi(yi0[y], 0, h - 1), a1 = min(a0 + 1, h - 1);
      const int b0 = clampi(xi0[x], 0, w - 1), b1 = min(b0 + 1, w - 1);
      const float wy1 = yw1[y], wy0 = 1.f - wy1, wx1 = xw1[x], wx0 = 1.f - wx1;
      const int ly0 = clampi(a0 - i_first + 1, 0, kHalo - 1), ly1 = clampi(a1 - i_first + 1, 0, kHalo - 1);
      const int lx0 = clampi(b0 - j_first + 1, 0, kHalo - 1), lx1 = clampi(b1 - j_first + 1, 0, kHalo - 1);
      const float* p00 = zt + (ly0 * kHalo + lx0) * kPitch;
      const float* p01 = zt + (ly0 * kHalo + lx1) * kPitch;
      const float* p10 = zt + (ly1 * kHalo + lx0) * kPitch;
      const float* p11 = zt + (ly1 * kHalo + lx1) * kPitch;
      const int lab = lab_b[(long long)y * k.W + x];
      const bool counted = lab != k.ignore, valid = counted && lab < C;
      float z[CP];
#pragma unroll
      for (int c = 0; c < CP; ++c)
        z[c] = c < C ? wy0 * (wx0 * p00[c] + wx1 * p01[c]) + wy1 * (wx0 * p10[c] + wx1 * p11[c]) : -INFINITY;
      float mx = z[0], zl = 0.f;
      int am = 0;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        if (c > 0 && z[c] > mx) { mx = z[c]; am = c; }        // strictly greater: ties to the lowest class
        if (c == lab) zl = z[c];
      }
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        z[c] = c < C ? expf(z[c] - mx) : 0.f;
        s += z[c];
      }
      const float inv = valid ? 1.f / s : 0.f;
      const bool home = a0 >= i_first && a0 <= i_last && b0 >= j_first && b0 <= j_last;
      if constexpr (WEIGHTED) {
        bool keep = valid;
        if (valid && sw.sampler) {                             // the decision is taken on the stored key, never recomputed
          const float key = sw.keys[((long long)b * k.H + y) * k.W + x];
          keep = key >= 0.f && (sw.sampler == 1 ? key < thr : key >= thr);
        }
        const float f = keep ? s_cw[valid ? lab : 0] : 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) qs[c * kChunk + t] = valid ? (z[c] * inv - (c == lab ? 1.f : 0.f)) * f : 0.f;
        if (home && valid) {
          loss += (double)f * (double)(logf(s) - (zl - mx));
          n_kept += keep;
        }
      } else {
#pragma unroll
        for (int c = 0; c < CP; ++c) qs[c * kChunk + t] = valid ? z[c] * inv - (c == lab ? 1.f : 0.f) : 0.f;
        if (home && valid) loss += (double)(logf(s) - (zl - mx));
      }
      if (home && valid) {
        n_valid += 1;
        n_correct += am == lab;
      } else if (home && counted) {
        n_bad += 1;
      }
    }
    __syncthreads();
    if (owner) {
      const int lim = min(kChunk, nfp - base);
      const int ya = max(ylo_i, Y0 + base / fw), yb = min(yhi_i, Y0 + (base + lim - 1) / fw);
      for (int y = ya; y <= yb; ++y) {
        const int a0 = clampi(yi0[y], 0, h - 1);
        const float wy = weight_of(i, a0, min(a0 + 1, h - 1), yw1[y]);
        const int rowbase = (y - Y0) * fw - base - X0;        // index in the chunk = rowbase + x
        const int xa = max(xlo_j, -rowbase), xb = min(xhi_j, lim - 1 - rowbase);
        float racc[CP / 4];
#pragma unroll
        for (int m = 0; m < CP / 4; ++m) racc[m] = 0.f;
        for (int x = xa; x <= xb; ++x) {
          const int b0 = clampi(xi0[x], 0, w - 1);
          const float wx = weight_of(j, b0, min(b0 + 1, w - 1), xw1[x]);
          const float* q = qs + rowbase + x;
#pragma unroll
          for (int m = 0; m < CP / 4; ++m) racc[m] = fmaf(wx, q[(g + 4 * m) * kChunk], racc[m]);
        }
#pragma unroll
        for (int m = 0; m < CP / 4; ++m) acc[m] = fmaf(wy, racc[m], acc[m]);
      }
    }
    __syncthreads();
  }

  if (owner) {
    float* out = k.dz + (long long)b * k.db + (long long)i * k.dy + (long long)j * k.dx;
#pragma unroll
    for (int m = 0; m < CP / 4; ++m)
      if (g + 4 * m < C) out[(long long)(g + 4 * m) * k.dc] = acc[m];
  }

  // the workgroup's partial: fixed-order fold through LDS (qs is free: the loop ended on a barrier)
  double* r_loss = reinterpret_cast<double*>(qs);             // qs is 8-byte aligned: kHalo^2 = 100 floats per channel
  int* r_cnt = reinterpret_cast<int*>(r_loss + kThreads);
  r_loss[t] = loss;
  r_cnt[t] = n_valid; r_cnt[kThreads + t] = n_correct; r_cnt[2 * kThreads + t] = n_bad;
  if constexpr (WEIGHTED) r_cnt[3 * kThreads + t] = n_kept;   // 6 KiB of the 8 KiB that eight channels of q give
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      r_loss[t] += r_loss[t + s];
      r_cnt[t] += r_cnt[t + s]; r_cnt[kThreads + t] += r_cnt[kThreads + t + s]; r_cnt[2 * kThreads + t] += r_cnt[2 * kThreads + t + s];
      if constexpr (WEIGHTED) r_cnt[3 * kThreads + t] += r_cnt[3 * kThreads + t + s];
    }
    __syncthreads();
  }
  if (t == 0) k.ws[blockIdx.x] = Partial{r_loss[0], r_cnt[0], r_cnt[kThreads], r_cnt[2 * kThreads], WEIGHTED ? r_cnt[3 * kThreads] : 0};
}

// one workgroup: the G partials in a fixed order -> loss [3] = loss, loss_weight / N, loss_sum; stats [3], or [4] with_kept
__global__ __launch_bounds__(kThreads) void seg_finish_kernel(const Partial* __restrict__ ws, int G, long long pixels, int avg_non_ignore,
                                                              float loss_weight, float* __restrict__ loss, long long* __restrict__ stats,
                                                              int with_kept) {
  __shared__ double r_loss[kThreads];
  __shared__ long long r_cnt[4 * kThreads];
  const int t = threadIdx.x;
  double l = 0.0;
  long long v = 0, c = 0, bad = 0, kept = 0;
  for (int gi = t; gi < G; gi += kThreads) {
    const Partial p = ws[gi];
    l += p.loss; v += p.valid; c += p.correct; bad += p.bad; kept += p.kept;
  }
  r_loss[t] = l;
  r_cnt[t] = v; r_cnt[kThreads + t] = c; r_cnt[2 * kThreads + t] = bad; r_cnt[3 * kThreads + t] = kept;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      r_loss[t] += r_loss[t + s];
      r_cnt[t] += r_cnt[t + s]; r_cnt[kThreads + t] += r_cnt[kThreads + t + s]; r_cnt[2 * kThreads + t] += r_cnt[2 * kThreads + t + s];
      r_cnt[3 * kThreads + t] += r_cnt[3 * kThreads + t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const long long nv = r_cnt[0];
    const double N = avg_non_ignore ? (double)(nv > 1 ? nv : 1) : (double)pixels;
    loss[0] = (float)((double)loss_weight * r_loss[0] / N);
    loss[1] = (float)((double)loss_weight / N);
    loss[2] = (float)r_loss[0];
    stats[0] = nv; stats[1] = r_cnt[kThreads]; stats[2] = r_cnt[2 * kThreads];
    if (with_kept) stats[3] = r_cnt[3 * kThreads];
  }
}

__global__ __launch_bounds__(kConfThreads) void seg_confusion_kernel(SegK k, long long total, unsigned long long* __restrict__ conf) {
  __shared__ int hist[kMaxC * kMaxC];
  const int t = threadIdx.x, C = k.C;
  for (int e = t; e < C * C; e += kConfThreads) hist[e] = 0;
  __syncthreads();
  const long long HW = (long long)k.H * k.W;
  for (long long n = (long long)blockIdx.x * kConfThreads + t; n < total; n += (long long)gridDim.x * kConfThreads) {
    const int lab = k.labels[n];
    if (lab == k.ignore || lab >= C) continue;
    const long long b = n / HW;
    const int r = (int)(n - b * HW), y = r / k.W, x = r - y * k.W;
    const int a0 = clampi(k.y_i0[y], 0, k.h - 1), a1 = min(a0 + 1, k.h - 1);
    const int b0 = clampi(k.x_i0[x], 0, k.w - 1), b1 = min(b0 + 1, k.w - 1);
    const float wy1 = k.y_w1[y], wy0 = 1.f - wy1, wx1 = k.x_w1[x], wx0 = 1.f - wx1;
    const float* src = k.logits + b * k.sb;
    const float* p00 = src + a0 * k.sy + b0 * k.sx;
    const float* p01 = src + a0 * k.sy + b1 * k.sx;
    const float* p10 = src + a1 * k.sy + b0 * k.sx;
    const float* p11 = src + a1 * k.sy + b1 * k.sx;
    float mx = 0.f;
    int am = 0;
    for (int c = 0; c < C; ++c) {
      const long long o = c * k.sc;
      const float z = wy0 * (wx0 * p00[o] + wx1 * p01[o]) + wy1 * (wx0 * p10[o] + wx1 * p11[o]);
      if (c == 0 || z > mx) { mx = z; am = c; }
    }
    atomicAdd(&hist[lab * C + am], 1);
  }
  __syncthreads();
  for (int e = t; e < C * C; e += kConfThreads)
    if (hist[e]) atomicAdd(conf + e, (unsigned long long)hist[e]);
}

// The sampler's keys: a thread per output pixel, the interpolation of the kernels above, two walks over the channels (the
// maximum and the label's logit, then the sum of expf(z - max): the same fp32 chain as the training kernel's).
// mode 1: softmax[label]; mode 2: cw[label] * nll.  Pixels that are not valid store -1.0f.
__global__ __launch_bounds__(kConfThreads) void seg_ohem_keys_kernel(SegK k, long long total, int mode, const float* __restrict__ cw,
                                                                     float* __restrict__ keys) {
  const int C = k.C;
  const long long HW = (long long)k.H * k.W;
  for (long long n = (long long)blockIdx.x * kConfThreads + threadIdx.x; n < total; n += (long long)gridDim.x * kConfThreads) {
    const int lab = k.labels[n];
    if (lab == k.ignore || lab >= C) { keys[n] = -1.f; continue; }
    const long long b = n / HW;
    const int r = (int)(n - b * HW), y = r / k.W, x = r - y * k.W;
    const int a0 = clampi(k.y_i0[y], 0, k.h - 1), a1 = min(a0 + 1, k.h - 1);
    const int b0 = clampi(k.x_i0[x], 0, k.w - 1), b1 = min(b0 + 1, k.w - 1);
    const float wy1 = k.y_w1[y], wy0 = 1.f - wy1, wx1 = k.x_w1[x], wx0 = 1.f - wx1;
    const float* src = k.logits + b * k.sb;
    const float* p00 = src + a0 * k.sy + b0 * k.sx;
    const float* p01 = src + a0 * k.sy + b1 * k.sx;
    const float* p10 = src + a1 * k.sy + b0 * k.sx;
    const float* p11 = src + a1 * k.sy + b1 * k.sx;
    float mx = 0.f, zl = 0.f;
    for (int c = 0; c < C; ++c) {
      const long long o = c * k.sc;
      const float z = wy0 * (wx0 * p00[o] + wx1 * p01[o]) + wy1 * (wx0 * p10[o] + wx1 * p11[o]);
      if (c == 0 || z > mx) mx = z;
      if (c == lab) zl = z;
    }
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      const long long o = c * k.sc;
      const float z = wy0 * (wx0 * p00[o] + wx1 * p01[o]) + wy1 * (wx0 * p10[o] + wx1 * p11[o]);
      s += expf(z - mx);
    }
    float key;
    if (mode == 1) {
      key = expf(zl - mx) / s;
    } else {
      key = (logf(s) - (zl - mx)) * (cw ? cw[lab] : 1.f);
    }
    keys[n] = key > 0.f ? key : 0.f;                          // never -0.0f, never below the smallest key that counts
  }
}

SegK kernel_args(const memhip_seg_args_t* a, const memhip_seg_plan_t& p) {
  SegK k{};
  k.logits = a->logits; k.sb = a->sb; k.sc = a->sc; k.sy = a->sy; k.sx = a->sx;
  k.labels = a->labels;
  k.B = a->B; k.C = a->C; k.h = a->h; k.w = a->w; k.H = a->H; k.W = a->W; k.ignore = a->ignore_index;
  k.y_i0 = a->y_i0; k.y_w1 = a->y_w1; k.y_lo = a->y_lo; k.y_hi = a->y_hi;
  k.x_i0 = a->x_i0; k.x_w1 = a->x_w1; k.x_lo = a->x_lo; k.x_hi = a->x_hi;
  k.dz = a->dz; k.db = a->db; k.dc = a->dc; k.dy = a->dy; k.dx = a->dx;
  k.ws = static_cast<Partial*>(a->workspace);
  k.tiles_y = p.tiles_y; k.tiles_x = p.tiles_x; k.max_fh = p.max_fh; k.max_fw = p.max_fw; k.tab_lds = p.tables_in_lds;
  return k;
}

// the training kernel of either entry and its finish kernel
template <bool WEIGHTED>
void launch_ce(const memhip_seg_args_t* a, const memhip_seg_plan_t& p, const SegW& sw, memhip_stream_t stream) {
  const SegK k = kernel_args(a, p);
  const dim3 grid(p.grid), block(p.block);
  switch (padded_channels(a->C)) {
    case 8: hipLaunchKernelGGL((seg_ce_kernel<8, WEIGHTED>), grid, block, p.lds_bytes, as_stream(stream), k, sw); break;
    case 12: hipLaunchKernelGGL((seg_ce_kernel<12, WEIGHTED>), grid, block, p.lds_bytes, as_stream(stream), k, sw); break;
    case 16: hipLaunchKernelGGL((seg_ce_kernel<16, WEIGHTED>), grid, block, p.lds_bytes, as_stream(stream), k, sw); break;
    case 20: hipLaunchKernelGGL((seg_ce_kernel<20, WEIGHTED>), grid, block, p.lds_bytes, as_stream(stream), k, sw); break;
    case 24: hipLaunchKernelGGL((seg_ce_kernel<24, WEIGHTED>), grid, block, p.lds_bytes, as_stream(stream), k, sw); break;
    case 28: hipLaunchKernelGGL((seg_ce_kernel<28, WEIGHTED>), grid, block, p.lds_bytes, as_stream(stream), k, sw); break;
    default: hipLaunchKernelGGL((seg_ce_kernel<32, WEIGHTED>), grid, block, p.lds_bytes, as_stream(stream), k, sw); break;
  }
  hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), k.ws, p.grid, (long long)a->B * a->H * a->W,
                     a->avg_non_ignore, a->loss_weight, a->loss, reinterpret_cast<long long*>(a->stats), WEIGHTED ? 1 : 0);
}

}  // namespace

extern "C" int memhip_seg_ce(const memhip_seg_args_t* a, memhip_stream_t stream) {
  memhip_seg_plan_t p;
  if (int rc = seg_plan(a, SEG_CE, &p)) return rc;
  launch_ce<false>(a, p, SegW{}, stream);
  return check_launch("seg_ce");
}

extern "C" int memhip_seg_ce_w(const memhip_segohem_args_t* a, memhip_stream_t stream) {
  memhip_segohem_plan_t p;
  if (int rc = seg_ohem_plan(a, OHEM_CE, &p)) return rc;
  launch_ce<true>(&a->seg, p.seg, SegW{a->class_weight, a->keys, a->threshold, a->sampler}, stream);
  return check_launch("seg_ce_w");
}

extern "C" int memhip_seg_confusion(const memhip_seg_args_t* a, memhip_stream_t stream) {
  memhip_seg_plan_t p;
  if (int rc = seg_plan(a, SEG_CONFUSION, &p)) return rc;
  hipLaunchKernelGGL(seg_confusion_kernel, dim3(p.conf_grid), dim3(p.conf_block), 0, as_stream(stream), kernel_args(a, p),
                     (long long)a->B * a->H * a->W, reinterpret_cast<unsigned long long*>(a->confusion));
  return check_launch("seg_confusion");
}

extern "C" int memhip_seg_ohem_keys(const memhip_segohem_args_t* a, memhip_stream_t stream) {
  memhip_segohem_plan_t p;
  if (int rc = seg_ohem_plan(a, OHEM_KEYS, &p)) return rc;
  hipLaunchKernelGGL(seg_ohem_keys_kernel, dim3(p.keys_grid), dim3(p.keys_block), 0, as_stream(stream), kernel_args(&a->seg, p.seg),
                     (long long)a->seg.B * a->seg.H * a->seg.W, a->sampler, a->class_weight, a->keys);
  return check_launch("seg_ohem_keys");
}
