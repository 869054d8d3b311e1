// The FCN decode head around its 3x3 convolution (mmseg 0.30 FCNHead.forward / BaseDecodeHead.cls_seg: Conv2d(3, padding 1,
// bias=False) -> SyncBN -> ReLU -> Dropout2d -> Conv2d(1); mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:38-50).
// The convolution, its data gradient and its weight gradient are conv.hip / conv_wgrad.hip on the tokenizer's activation
// format, bf16 [B, h+2, w+2, C] with a one-pixel zero border.  Here: the movers between the engine's fp32 maps and that
// format, the batch statistics, and the fused batch norm + ReLU + Dropout2d + classifier, forward and backward.
//
// Every kernel streams: 256 threads, a lane moves 16 bytes of bf16 (8 channels), 8 neighbouring lanes the 128 bytes of 64
// channels of one pixel.  Pixel r = (b, y, x) of the R = B h w lies at ((b (h+2) + y+1) (w+2) + x+1) C of the padded format;
// rings are neither read nor written.  No float atomics: sums are per-workgroup partials stored plainly and folded in
// ascending order by a second launch, so two calls give the same bits.
//
//   movers       bn_tile.hpp's map side and row side (shared with necks.hip) around one 64 pixel x 64 channel LDS tile; the
//                rows are those of the padded format
//   bn_stats     thread (row lane j = t / 8, channels 8 (t % 8)..): a chain over the rows 32 g + j, + 32 G, ..; the 32 row
//                lanes folded in LDS in order (bn_tile.hpp), the partials by the library's one ordered fold (fold.hip)
//   bnhead_fwd   the classifier weight [KP, C] fp32 in LDS once per workgroup (KP = K rounded up to 8, zero rows behind K);
//                a tile is 32 pixels, the 8 lanes of a pixel walk the channels in chunks of 64 with KP accumulators each
//                (weights as ds_read_b128, broadcast over the pixels) and add up in a 3-step butterfly; lane i of the 8
//                stores the classes i, i + 8, ..
//   bwd_sums     grid (pixel groups, C / 64): the weight's chunk [KP, 64] and the gradients of 64 pixels [64, KP + 1] in LDS;
//                phase B (the forward's thread shape) recomputes xhat, the gate and z, takes dz from the gradient tile and
//                the weight chunk, chains sum g and sum g xhat in registers and leaves z [64, 65] in LDS; phase C (thread =
//                channel t % 64, classes t / 64 + 4 j) adds dlogit[p, k] z[p, c] over the tile's pixels
//   bwd_apply    phase B again with the two correction terms, written as bf16 into the padded interior
#include "common.h"
#include "bn_tile.hpp"
#include "dropout.hpp"
#include "seg_head_plan.hpp"

namespace {

using namespace memhip;
using namespace memhip::seghead;
using bn::kT, bn::kTile, bn::kPitch, bn::f4, bn::us8, bn::bf16_t, bn::bf2f, bn::f2bf, bn::BnParams, bn::FoldOut, bn::aligned;
static_assert(kThreads == kT && kChunk == kTile && seghead::kGroups == bn::kGroups, "the plan's constants are the tile's");

struct Geom {
  int C, h, w, P;    // P = h * w
  long long R;       // B * P
};

// element offset of channel 0 of pixel r in the padded format
__device__ __forceinline__ long long pad_off(const Geom& g, long long r) {
  const long long b = r / g.P;
  const int p = (int)(r - b * g.P), y = p / g.w, x = p - y * g.w;
  return ((b * (g.h + 2) + y + 1) * (g.w + 2) + x + 1) * g.C;
}

// ---------------------------------------------------------------- movers
// where the rows of the padded format lie (bn_tile.hpp: row_side)
struct PadRows {
  Geom g;
  __device__ __forceinline__ long long operator()(long long r) const { return pad_off(g, r); }
};

template <bool VEC>
__global__ __launch_bounds__(kT) void map_to_nhwc_pad_kernel(const float* __restrict__ map, Geom g, bf16_t* __restrict__ out) {
  __shared__ float tile[kTile * kPitch];
  const long long z0 = (long long)blockIdx.x * kTile;
  const int c0 = blockIdx.y * kTile;
  bn::map_side<VEC, true>(map, g.C, g.P, g.R, z0, c0, tile);
  __syncthreads();
  bn::row_side<false>(out, g.R, PadRows{g}, z0, c0, tile);
}

template <bool VEC>
__global__ __launch_bounds__(kT) void nhwc_pad_to_map_kernel(const bf16_t* __restrict__ in, Geom g, float* __restrict__ map) {
  __shared__ float tile[kTile * kPitch];
  const long long z0 = (long long)blockIdx.x * kTile;
  const int c0 = blockIdx.y * kTile;
  bn::row_side<true>(in, g.R, PadRows{g}, z0, c0, tile);
  __syncthreads();
  bn::map_side<VEC, false>(map, g.C, g.P, g.R, z0, c0, tile);
}

// ---------------------------------------------------------------- batch statistics
template <bool PADDED>
__global__ __launch_bounds__(kT) void bn_stats_kernel(const bf16_t* __restrict__ x, Geom g, const float* __restrict__ shift,
                                                      float* __restrict__ ws) {
  __shared__ float red[2 * 32 * 64];
  const int t = threadIdx.x, c0 = blockIdx.y * kChunk, c = 8 * (t & 7);
  float s[8], a1[8], a2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    s[e] = shift ? shift[c0 + c + e] : 0.f;
    a1[e] = a2[e] = 0.f;
  }
  for (long long r = (long long)blockIdx.x * 32 + (t >> 3); r < g.R; r += 32LL * gridDim.x) {
    const long long off = PADDED ? pad_off(g, r) : r * g.C;
    const us8 v = *reinterpret_cast<const us8*>(x + off + c0 + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = bf2f(v[e]) - s[e];
      a1[e] += d;
      a2[e] = fmaf(d, d, a2[e]);
    }
  }
  bn::fold_rows_and_store<32, 8>(a1, a2, red, ws + (long long)blockIdx.x * 2 * g.C, g.C, c0);
}

// ---------------------------------------------------------------- batch norm + ReLU + Dropout2d + classifier
struct Chan8 { float m[8], rs[8], ga[8], be[8]; };

__device__ __forceinline__ void load8(const float* __restrict__ p, float (&o)[8]) {
  const f4 a = *reinterpret_cast<const f4*>(p), b = *reinterpret_cast<const f4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { o[e] = a[e]; o[4 + e] = b[e]; }
}

__device__ __forceinline__ Chan8 chan8(const BnParams& p, int c) {
  Chan8 k;
  load8(p.mean + c, k.m); load8(p.rstd + c, k.rs); load8(p.gamma + c, k.ga); load8(p.beta + c, k.be);
  return k;
}

struct Drop {
  DropParams d;
  int on;
};

// the keep multipliers of channels c .. c + 7 of sample b: scale (kept) or 0 (dropped); 1 without dropout
__device__ __forceinline__ void keep8(const Drop& dr, long long b, int c, float (&km)[8]) {
  unsigned bits = 0xffu;
  float scale = 1.f;
  if (dr.on) {
    bits = dropout_keep8(dr.d, (unsigned)(dr.d.row0 + b), (unsigned)(c >> 3));
    scale = dr.d.scale;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) km[e] = ((bits >> e) & 1u) ? scale : 0.f;
}

// xhat, u = gamma xhat + beta of 8 channels of one pixel
__device__ __forceinline__ void bn8(const us8& v, const Chan8& k, float (&xh)[8], float (&u)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    xh[e] = (bf2f(v[e]) - k.m[e]) * k.rs[e];
    u[e] = fmaf(xh[e], k.ga[e], k.be[e]);
  }
}

// the classifier weight rows [KP, ncols] of columns col0 .. into LDS, rows >= K zero; wl[k * ncols + c]
__device__ __forceinline__ void stage_weight(const float* __restrict__ wcls, int K, int KP, int C, int col0, int ncols, float* wl) {
  const int per_row = ncols >> 2;
  for (int i = threadIdx.x; i < KP * per_row; i += kT) {
    const int k = i / per_row, c4 = (i - k * per_row) << 2;
    f4 v = 0.f;
    if (k < K) v = *reinterpret_cast<const f4*>(wcls + (long long)k * C + col0 + c4);
    *reinterpret_cast<f4*>(wl + k * ncols + c4) = v;
  }
}

template <int KP>
__global__ __launch_bounds__(kT) void bnhead_fwd_kernel(const bf16_t* __restrict__ y, Geom g, BnParams bp, const float* __restrict__ wcls,
                                                        const float* __restrict__ bias, int K, Drop dr, float* __restrict__ logits,
                                                        long long ld) {
  extern __shared__ __attribute__((aligned(16))) float wl[];         // [KP, C]
  const int t = threadIdx.x, cg = t & 7;
  stage_weight(wcls, K, KP, g.C, 0, g.C, wl);
  __syncthreads();
  const long long tiles = (g.R + kFwdPixels - 1) / kFwdPixels;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long r = tile * kFwdPixels + (t >> 3);
    const bool ok = r < g.R;
    const long long b = ok ? r / g.P : 0;
    const bf16_t* src = y + (ok ? pad_off(g, r) : 0) + 8 * cg;
    float acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.f;
    for (int ch = 0; ch < g.C; ch += kChunk) {
      const int c = ch + 8 * cg;
      us8 v = 0;
      if (ok) v = *reinterpret_cast<const us8*>(src + ch);
      const Chan8 k8 = chan8(bp, c);
      float xh[8], u[8], km[8], z[8];
      bn8(v, k8, xh, u);
      keep8(dr, b, c, km);
#pragma unroll
      for (int e = 0; e < 8; ++e) z[e] = fmaxf(u[e], 0.f) * km[e];
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        const f4 w0 = *reinterpret_cast<const f4*>(wl + k * g.C + c), w1 = *reinterpret_cast<const f4*>(wl + k * g.C + c + 4);
        float s = acc[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(z[e], w0[e], s);
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(z[4 + e], w1[e], s);
        acc[k] = s;
      }
    }
    // the 8 lanes of a pixel: a butterfly in fixed order, every lane ends with the whole sum
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      float s = acc[k];
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      s += __shfl_xor(s, 4);
      acc[k] = s;
    }
#pragma unroll
    for (int j = 0; j < KP / 8; ++j) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s = cg == i ? acc[8 * j + i] : s;
      const int k = 8 * j + cg;
      if (ok && k < K) logits[r * ld + k] = s + (bias ? bias[k] : 0.f);
    }
  }
}

// the gradients of `npix` pixels from r0 into dlt [npix, KP + 1], zero past the end and behind K
struct DlStrides { long long b, k, y, x; };
template <int KP>
__device__ __forceinline__ void load_dl_tile(const float* __restrict__ dlogit, const DlStrides& ds, const Geom& g, int K,
                                             long long r0, int npix, float* dlt) {
  const int lanes = kT / npix;                                       // 4 (64 pixels) or 8 (32 pixels)
  const int p = threadIdx.x / lanes, kk = threadIdx.x % lanes;
  const long long r = r0 + p;
  const bool ok = r < g.R;
  long long base = 0;
  if (ok) {
    const long long b = r / g.P;
    const int q = (int)(r - b * g.P), yy = q / g.w, xx = q - yy * g.w;
    base = b * ds.b + yy * ds.y + xx * ds.x;
  }
  for (int k = kk; k < KP; k += lanes) dlt[p * (KP + 1) + k] = (ok && k < K) ? dlogit[base + k * ds.k] : 0.f;
}

// phase B for the 8 channels c0 + 8 cg .. of pixel row `pl` of the tile: xhat and g = dz keep scale (u > 0), z
template <int KP>
__device__ __forceinline__ void head_grad8(const us8& v, const Chan8& k8, const float (&km)[8], const float* wl, const float* dl,
                                           int cg, float (&xh)[8], float (&gg)[8], float (&z)[8]) {
  float u[8], dz[8];
  bn8(v, k8, xh, u);
#pragma unroll
  for (int e = 0; e < 8; ++e) dz[e] = 0.f;
#pragma unroll 4
  for (int k = 0; k < KP; ++k) {                   // (not unrolled whole: the weight reads would all be hoisted into registers)
    const float d = dl[k];
    const f4 w0 = *reinterpret_cast<const f4*>(wl + k * kChunk + 8 * cg), w1 = *reinterpret_cast<const f4*>(wl + k * kChunk + 8 * cg + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dz[e] = fmaf(d, w0[e], dz[e]);
      dz[4 + e] = fmaf(d, w1[e], dz[4 + e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    gg[e] = u[e] > 0.f ? dz[e] * km[e] : 0.f;
    z[e] = fmaxf(u[e], 0.f) * km[e];
  }
}

template <int KP>
__global__ __launch_bounds__(kT) void bnhead_bwd_sums_kernel(const float* __restrict__ dlogit, DlStrides ds, const bf16_t* __restrict__ y,
                                                             Geom g, BnParams bp, const float* __restrict__ wcls, int K, Drop dr,
                                                             float* __restrict__ ws, int slot) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* wl = lds;                                   // [KP, 64]
  float* dlt = wl + KP * kChunk;                     // [64, KP + 1]
  float* zt = dlt + kBwdPixels * (KP + 1);           // [64, 65]; the fold's scratch at the end
  const int t = threadIdx.x, cg = t & 7, c0 = blockIdx.y * kChunk;
  stage_weight(wcls, K, KP, g.C, c0, kChunk, wl);
  const Chan8 k8 = chan8(bp, c0 + 8 * cg);
  float a1[8], a2[8], dw[KP / 4], dbs = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) a1[e] = a2[e] = 0.f;
#pragma unroll
  for (int j = 0; j < KP / 4; ++j) dw[j] = 0.f;
  const long long tiles = (g.R + kBwdPixels - 1) / kBwdPixels;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long r0 = tile * kBwdPixels;
    __syncthreads();                                 // the weight is staged; the previous tile's readers are done
    load_dl_tile<KP>(dlogit, ds, g, K, r0, kBwdPixels, dlt);
    __syncthreads();
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      const int pl = (t >> 3) + 32 * half;
      const long long r = r0 + pl;
      const bool ok = r < g.R;
      us8 v = 0;
      if (ok) v = *reinterpret_cast<const us8*>(y + pad_off(g, r) + c0 + 8 * cg);
      float km[8], xh[8], gg[8], z[8];
      keep8(dr, ok ? r / g.P : 0, c0 + 8 * cg, km);
      head_grad8<KP>(v, k8, km, wl, dlt + pl * (KP + 1), cg, xh, gg, z);
#pragma unroll
      for (int e = 0; e < 8; ++e) {                  // a pixel past the end has a zero gradient row: g = 0
        a1[e] += gg[e];
        a2[e] = fmaf(gg[e], xh[e], a2[e]);
        zt[pl * kPitch + 8 * cg + e] = ok ? z[e] : 0.f;
      }
    }
    __syncthreads();
    {
      const int c = t & 63, kq = t >> 6;
#pragma unroll 4
      for (int p = 0; p < kBwdPixels; ++p) {
        const float zz = zt[p * kPitch + c];
#pragma unroll
        for (int j = 0; j < KP / 4; ++j) dw[j] = fmaf(dlt[p * (KP + 1) + kq + 4 * j], zz, dw[j]);
      }
      if (blockIdx.y == 0 && t < K) {
#pragma unroll 4
        for (int p = 0; p < kBwdPixels; ++p) dbs += dlt[p * (KP + 1) + t];
      }
    }
  }
  float* ws_slot = ws + (long long)blockIdx.x * slot;
  {
    const int c = t & 63, kq = t >> 6;
#pragma unroll
    for (int j = 0; j < KP / 4; ++j) {
      const int k = kq + 4 * j;
      if (k < K) ws_slot[2 * g.C + k * g.C + c0 + c] = dw[j];
    }
    if (blockIdx.y == 0 && t < K) ws_slot[2 * g.C + K * g.C + t] = dbs;
  }
  __syncthreads();                                   // the last tile's readers of zt are done
  bn::fold_rows_and_store<32, 8>(a1, a2, zt, ws_slot, g.C, c0);
}

template <int KP>
__global__ __launch_bounds__(kT) void bnhead_bwd_apply_kernel(const float* __restrict__ dlogit, DlStrides ds, const bf16_t* __restrict__ y,
                                                              Geom g, BnParams bp, const float* __restrict__ wcls, int K, Drop dr,
                                                              const float* __restrict__ tot, float inv_n, bf16_t* __restrict__ dy) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* wl = lds;                                   // [KP, 64]
  float* dlt = wl + KP * kChunk;                     // [32, KP + 1]
  const int t = threadIdx.x, cg = t & 7, c0 = blockIdx.y * kChunk, c = c0 + 8 * cg;
  const long long r0 = (long long)blockIdx.x * kFwdPixels;
  stage_weight(wcls, K, KP, g.C, c0, kChunk, wl);
  load_dl_tile<KP>(dlogit, ds, g, K, r0, kFwdPixels, dlt);
  const Chan8 k8 = chan8(bp, c);
  float m1[8], m2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    m1[e] = tot ? tot[c + e] * inv_n : 0.f;
    m2[e] = tot ? tot[g.C + c + e] * inv_n : 0.f;
  }
  __syncthreads();
  const int pl = t >> 3;
  const long long r = r0 + pl;
  if (r >= g.R) return;
  const long long off = pad_off(g, r) + c;
  const us8 v = *reinterpret_cast<const us8*>(y + off);
  float km[8], xh[8], gg[8], z[8];
  keep8(dr, r / g.P, c, km);
  head_grad8<KP>(v, k8, km, wl, dlt + pl * (KP + 1), cg, xh, gg, z);
  us8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = f2bf(k8.ga[e] * k8.rs[e] * (gg[e] - m1[e] - xh[e] * m2[e]));
  *reinterpret_cast<us8*>(dy + off) = o;
}

// ---------------------------------------------------------------- host side
int check_geom(const char* what, int B, int C, int h, int w, Geom& g) {
  MEMHIP_REQUIRE(B >= 0 && h >= 1 && w >= 1 && C > 0 && C % kChunk == 0 && C / kChunk <= 65535,
                 "%s: bad shape B=%d C=%d h=%d w=%d (B >= 0, h and w positive, C a positive multiple of 64)", what, B, C, h, w);
  const long long R = (long long)B * h * w;
  MEMHIP_REQUIRE((long long)h * w <= (1 << 24) && R <= (1LL << 30), "%s: bad shape, too many pixels (B=%d h=%d w=%d)", what, B, h, w);
  g = Geom{C, h, w, h * w, R};
  return MEMHIP_OK;
}

Drop drop_of(const memhip_dropout_t* d) {
  Drop dr{};
  if (d) { dr.d = drop_params(*d); dr.on = 1; }
  return dr;
}

// f(std::integral_constant<int, KP>) for KP = 8, 16, 24, 32
template <typename F>
int dispatch_kp(int kp, F&& f) {
  switch (kp) {
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 24: return f(std::integral_constant<int, 24>{});
    default: return f(std::integral_constant<int, 32>{});
  }
}

}  // namespace

extern "C" int memhip_map_to_nhwc_pad(const float* map, int B, int D, int h, int w, void* out, memhip_stream_t stream) {
  Geom g;
  if (int rc = check_geom("map_to_nhwc_pad", B, D, h, w, g)) return rc;
  if (g.R == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(map && out, "map_to_nhwc_pad: null pointer");
  MEMHIP_REQUIRE(aligned(map, 4) && aligned(out, 16), "map_to_nhwc_pad: map is not 4-byte or out is not 16-byte aligned");
  const dim3 grid(cdiv(g.R, kTile), D / kTile);
  bf16_t* o = static_cast<bf16_t*>(out);
  if (g.P % 4 == 0 && aligned(map, 16))
    hipLaunchKernelGGL(map_to_nhwc_pad_kernel<true>, grid, dim3(kT), 0, as_stream(stream), map, g, o);
  else
    hipLaunchKernelGGL(map_to_nhwc_pad_kernel<false>, grid, dim3(kT), 0, as_stream(stream), map, g, o);
  return check_launch("map_to_nhwc_pad");
}

extern "C" int memhip_nhwc_pad_to_map(const void* in, int B, int D, int h, int w, float* map, memhip_stream_t stream) {
  Geom g;
  if (int rc = check_geom("nhwc_pad_to_map", B, D, h, w, g)) return rc;
  if (g.R == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(map && in, "nhwc_pad_to_map: null pointer");
  MEMHIP_REQUIRE(aligned(map, 4) && aligned(in, 16), "nhwc_pad_to_map: map is not 4-byte or in is not 16-byte aligned");
  const dim3 grid(cdiv(g.R, kTile), D / kTile);
  const bf16_t* i = static_cast<const bf16_t*>(in);
  if (g.P % 4 == 0 && aligned(map, 16))
    hipLaunchKernelGGL(nhwc_pad_to_map_kernel<true>, grid, dim3(kT), 0, as_stream(stream), i, g, map);
  else
    hipLaunchKernelGGL(nhwc_pad_to_map_kernel<false>, grid, dim3(kT), 0, as_stream(stream), i, g, map);
  return check_launch("nhwc_pad_to_map");
}

extern "C" size_t memhip_bn_stats_workspace(int C) { return C > 0 ? (size_t)kGroups * 2 * C * sizeof(float) : 0; }

extern "C" int memhip_bn_stats_nhwc(const void* x, int padded, int B, int h, int w, int C, const float* shift, float* workspace,
                                    size_t workspace_bytes, float* out, memhip_stream_t stream) {
  Geom g;
  if (int rc = check_geom("bn_stats_nhwc", B, C, h, w, g)) return rc;
  MEMHIP_REQUIRE(padded == 0 || padded == 1, "bn_stats_nhwc: padded=%d must be 0 or 1", padded);
  if (g.R == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(x && workspace && out, "bn_stats_nhwc: null pointer");
  MEMHIP_REQUIRE(aligned(x, 16), "bn_stats_nhwc: x is not 16-byte aligned");
  MEMHIP_REQUIRE(workspace_bytes >= memhip_bn_stats_workspace(C), "bn_stats_nhwc: workspace of %zu bytes, %zu needed", workspace_bytes,
                 memhip_bn_stats_workspace(C));
  const long long units = (g.R + 31) / 32;
  const int G = (int)(units < kGroups ? units : kGroups);
  const bf16_t* xb = static_cast<const bf16_t*>(x);
  if (padded)
    hipLaunchKernelGGL(bn_stats_kernel<true>, dim3(G, C / kChunk), dim3(kT), 0, as_stream(stream), xb, g, shift, workspace);
  else
    hipLaunchKernelGGL(bn_stats_kernel<false>, dim3(G, C / kChunk), dim3(kT), 0, as_stream(stream), xb, g, shift, workspace);
  bn::launch_fold(workspace, G, 2 * C, bn::fold_grid(2 * C), FoldOut{{out + C, nullptr, nullptr}, {2 * C, 0, 0}, out, C, (float)g.R},
                  as_stream(stream));
  return check_launch("bn_stats_nhwc");
}

extern "C" int memhip_bnhead_fwd(const memhip_bnhead_args_t* a, memhip_stream_t stream) {
  memhip_bnhead_plan_t p;
  if (int rc = bnhead_plan(a, BNHEAD_FWD, &p)) return rc;
  if (p.R == 0) return MEMHIP_OK;
  const Geom g{a->C, a->h, a->w, a->h * a->w, p.R};
  const BnParams bp{a->mean, a->rstd, a->gamma, a->beta};
  const Drop dr = drop_of(a->dropout);
  dispatch_kp(p.kp, [&](auto kp) {
    hipLaunchKernelGGL(bnhead_fwd_kernel<decltype(kp)::value>, dim3(p.fwd_grid), dim3(p.block), p.fwd_lds_bytes, as_stream(stream),
                       static_cast<const bf16_t*>(a->y), g, bp, a->wcls, a->bias, a->K, dr, a->logits, (long long)a->ld);
    return 0;
  });
  return check_launch("bnhead_fwd");
}

extern "C" int memhip_bnhead_bwd_sums(const memhip_bnhead_args_t* a, memhip_stream_t stream) {
  memhip_bnhead_plan_t p;
  if (int rc = bnhead_plan(a, BNHEAD_SUMS, &p)) return rc;
  if (p.R == 0) return MEMHIP_OK;
  const Geom g{a->C, a->h, a->w, a->h * a->w, p.R};
  const BnParams bp{a->mean, a->rstd, a->gamma, a->beta};
  const Drop dr = drop_of(a->dropout);
  const DlStrides ds{a->db, a->dk, a->dy, a->dx};
  float* ws = static_cast<float*>(a->workspace);
  dispatch_kp(p.kp, [&](auto kp) {
    hipLaunchKernelGGL(bnhead_bwd_sums_kernel<decltype(kp)::value>, dim3(p.sums_grid_x, p.sums_grid_y), dim3(p.block), p.sums_lds_bytes,
                       as_stream(stream), a->dlogit, ds, static_cast<const bf16_t*>(a->y), g, bp, a->wcls, a->K, dr, ws, p.slot_floats);
    return 0;
  });
  bn::launch_fold(ws, p.sums_grid_x, p.slot_floats, p.fold_grid,
                  FoldOut{{a->sums, a->dwcls, a->dbias}, {2 * a->C, a->K * a->C, a->K}, nullptr, 0, 0.f}, as_stream(stream));
  return check_launch("bnhead_bwd_sums");
}

extern "C" int memhip_bnhead_bwd_apply(const memhip_bnhead_args_t* a, memhip_stream_t stream) {
  memhip_bnhead_plan_t p;
  if (int rc = bnhead_plan(a, BNHEAD_APPLY, &p)) return rc;
  if (p.R == 0) return MEMHIP_OK;
  const Geom g{a->C, a->h, a->w, a->h * a->w, p.R};
  const BnParams bp{a->mean, a->rstd, a->gamma, a->beta};
  const Drop dr = drop_of(a->dropout);
  const DlStrides ds{a->db, a->dk, a->dy, a->dx};
  dispatch_kp(p.kp, [&](auto kp) {
    hipLaunchKernelGGL(bnhead_bwd_apply_kernel<decltype(kp)::value>, dim3(p.apply_grid_x, p.apply_grid_y), dim3(p.block),
                       p.apply_lds_bytes, as_stream(stream), a->dlogit, ds, static_cast<const bf16_t*>(a->y), g, bp, a->wcls, a->K, dr,
                       a->tot, a->inv_n, static_cast<bf16_t*>(a->dy_out));
    return 0;
  });
  return check_launch("bnhead_bwd_apply");
}
