// The pyramid pooling of the PSP decode head (mmseg 0.30 mmseg/models/decode_heads/psp_head.py, PPM and PSPHead.forward up
// to the bottleneck's operand -- UPerHead.psp_forward is the same lines; pool_scales=(1, 2, 3, 6), channels=512:
// mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:25-37): per pool scale AdaptiveAvgPool2d(s) -> Conv2d(1,
// bias=False) -> SyncBN -> ReLU -> bilinear resize to the map's size, then cat([x] + outs, dim=1).  The 1x1 convolutions,
// their data and weight gradients and the batch statistics are conv.hip / conv_wgrad.hip / seg_head.hip on the activation
// format bf16 [B, m+2, m'+2, channels] with a zero ring.  Here: what makes the head a pyramid head.
//
// Every kernel streams: 256 threads, a lane moves 16 bytes of bf16 (8 channels), 8 neighbouring lanes the 128 bytes of 64
// channels; rings are neither read nor written.  No float atomics and no partials: every sum is one thread's chain in an order
// the shapes fix (the 32 row lanes of the channel sums are folded in LDS in order by the one workgroup that owns the channels).
//
//   pool         a workgroup per (sample, 64 channels) walks the sample's pixels in tiles of 64 through bn_tile.hpp's map side
//                (the map is read once); thread (channel t % 64, t / 64) owns the bins t / 64, + 4, .. of all scales for its
//                channel, an fp32 accumulator each in LDS, and adds the tile's pixels of the bin in row-major order
//   concat_fwd   grid (tiles of 64 pixels, Cin / 64 + n C / 64): the first Cin / 64 are the mover of seg_head.hip with the row
//                pitch Cin + n C; the others take 8 channels of a pixel of one scale: four 16-byte taps of Y, batch norm and
//                ReLU on each, the bilinear combination, one 16-byte store
//   bwd gather   thread = 8 channels of one (sample, bin) row of one scale: the outputs lo .. hi of both axes in ascending
//                order, the weight of each from the tables the forward read; the gate from the stored Y; g as fp32 rows
//   bwd sums     grid (n, C / 64): row lane t / 8 chains over the rows j, j + 32, ..; fold_rows_and_store straight into `sums`
//   bwd_apply    the gather's thread shape over g and Y, written as bf16 into the padded interior
//   dmap         tile of 64 pixels x 64 channels: dXcat's map channels plus the at most 2 x 2 bins per scale that hold the
//                pixel, through the LDS tile to bn_tile.hpp's map side
#include "common.h"
#include "bn_taps.hpp"
#include "ppm_plan.hpp"

namespace {

using namespace memhip;
using namespace memhip::ppm;
using bn::kT, bn::kTile, bn::kPitch, bn::f4, bn::us8, bn::bf16_t, bn::bf2f, bn::f2bf;
using bn::clampi, bn::pad_at, bn::weight_of, bn::Chan8, bn::load8, bn::bn8;     // bn_taps.hpp: shared with fpn.hip
static_assert(kThreads == kT && kChunk == kTile && kPixels == kTile && kTileLdsBytes == kTile * kPitch * 4, "the plan's constants are the tile's");
constexpr int kN = MEMHIP_PPM_MAX_SCALES;

// what the kernels read of a memhip_ppm_args_t and its plan
struct Dev {
  int B, Cin, C, h, w, n, CT, P;     // CT = Cin + n C, P = h w
  long long R;                       // B P
  int s[kN], rows[kN], tile0[kN];
  const float* map; float* dmap;
  bf16_t* pool[kN]; const bf16_t* y[kN]; bf16_t* dy[kN]; const bf16_t* dp[kN]; float* g[kN];
  const float* mean; const float* rstd; const float* gamma; const float* beta;
  const int* y_i0[kN]; const float* y_w1[kN]; const int* y_lo[kN]; const int* y_hi[kN];
  const int* x_i0[kN]; const float* x_w1[kN]; const int* x_lo[kN]; const int* x_hi[kN];
  bf16_t* xcat; const bf16_t* dxcat;
  float* sums; const float* tot; float inv_n[kN];
};

// where the rows of Xcat lie (bn_tile.hpp: row_side)
struct CatRows {
  int h, w, P, CT;
  __device__ __forceinline__ long long operator()(long long r) const {
    const long long b = r / P;
    const int p = (int)(r - b * P), y = p / w;
    return pad_at(b, y, p - y * w, h, w, CT);
  }
};

// the vectors of channels c .. c + 7 of scale i
__device__ __forceinline__ Chan8 chan8(const Dev& d, int i, int c) {
  return bn::chan8(bn::BnParams{d.mean, d.rstd, d.gamma, d.beta}, i, d.C, c);
}

// ---------------------------------------------------------------- pool
// bin k of the bins of all scales, scale-major, row-major within a scale: its scale and its place there
__device__ __forceinline__ void locate_bin(const Dev& d, int k, int& i, int& by, int& bx) {
  i = 0;
  while (i < d.n - 1 && k >= d.s[i] * d.s[i]) { k -= d.s[i] * d.s[i]; ++i; }
  by = k / d.s[i];
  bx = k - by * d.s[i];
}

template <bool VEC>
__global__ __launch_bounds__(kT) void ppm_pool_kernel(Dev d, int nbins) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* tile = lds;                                                 // [64, 65]
  float* acc = tile + kTile * kPitch;                                // [nbins, 64]
  int* rect = reinterpret_cast<int*>(acc + nbins * kTile);           // [nbins, 4]: y0, y1, x0, x1
  const int t = threadIdx.x, c = t & 63, j = t >> 6;
  const int per = d.Cin / kTile, b = blockIdx.x / per, c0 = (blockIdx.x - b * per) * kTile;
  for (int k = t; k < nbins; k += kT) {
    int i, by, bx;
    locate_bin(d, k, i, by, bx);
    rect[4 * k + 0] = bin_start(by, d.h, d.s[i]); rect[4 * k + 1] = bin_end(by, d.h, d.s[i]);
    rect[4 * k + 2] = bin_start(bx, d.w, d.s[i]); rect[4 * k + 3] = bin_end(bx, d.w, d.s[i]);
  }
  // -0 + x = x for every x, the two zeros included: a bin of one pixel keeps the pixel's bits
  for (int k = j; k < nbins; k += 4) acc[k * kTile + c] = -0.f;
  const float* mp = d.map + (long long)b * d.Cin * d.P;
  for (int p0 = 0; p0 < d.P; p0 += kTile) {
    __syncthreads();                                                 // the rectangles are written; the previous tile's readers are done
    bn::map_side<VEC, true>(mp, d.Cin, d.P, (long long)d.P, (long long)p0, c0, tile);
    __syncthreads();
    const int ya = p0 / d.w, yb = min(p0 + kTile - 1, d.P - 1) / d.w;
    for (int k = j; k < nbins; k += 4) {
      const int y0 = max(rect[4 * k], ya), y1 = min(rect[4 * k + 1] - 1, yb), x0 = rect[4 * k + 2], x1 = rect[4 * k + 3];
      if (y0 > y1) continue;
      float a = acc[k * kTile + c];
      for (int y = y0; y <= y1; ++y)
        for (int x = x0; x < x1; ++x) {
          const int q = y * d.w + x - p0;
          if (q >= 0 && q < kTile) a += tile[q * kPitch + c];
        }
      acc[k * kTile + c] = a;
    }
  }
  __syncthreads();
  for (int e8 = t; e8 < nbins * 8; e8 += kT) {
    const int k = e8 >> 3, cg = e8 & 7;
    int i, by, bx;
    locate_bin(d, k, i, by, bx);
    const float cnt = (float)((rect[4 * k + 1] - rect[4 * k]) * (rect[4 * k + 3] - rect[4 * k + 2]));
    us8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(acc[k * kTile + 8 * cg + e] / cnt);
    *reinterpret_cast<us8*>(d.pool[i] + pad_at(b, by, bx, d.s[i], d.s[i], d.Cin) + c0 + 8 * cg) = o;
  }
}

// ---------------------------------------------------------------- concat, forward
template <bool VEC>
__global__ __launch_bounds__(kT) void ppm_concat_fwd_kernel(Dev d) {
  __shared__ float tile[kTile * kPitch];
  const long long z0 = (long long)blockIdx.x * kTile;
  const int t = threadIdx.x, nid = d.Cin / kTile;
  if ((int)blockIdx.y < nid) {                                       // the map's channels: seg_head.hip's mover, pitch CT
    const int c0 = blockIdx.y * kTile;
    bn::map_side<VEC, true>(d.map, d.Cin, d.P, d.R, z0, c0, tile);
    __syncthreads();
    bn::row_side<false>(d.xcat, d.R, CatRows{d.h, d.w, d.P, d.CT}, z0, c0, tile);
    return;
  }
  const int q = blockIdx.y - nid, per = d.C / kTile, i = q / per, cc = (q - i * per) * kTile + 8 * (t & 7), s = d.s[i];
  const Chan8 k8 = chan8(d, i, cc);
  const bf16_t* Y = d.y[i];
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    const long long r = z0 + (t >> 3) + 32 * half;
    if (r >= d.R) continue;
    const long long b = r / d.P;
    const int p = (int)(r - b * d.P), y = p / d.w, x = p - y * d.w;
    const int a0 = clampi(d.y_i0[i][y], 0, s - 1), a1 = min(a0 + 1, s - 1);
    const int b0 = clampi(d.x_i0[i][x], 0, s - 1), b1 = min(b0 + 1, s - 1);
    const float wy1 = d.y_w1[i][y], wy0 = 1.f - wy1, wx1 = d.x_w1[i][x], wx0 = 1.f - wx1;
    const us8 va = *reinterpret_cast<const us8*>(Y + pad_at(b, a0, b0, s, s, d.C) + cc);
    const us8 vb = *reinterpret_cast<const us8*>(Y + pad_at(b, a0, b1, s, s, d.C) + cc);
    const us8 vc = *reinterpret_cast<const us8*>(Y + pad_at(b, a1, b0, s, s, d.C) + cc);
    const us8 vd = *reinterpret_cast<const us8*>(Y + pad_at(b, a1, b1, s, s, d.C) + cc);
    float xh[8], ua[8], ub[8], uc[8], ud[8];
    bn8(va, k8, xh, ua); bn8(vb, k8, xh, ub); bn8(vc, k8, xh, uc); bn8(vd, k8, xh, ud);
    us8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      o[e] = f2bf(wy0 * (wx0 * fmaxf(ua[e], 0.f) + wx1 * fmaxf(ub[e], 0.f)) + wy1 * (wx0 * fmaxf(uc[e], 0.f) + wx1 * fmaxf(ud[e], 0.f)));
    *reinterpret_cast<us8*>(d.xcat + pad_at(b, y, x, d.h, d.w, d.CT) + d.Cin + i * d.C + cc) = o;
  }
}

// ---------------------------------------------------------------- concat, backward
// the (scale, row) of a thread of the gather's grid; false past the scale's last row
__device__ __forceinline__ bool locate_row(const Dev& d, int& i, int& row) {
  i = d.n - 1;
  while (i > 0 && (int)blockIdx.x < d.tile0[i]) --i;
  row = ((int)blockIdx.x - d.tile0[i]) * kRows + (threadIdx.x >> 3);
  return row < d.rows[i];
}

__global__ __launch_bounds__(kT) void ppm_gather_kernel(Dev d) {
  int i, row;
  if (!locate_row(d, i, row)) return;
  const int s = d.s[i], cc = blockIdx.y * kTile + 8 * (threadIdx.x & 7);
  const int b = row / (s * s), k = row - b * s * s, iy = k / s, ix = k - iy * s;
  const int ylo = max(d.y_lo[i][iy], 0), yhi = min(d.y_hi[i][iy], d.h - 1);
  const int xlo = max(d.x_lo[i][ix], 0), xhi = min(d.x_hi[i][ix], d.w - 1);
  const bf16_t* src = d.dxcat + d.Cin + i * d.C + cc;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int y = ylo; y <= yhi; ++y) {
    const int a0 = clampi(d.y_i0[i][y], 0, s - 1);
    const float wy = weight_of(iy, a0, min(a0 + 1, s - 1), d.y_w1[i][y]);
    for (int x = xlo; x <= xhi; ++x) {
      const int b0 = clampi(d.x_i0[i][x], 0, s - 1);
      const float wgt = wy * weight_of(ix, b0, min(b0 + 1, s - 1), d.x_w1[i][x]);
      const us8 v = *reinterpret_cast<const us8*>(src + pad_at(b, y, x, d.h, d.w, d.CT));
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(wgt, bf2f(v[e]), acc[e]);
    }
  }
  const us8 v = *reinterpret_cast<const us8*>(d.y[i] + pad_at(b, iy, ix, s, s, d.C) + cc);
  float xh[8], u[8];
  bn8(v, chan8(d, i, cc), xh, u);
  f4 g0, g1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    g0[e] = u[e] > 0.f ? acc[e] : 0.f;
    g1[e] = u[4 + e] > 0.f ? acc[4 + e] : 0.f;
  }
  float* dst = d.g[i] + (long long)row * d.C + cc;
  *reinterpret_cast<f4*>(dst) = g0;
  *reinterpret_cast<f4*>(dst + 4) = g1;
}

__global__ __launch_bounds__(kT) void ppm_sums_kernel(Dev d) {
  __shared__ float red[2 * 32 * 64];
  const int t = threadIdx.x, i = blockIdx.x, c0 = blockIdx.y * kTile, cc = c0 + 8 * (t & 7), s = d.s[i];
  const Chan8 k8 = chan8(d, i, cc);
  float a1[8], a2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a1[e] = a2[e] = 0.f;
  for (int row = t >> 3; row < d.rows[i]; row += 32) {
    const int b = row / (s * s), k = row - b * s * s, iy = k / s;
    const us8 v = *reinterpret_cast<const us8*>(d.y[i] + pad_at(b, iy, k - iy * s, s, s, d.C) + cc);
    float xh[8], u[8], g[8];
    bn8(v, k8, xh, u);
    load8(d.g[i] + (long long)row * d.C + cc, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      a1[e] += g[e];
      a2[e] = fmaf(g[e], xh[e], a2[e]);
    }
  }
  bn::fold_rows_and_store<32, 8>(a1, a2, red, d.sums + (long long)i * 2 * d.C, d.C, c0);
}

__global__ __launch_bounds__(kT) void ppm_bwd_apply_kernel(Dev d) {
  int i, row;
  if (!locate_row(d, i, row)) return;
  const int s = d.s[i], cc = blockIdx.y * kTile + 8 * (threadIdx.x & 7);
  const int b = row / (s * s), k = row - b * s * s, iy = k / s, ix = k - iy * s;
  const Chan8 k8 = chan8(d, i, cc);
  const long long off = pad_at(b, iy, ix, s, s, d.C) + cc;
  const us8 v = *reinterpret_cast<const us8*>(d.y[i] + off);
  float xh[8], u[8], g[8], m1[8], m2[8];
  bn8(v, k8, xh, u);
  load8(d.g[i] + (long long)row * d.C + cc, g);
#pragma unroll
  for (int e = 0; e < 8; ++e) m1[e] = m2[e] = 0.f;
  if (d.tot) {
    load8(d.tot + (long long)i * 2 * d.C + cc, m1);
    load8(d.tot + (long long)i * 2 * d.C + d.C + cc, m2);
#pragma unroll
    for (int e = 0; e < 8; ++e) { m1[e] *= d.inv_n[i]; m2[e] *= d.inv_n[i]; }
  }
  us8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = f2bf(k8.ga[e] * k8.rs[e] * (g[e] - m1[e] - xh[e] * m2[e]));
  *reinterpret_cast<us8*>(d.dy[i] + off) = o;
}

// ---------------------------------------------------------------- the map's gradient
template <bool VEC>
__global__ __launch_bounds__(kT) void ppm_dmap_kernel(Dev d) {
  __shared__ float tile[kTile * kPitch];
  const long long z0 = (long long)blockIdx.x * kTile;
  const int t = threadIdx.x, c0 = blockIdx.y * kTile, cg = 8 * (t & 7);
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    const int pl = (t >> 3) + 32 * half;
    const long long r = z0 + pl;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    if (r < d.R) {
      const long long b = r / d.P;
      const int p = (int)(r - b * d.P), y = p / d.w, x = p - y * d.w;
      const us8 v = *reinterpret_cast<const us8*>(d.dxcat + pad_at(b, y, x, d.h, d.w, d.CT) + c0 + cg);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = bf2f(v[e]);
      for (int i = 0; i < d.n; ++i) {
        const int s = d.s[i];
        const int by1 = min(bin_last(y, d.h, s), s - 1), bx1 = min(bin_last(x, d.w, s), s - 1);
        for (int by = bin_first(y, d.h, s); by <= by1; ++by)
          for (int bx = bin_first(x, d.w, s); bx <= bx1; ++bx) {
            const float cnt = (float)((bin_end(by, d.h, s) - bin_start(by, d.h, s)) * (bin_end(bx, d.w, s) - bin_start(bx, d.w, s)));
            const us8 q = *reinterpret_cast<const us8*>(d.dp[i] + pad_at(b, by, bx, s, s, d.Cin) + c0 + cg);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += bf2f(q[e]) / cnt;
          }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) tile[pl * kPitch + cg + e] = acc[e];
  }
  __syncthreads();
  bn::map_side<VEC, false>(d.dmap, d.Cin, d.P, d.R, z0, c0, tile);
}

// ---------------------------------------------------------------- host side
Dev dev_of(const memhip_ppm_args_t* a, const memhip_ppm_plan_t& p) {
  Dev d{};
  d.B = a->B; d.Cin = a->Cin; d.C = a->C; d.h = a->h; d.w = a->w; d.n = a->n; d.CT = p.ct; d.P = a->h * a->w; d.R = p.R;
  d.map = a->map; d.dmap = a->dmap;
  d.mean = a->mean; d.rstd = a->rstd; d.gamma = a->gamma; d.beta = a->beta;
  d.xcat = static_cast<bf16_t*>(a->xcat); d.dxcat = static_cast<const bf16_t*>(a->dxcat);
  d.sums = a->sums; d.tot = a->tot;
  for (int i = 0; i < a->n; ++i) {
    d.s[i] = a->scales[i]; d.rows[i] = p.rows[i]; d.tile0[i] = p.row_tile0[i];
    d.pool[i] = static_cast<bf16_t*>(a->P[i]); d.y[i] = static_cast<const bf16_t*>(a->Y[i]);
    d.dy[i] = static_cast<bf16_t*>(a->dY[i]); d.dp[i] = static_cast<const bf16_t*>(a->dP[i]); d.g[i] = a->g[i];
    d.y_i0[i] = a->y_i0[i]; d.y_w1[i] = a->y_w1[i]; d.y_lo[i] = a->y_lo[i]; d.y_hi[i] = a->y_hi[i];
    d.x_i0[i] = a->x_i0[i]; d.x_w1[i] = a->x_w1[i]; d.x_lo[i] = a->x_lo[i]; d.x_hi[i] = a->x_hi[i];
    d.inv_n[i] = a->inv_n[i];
  }
  return d;
}

// the map side moves 16 bytes per lane when the four pixels of a lane lie in one channel and the map is aligned
bool vec_map(const Dev& d, const float* map) { return d.P % 4 == 0 && bn::aligned(map, 16); }

}  // namespace

extern "C" int memhip_ppm_pool(const memhip_ppm_args_t* a, memhip_stream_t stream) {
  memhip_ppm_plan_t p;
  if (int rc = ppm_plan(a, PPM_POOL, &p)) return rc;
  if (p.R == 0) return MEMHIP_OK;
  const Dev d = dev_of(a, p);
  dispatch_bool(vec_map(d, d.map), [&](auto vec) {
    hipLaunchKernelGGL(ppm_pool_kernel<decltype(vec)::value>, dim3(p.pool_grid), dim3(p.block), p.pool_lds_bytes, as_stream(stream), d,
                       p.bins);
    return 0;
  });
  return check_launch("ppm_pool");
}

extern "C" int memhip_ppm_concat_fwd(const memhip_ppm_args_t* a, memhip_stream_t stream) {
  memhip_ppm_plan_t p;
  if (int rc = ppm_plan(a, PPM_CONCAT, &p)) return rc;
  if (p.R == 0) return MEMHIP_OK;
  const Dev d = dev_of(a, p);
  dispatch_bool(vec_map(d, d.map), [&](auto vec) {
    hipLaunchKernelGGL(ppm_concat_fwd_kernel<decltype(vec)::value>, dim3(p.concat_grid_x, p.concat_grid_y), dim3(p.block), 0,
                       as_stream(stream), d);
    return 0;
  });
  return check_launch("ppm_concat_fwd");
}

extern "C" int memhip_ppm_concat_bwd_sums(const memhip_ppm_args_t* a, memhip_stream_t stream) {
  memhip_ppm_plan_t p;
  if (int rc = ppm_plan(a, PPM_SUMS, &p)) return rc;
  if (p.R == 0) return MEMHIP_OK;
  const Dev d = dev_of(a, p);
  hipLaunchKernelGGL(ppm_gather_kernel, dim3(p.gather_grid_x, p.gather_grid_y), dim3(p.block), 0, as_stream(stream), d);
  hipLaunchKernelGGL(ppm_sums_kernel, dim3(p.sums_grid_x, p.sums_grid_y), dim3(p.block), 0, as_stream(stream), d);
  return check_launch("ppm_concat_bwd_sums");
}

extern "C" int memhip_ppm_bwd_apply(const memhip_ppm_args_t* a, memhip_stream_t stream) {
  memhip_ppm_plan_t p;
  if (int rc = ppm_plan(a, PPM_APPLY, &p)) return rc;
  if (p.R == 0) return MEMHIP_OK;
  const Dev d = dev_of(a, p);
  hipLaunchKernelGGL(ppm_bwd_apply_kernel, dim3(p.gather_grid_x, p.gather_grid_y), dim3(p.block), 0, as_stream(stream), d);
  return check_launch("ppm_bwd_apply");
}

extern "C" int memhip_ppm_dmap(const memhip_ppm_args_t* a, memhip_stream_t stream) {
  memhip_ppm_plan_t p;
  if (int rc = ppm_plan(a, PPM_DMAP, &p)) return rc;
  if (p.R == 0) return MEMHIP_OK;
  const Dev d = dev_of(a, p);
  dispatch_bool(vec_map(d, d.dmap), [&](auto vec) {
    hipLaunchKernelGGL(ppm_dmap_kernel<decltype(vec)::value>, dim3(p.dmap_grid_x, p.dmap_grid_y), dim3(p.block), 0, as_stream(stream), d);
    return 0;
  });
  return check_launch("ppm_dmap");
}
