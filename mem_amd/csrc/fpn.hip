// The FPN part of the UPerNet decode head (mmseg 0.30 mmseg/models/decode_heads/uper_head.py, UPerHead.forward between its
// convolutions; decode_head = dict(type='UPerHead', in_index=[0, 1, 2, 3], channels=512):
// mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:25-37): the top-down path, the resize + concat into
// fpn_bottleneck's operand, and the transposes of both for the backward, with the batch-norm + ReLU of the lateral, FPN and
// pyramid-bottleneck ConvModules evaluated on the fly from their stored convolution outputs.  The convolutions, their data and
// weight gradients and the batch statistics are conv.hip / conv_wgrad.hip / seg_head.hip on the activation format bf16
// [B, m+2, m'+2, channels].
//
// Every kernel streams: 256 threads, a thread owns 8 channels (16 bytes of bf16) of one pixel, 8 neighbouring lanes the 128
// bytes of 64 channels; the parallelism is that of the level's pixels.  Rings are neither read nor written.  No float atomics:
// every sum is one thread's chain in an order the shapes fix, the channel sums two-stage as in bn_tile.hpp.
//
//   topdown_fwd  grid (tiles of 64 pixels of level l, C / 64): batch norm + ReLU of the lateral's output at the pixel, the four
//                taps of the coarser level (the stored T_{l+1}, or batch norm + ReLU of the pyramid bottleneck's output at each
//                tap), the bilinear combination, one 16-byte store
//   concat_fwd   grid (tiles of 64 pixels of level 0, L C / 64): ppm.hip's gather on Y[l] with the tables (l -> 0)
//   resize_bwd   grid (tiles of 32 destination pixels, C / 64): own term, then the outputs lo .. hi of both axes in ascending
//                order of each source, the weight of each from the tables the forward read; fp32 rows, ungated
//   bn_bwd_sums  grid (G, C / 64): row lane t / 8 chains over the rows 32 g + j, + 32 G, ..; fold_rows_and_store; launch_fold
//   bn_bwd_apply grid (tiles of 64 pixels, C / 64): the gate from the stored Y, bf16 into the padded interior
#include "common.h"
#include "bn_taps.hpp"
#include "fpn_plan.hpp"

namespace {

using namespace memhip;
using namespace memhip::fpn;
using bn::kT, bn::kTile, bn::f4, bn::us8, bn::bf16_t, bn::bf2f, bn::f2bf, bn::BnParams, bn::FoldOut;
using bn::clampi, bn::pad_at, bn::weight_of, bn::Chan8, bn::chan8, bn::load8, bn::bn8, bn::Tap, bn::tap_of, bn::bilerp;
static_assert(kThreads == kT && kChunk == kTile && kPixels == kTile && fpn::kGroups == bn::kGroups, "the plan's constants are the tile's");

struct Axis { const int* i0; const float* w1; const int* lo; const int* hi; };

__device__ __forceinline__ us8 ld8(const bf16_t* p) { return *reinterpret_cast<const us8*>(p); }

// pixel r of a level of h x w pixels: sample, row, column
__device__ __forceinline__ void locate(long long r, int h, int w, long long& b, int& y, int& x) {
  const int P = h * w;
  b = r / P;
  const int p = (int)(r - b * P);
  y = p / w;
  x = p - y * w;
}

// relu(u) of 8 channels of one stored pixel
__device__ __forceinline__ void act8(const us8& v, const Chan8& k, float (&z)[8]) {
  float xh[8];
  bn8(v, k, xh, z);
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = fmaxf(z[e], 0.f);
}

__device__ __forceinline__ void cvt8(const us8& v, float (&z)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = bf2f(v[e]);
}

// ---------------------------------------------------------------- top-down step, forward
struct TopdownP {
  int C, h, w, hs, ws, level;        // hs x ws: the coarser level
  long long R;
  const bf16_t* y; const bf16_t* src; const bf16_t* ysrc; bf16_t* T;
  BnParams v;
  Axis ay, ax;
};

template <bool ACT>                  // the source is a stored convolution output: batch norm + ReLU at each tap
__global__ __launch_bounds__(kT) void fpn_topdown_kernel(TopdownP p) {
  const int t = threadIdx.x, cc = blockIdx.y * kTile + 8 * (t & 7);
  const Chan8 k8 = chan8(p.v, p.level, p.C, cc);
  const Chan8 ks = ACT ? chan8(p.v, p.level + 1, p.C, cc) : k8;
  const bf16_t* S = ACT ? p.ysrc : p.src;
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    const long long r = (long long)blockIdx.x * kTile + (t >> 3) + 32 * half;
    if (r >= p.R) continue;
    long long b;
    int y, x;
    locate(r, p.h, p.w, b, y, x);
    const Tap ty = tap_of(p.ay.i0, p.ay.w1, y, p.hs), tx = tap_of(p.ax.i0, p.ax.w1, x, p.ws);
    const us8 va = ld8(S + pad_at(b, ty.i0, tx.i0, p.hs, p.ws, p.C) + cc), vb = ld8(S + pad_at(b, ty.i0, tx.i1, p.hs, p.ws, p.C) + cc);
    const us8 vc = ld8(S + pad_at(b, ty.i1, tx.i0, p.hs, p.ws, p.C) + cc), vd = ld8(S + pad_at(b, ty.i1, tx.i1, p.hs, p.ws, p.C) + cc);
    const long long off = pad_at(b, y, x, p.h, p.w, p.C) + cc;
    const us8 vy = ld8(p.y + off);
    float za[8], zb[8], zc[8], zd[8], z[8];
    if constexpr (ACT) {
      act8(va, ks, za); act8(vb, ks, zb); act8(vc, ks, zc); act8(vd, ks, zd);
    } else {
      cvt8(va, za); cvt8(vb, zb); cvt8(vc, zc); cvt8(vd, zd);
    }
    act8(vy, k8, z);
    us8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(z[e] + bilerp(ty, tx, za[e], zb[e], zc[e], zd[e]));
    *reinterpret_cast<us8*>(p.T + off) = o;
  }
}

// ---------------------------------------------------------------- concat, forward
struct ConcatP {
  int C, L, CT;
  long long R;                       // pixels of level 0
  int h[MEMHIP_FPN_MAX_LEVELS], w[MEMHIP_FPN_MAX_LEVELS];
  const bf16_t* y[MEMHIP_FPN_MAX_LEVELS];
  Axis ay[MEMHIP_FPN_MAX_LEVELS], ax[MEMHIP_FPN_MAX_LEVELS];
  BnParams v;
  bf16_t* xcat;
};

__global__ __launch_bounds__(kT) void fpn_concat_fwd_kernel(ConcatP p) {
  const int t = threadIdx.x, per = p.C / kTile, l = blockIdx.y / per, cc = (blockIdx.y - l * per) * kTile + 8 * (t & 7);
  const int hs = p.h[l], ws = p.w[l];
  const Chan8 k8 = chan8(p.v, l, p.C, cc);
  const bf16_t* Y = p.y[l];
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    const long long r = (long long)blockIdx.x * kTile + (t >> 3) + 32 * half;
    if (r >= p.R) continue;
    long long b;
    int y, x;
    locate(r, p.h[0], p.w[0], b, y, x);
    const Tap ty = tap_of(p.ay[l].i0, p.ay[l].w1, y, hs), tx = tap_of(p.ax[l].i0, p.ax[l].w1, x, ws);
    const us8 va = ld8(Y + pad_at(b, ty.i0, tx.i0, hs, ws, p.C) + cc), vb = ld8(Y + pad_at(b, ty.i0, tx.i1, hs, ws, p.C) + cc);
    const us8 vc = ld8(Y + pad_at(b, ty.i1, tx.i0, hs, ws, p.C) + cc), vd = ld8(Y + pad_at(b, ty.i1, tx.i1, hs, ws, p.C) + cc);
    float za[8], zb[8], zc[8], zd[8];
    act8(va, k8, za); act8(vb, k8, zb); act8(vc, k8, zc); act8(vd, k8, zd);
    us8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(bilerp(ty, tx, za[e], zb[e], zc[e], zd[e]));
    *reinterpret_cast<us8*>(p.xcat + pad_at(b, y, x, p.h[0], p.w[0], p.CT) + l * p.C + cc) = o;
  }
}

// ---------------------------------------------------------------- the transposed resizes
struct ResizeP {
  int C, h, w;                       // the destination
  long long R;
  const bf16_t* own;
  const bf16_t* dxcat; int CT, c_off, h0, w0; Axis cy, cx;
  const float* fine; int hf, wf; Axis ty, tx;
  float* rows;
};

__global__ __launch_bounds__(kT) void fpn_resize_bwd_kernel(ResizeP p) {
  const int t = threadIdx.x, cc = blockIdx.y * kTile + 8 * (t & 7);
  const long long row = (long long)blockIdx.x * kRows + (t >> 3);
  if (row >= p.R) return;
  long long b;
  int iy, ix;
  locate(row, p.h, p.w, b, iy, ix);
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (p.own) cvt8(ld8(p.own + pad_at(b, iy, ix, p.h, p.w, p.C) + cc), acc);
  if (p.dxcat) {
    const int ylo = max(p.cy.lo[iy], 0), yhi = min(p.cy.hi[iy], p.h0 - 1);
    const int xlo = max(p.cx.lo[ix], 0), xhi = min(p.cx.hi[ix], p.w0 - 1);
    const bf16_t* src = p.dxcat + p.c_off + cc;
    for (int y = ylo; y <= yhi; ++y) {
      const int a0 = clampi(p.cy.i0[y], 0, p.h - 1);
      const float wy = weight_of(iy, a0, min(a0 + 1, p.h - 1), p.cy.w1[y]);
      for (int x = xlo; x <= xhi; ++x) {
        const int b0 = clampi(p.cx.i0[x], 0, p.w - 1);
        const float wgt = wy * weight_of(ix, b0, min(b0 + 1, p.w - 1), p.cx.w1[x]);
        const us8 v = ld8(src + pad_at(b, y, x, p.h0, p.w0, p.CT));
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(wgt, bf2f(v[e]), acc[e]);
      }
    }
  }
  if (p.fine) {
    const int ylo = max(p.ty.lo[iy], 0), yhi = min(p.ty.hi[iy], p.hf - 1);
    const int xlo = max(p.tx.lo[ix], 0), xhi = min(p.tx.hi[ix], p.wf - 1);
    for (int y = ylo; y <= yhi; ++y) {
      const int a0 = clampi(p.ty.i0[y], 0, p.h - 1);
      const float wy = weight_of(iy, a0, min(a0 + 1, p.h - 1), p.ty.w1[y]);
      for (int x = xlo; x <= xhi; ++x) {
        const int b0 = clampi(p.tx.i0[x], 0, p.w - 1);
        const float wgt = wy * weight_of(ix, b0, min(b0 + 1, p.w - 1), p.tx.w1[x]);
        float v[8];
        load8(p.fine + ((b * p.hf + y) * p.wf + x) * p.C + cc, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(wgt, v[e], acc[e]);
      }
    }
  }
  f4 g0, g1;
#pragma unroll
  for (int e = 0; e < 4; ++e) { g0[e] = acc[e]; g1[e] = acc[4 + e]; }
  float* dst = p.rows + row * p.C + cc;
  *reinterpret_cast<f4*>(dst) = g0;
  *reinterpret_cast<f4*>(dst + 4) = g1;
}

// ---------------------------------------------------------------- batch norm + ReLU, backward
struct BnP {
  int C, h, w, level;
  long long R;
  const bf16_t* y; const float* rows;
  BnParams v;
  float* ws;                         // _sums
  const float* tot; float inv_n; bf16_t* dy;     // _apply
};

// g = rows (u > 0) and xhat of 8 channels of pixel r
__device__ __forceinline__ void gate8(const BnP& p, const Chan8& k8, long long r, long long off, int cc, float (&g)[8], float (&xh)[8]) {
  float u[8];
  bn8(ld8(p.y + off), k8, xh, u);
  load8(p.rows + r * p.C + cc, g);
#pragma unroll
  for (int e = 0; e < 8; ++e) g[e] = u[e] > 0.f ? g[e] : 0.f;
}

__global__ __launch_bounds__(kT) void fpn_bn_bwd_sums_kernel(BnP p) {
  __shared__ float red[2 * kRows * kTile];
  const int t = threadIdx.x, c0 = blockIdx.y * kTile, cc = c0 + 8 * (t & 7);
  const Chan8 k8 = chan8(p.v, p.level, p.C, cc);
  float a1[8], a2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a1[e] = a2[e] = 0.f;
  for (long long r = (long long)blockIdx.x * kRows + (t >> 3); r < p.R; r += (long long)kRows * gridDim.x) {
    long long b;
    int y, x;
    locate(r, p.h, p.w, b, y, x);
    float g[8], xh[8];
    gate8(p, k8, r, pad_at(b, y, x, p.h, p.w, p.C) + cc, cc, g, xh);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      a1[e] += g[e];
      a2[e] = fmaf(g[e], xh[e], a2[e]);
    }
  }
  bn::fold_rows_and_store<kRows, 8>(a1, a2, red, p.ws + (long long)blockIdx.x * 2 * p.C, p.C, c0);
}

__global__ __launch_bounds__(kT) void fpn_bn_bwd_apply_kernel(BnP p) {
  const int t = threadIdx.x, cc = blockIdx.y * kTile + 8 * (t & 7);
  const Chan8 k8 = chan8(p.v, p.level, p.C, cc);
  float m1[8], m2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) m1[e] = m2[e] = 0.f;
  if (p.tot) {
    load8(p.tot + cc, m1);
    load8(p.tot + p.C + cc, m2);
#pragma unroll
    for (int e = 0; e < 8; ++e) { m1[e] *= p.inv_n; m2[e] *= p.inv_n; }
  }
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    const long long r = (long long)blockIdx.x * kTile + (t >> 3) + 32 * half;
    if (r >= p.R) continue;
    long long b;
    int y, x;
    locate(r, p.h, p.w, b, y, x);
    const long long off = pad_at(b, y, x, p.h, p.w, p.C) + cc;
    float g[8], xh[8];
    gate8(p, k8, r, off, cc, g, xh);
    us8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(k8.ga[e] * k8.rs[e] * (g[e] - m1[e] - xh[e] * m2[e]));
    *reinterpret_cast<us8*>(p.dy + off) = o;
  }
}

// ---------------------------------------------------------------- host side
BnParams vectors_of(const memhip_fpn_args_t* a) { return BnParams{a->mean, a->rstd, a->gamma, a->beta}; }
const bf16_t* bf(const void* p) { return static_cast<const bf16_t*>(p); }

BnP bn_of(const memhip_fpn_args_t* a, const memhip_fpn_plan_t& p) {
  BnP k{};
  const int l = a->level;
  k.C = a->C; k.h = a->h[l]; k.w = a->w[l]; k.level = l; k.R = p.R[l];
  k.y = bf(a->Y[l]); k.rows = a->rows; k.v = vectors_of(a);
  k.ws = static_cast<float*>(a->workspace);
  k.tot = a->tot; k.inv_n = a->inv_n; k.dy = static_cast<bf16_t*>(a->dY);
  return k;
}

}  // namespace

extern "C" int memhip_fpn_topdown_fwd(const memhip_fpn_args_t* a, memhip_stream_t stream) {
  memhip_fpn_plan_t p;
  if (int rc = fpn_plan(a, FPN_TOPDOWN, &p)) return rc;
  const int l = a->level;
  if (p.R[l] == 0) return MEMHIP_OK;
  TopdownP k{};
  k.C = a->C; k.h = a->h[l]; k.w = a->w[l]; k.hs = a->h[l + 1]; k.ws = a->w[l + 1]; k.level = l; k.R = p.R[l];
  k.y = bf(a->Y[l]); k.src = bf(a->src); k.ysrc = a->src ? nullptr : bf(a->Y[l + 1]); k.T = static_cast<bf16_t*>(a->T);
  k.v = vectors_of(a);
  k.ay = Axis{a->ty_i0[l], a->ty_w1[l], nullptr, nullptr};
  k.ax = Axis{a->tx_i0[l], a->tx_w1[l], nullptr, nullptr};
  dispatch_bool(a->src == nullptr, [&](auto act) {
    hipLaunchKernelGGL(fpn_topdown_kernel<decltype(act)::value>, dim3(p.topdown_grid_x[l], p.grid_y), dim3(p.block), 0, as_stream(stream), k);
    return 0;
  });
  return check_launch("fpn_topdown_fwd");
}

extern "C" int memhip_fpn_concat_fwd(const memhip_fpn_args_t* a, memhip_stream_t stream) {
  memhip_fpn_plan_t p;
  if (int rc = fpn_plan(a, FPN_CONCAT, &p)) return rc;
  if (p.R[0] == 0) return MEMHIP_OK;
  ConcatP k{};
  k.C = a->C; k.L = a->L; k.CT = p.ct; k.R = p.R[0];
  for (int l = 0; l < a->L; ++l) {
    k.h[l] = a->h[l]; k.w[l] = a->w[l]; k.y[l] = bf(a->Y[l]);
    k.ay[l] = Axis{a->cy_i0[l], a->cy_w1[l], nullptr, nullptr};
    k.ax[l] = Axis{a->cx_i0[l], a->cx_w1[l], nullptr, nullptr};
  }
  k.v = vectors_of(a);
  k.xcat = static_cast<bf16_t*>(a->xcat);
  hipLaunchKernelGGL(fpn_concat_fwd_kernel, dim3(p.concat_grid_x, p.concat_grid_y), dim3(p.block), 0, as_stream(stream), k);
  return check_launch("fpn_concat_fwd");
}

extern "C" int memhip_fpn_resize_bwd(const memhip_fpn_args_t* a, memhip_stream_t stream) {
  memhip_fpn_plan_t p;
  if (int rc = fpn_plan(a, FPN_RESIZE, &p)) return rc;
  const int l = a->level;
  if (p.R[l] == 0) return MEMHIP_OK;
  ResizeP k{};
  k.C = a->C; k.h = a->h[l]; k.w = a->w[l]; k.R = p.R[l];
  k.own = bf(a->own);
  k.dxcat = bf(a->dxcat); k.CT = p.ct; k.c_off = a->slice * a->C; k.h0 = a->h[0]; k.w0 = a->w[0];
  if (a->dxcat) {
    k.cy = Axis{a->cy_i0[l], a->cy_w1[l], a->cy_lo[l], a->cy_hi[l]};
    k.cx = Axis{a->cx_i0[l], a->cx_w1[l], a->cx_lo[l], a->cx_hi[l]};
  }
  k.fine = a->fine_rows;
  if (a->fine_rows) {
    k.hf = a->h[l - 1]; k.wf = a->w[l - 1];
    k.ty = Axis{a->ty_i0[l - 1], a->ty_w1[l - 1], a->ty_lo[l - 1], a->ty_hi[l - 1]};
    k.tx = Axis{a->tx_i0[l - 1], a->tx_w1[l - 1], a->tx_lo[l - 1], a->tx_hi[l - 1]};
  }
  k.rows = a->rows;
  hipLaunchKernelGGL(fpn_resize_bwd_kernel, dim3(p.resize_grid_x[l], p.grid_y), dim3(p.block), 0, as_stream(stream), k);
  return check_launch("fpn_resize_bwd");
}

extern "C" int memhip_fpn_bn_bwd_sums(const memhip_fpn_args_t* a, memhip_stream_t stream) {
  memhip_fpn_plan_t p;
  if (int rc = fpn_plan(a, FPN_SUMS, &p)) return rc;
  const int l = a->level;
  if (p.R[l] == 0) return MEMHIP_OK;
  const BnP k = bn_of(a, p);
  hipLaunchKernelGGL(fpn_bn_bwd_sums_kernel, dim3(p.sums_grid_x[l], p.grid_y), dim3(p.block), 0, as_stream(stream), k);
  bn::launch_fold(k.ws, p.sums_grid_x[l], p.slot_floats, p.fold_grid, FoldOut{{a->sums, nullptr, nullptr}, {p.slot_floats, 0, 0}, nullptr, 0, 0.f},
                  as_stream(stream));
  return check_launch("fpn_bn_bwd_sums");
}

extern "C" int memhip_fpn_bn_bwd_apply(const memhip_fpn_args_t* a, memhip_stream_t stream) {
  memhip_fpn_plan_t p;
  if (int rc = fpn_plan(a, FPN_APPLY, &p)) return rc;
  const int l = a->level;
  if (p.R[l] == 0) return MEMHIP_OK;
  const BnP k = bn_of(a, p);
  hipLaunchKernelGGL(fpn_bn_bwd_apply_kernel, dim3(p.apply_grid_x[l], p.grid_y), dim3(p.block), 0, as_stream(stream), k);
  return check_launch("fpn_bn_bwd_apply");
}
