// The DSEC segmentation data chain between the rasterizer and the backbone, image and label, batched on the GPU with
// PER-SAMPLE sizes and parameters (include/memhip.h: memhip_segdata_args_t).  The random draws stay on the host
// (mem_amd/seg_data.py); these kernels are the arithmetic of
//   Resize(ratio_range=(1.0, 1.01), keep_ratio=False)      mem/semantic_segmentation/configs/_base_/datasets/dsec.py:14
//   RemoveHotPixelsEvs                                      mem/semantic_segmentation/backbone/EventDataset.py:566-596
//   NormalizeEvs, ToUnit8Evs                                EventDataset.py:1339-1354, 1526-1535
//   RandomCrop, RandomFlip, Normalize(to_rgb), Pad          dsec.py:21-24
//   resize_in of the backbone                               mem/semantic_segmentation/backbone/mem.py:294,420
// Byte work (845 KB per 3 x 440 x 640 sample): one thread per pixel of a sample, the sample in blockIdx.y.  The resize is
// exact integer arithmetic; the normalisation and the final bilinear gather are the reference's separate fp32 operations
// (divide, multiply; multiply, add), so this translation unit is built with -ffp-contract=off (csrc/Makefile).
#include "common.h"

#pragma clang fp contract(off)

namespace {

using namespace memhip;

constexpr int kT = 256;

struct Sample { int h, w; long long off; bool ok; };

// dims / offs of sample b, validated against the bounds of the call: a bad sample is skipped, never addressed
__device__ __forceinline__ Sample sample_of(const int32_t* dims, const int64_t* offs, int b, int max_h, int max_w, long long elems) {
  Sample s;
  s.h = dims[2 * b];
  s.w = dims[2 * b + 1];
  s.off = offs[b];
  s.ok = s.h >= 1 && s.h <= max_h && s.w >= 1 && s.w <= max_w && s.off >= 0 && s.off + 3ll * s.h * s.w <= elems;
  return s;
}

// one axis of the exact resize: output i of n_out reads source taps i0, i1 of n_in with integer weights (2 n_out - f), f
__device__ __forceinline__ void axis_taps(int i, int n_in, int n_out, int& i0, int& i1, int& f) {
  int num = (2 * i + 1) * n_in - n_out;            // source position * 2 n_out; |num| < 2^31: n_in, n_out <= 4096
  const int den = 2 * n_out;
  if (num < 0) num = 0;
  if (num > (n_in - 1) * den) num = (n_in - 1) * den;
  i0 = num / den;
  f = num - i0 * den;
  i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
}

__global__ __launch_bounds__(kT) void resize_hist_kernel(const uint8_t* __restrict__ planes, int H, int W, const int64_t* __restrict__ offs,
                                                         const int32_t* __restrict__ dims, int max_h, int max_w, long long elems,
                                                         uint8_t* __restrict__ img, uint32_t* __restrict__ hist) {
  __shared__ uint32_t sh[512];
  const int b = blockIdx.y;
  const Sample s = sample_of(dims, offs, b, max_h, max_w, elems);
  if (!s.ok) return;                                // uniform over the workgroup
  const int npx = s.h * s.w;
  if ((long long)blockIdx.x * kT >= npx) return;    // uniform
  sh[threadIdx.x] = 0;
  sh[threadIdx.x + kT] = 0;
  __syncthreads();
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p < npx) {
    const int y = p / s.w, x = p - y * s.w;
    int y0, y1, fy, x0, x1, fx;
    axis_taps(y, H, s.h, y0, y1, fy);
    axis_taps(x, W, s.w, x0, x1, fx);
    // 64-bit: 255 * 4 h w passes 2^31 beyond 1448 x 1448
    const unsigned long long wy1 = fy, wy0 = 2 * s.h - fy, wx1 = fx, wx0 = 2 * s.w - fx;
    const unsigned long long half = 2ull * s.w * s.h, den = 4ull * s.w * s.h;
    const uint8_t* src = planes + (size_t)b * 3 * H * W;
    uint8_t* dst = img + s.off;
    uint32_t v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint8_t* pl = src + (size_t)c * H * W;
      const uint32_t a = pl[(size_t)y0 * W + x0], bb = pl[(size_t)y0 * W + x1];
      const uint32_t cc = pl[(size_t)y1 * W + x0], d = pl[(size_t)y1 * W + x1];
      v[c] = (uint32_t)((wy0 * (wx0 * a + wx1 * bb) + wy1 * (wx0 * cc + wx1 * d) + half) / den);
      dst[(size_t)c * npx + p] = (uint8_t)v[c];
    }
    atomicAdd(&sh[v[0]], 1u);
    atomicAdd(&sh[v[2]], 1u);
    atomicAdd(&sh[256 + (v[0] > v[2] ? v[0] : v[2])], 1u);
  }
  __syncthreads();
  uint32_t* hb = hist + (size_t)b * 512;
  for (int i = threadIdx.x; i < 512; i += kT)
    if (sh[i]) atomicAdd(&hb[i], sh[i]);
}

// thr and m of one sample from its 512 bins; every thread of the workgroup returns the same pair
__device__ __forceinline__ void hist_stats(const uint32_t* __restrict__ hb, double num_stds, double& thr, int& m) {
  __shared__ long long s_n[kT], s_1[kT], s_2[kT];
  __shared__ int s_m[kT];
  __shared__ double s_thr;
  const int k = threadIdx.x;                        // kT == 256: one bin per thread
  const long long c = hb[k];
  s_n[k] = c;
  s_1[k] = c * k;
  s_2[k] = c * k * k;
  __syncthreads();
  for (int st = kT / 2; st > 0; st >>= 1) {         // integer sums: any order gives the same value
    if (k < st) { s_n[k] += s_n[k + st]; s_1[k] += s_1[k + st]; s_2[k] += s_2[k + st]; }
    __syncthreads();
  }
  if (k == 0) {
    const long long n = s_n[0], S1 = s_1[0], S2 = s_2[0];
    double t = __builtin_inf();
    if (n >= 2) {
      const double mean = (double)S1 / (double)n;
      // n S2 - S1^2 <= 2^20 * 2^16 * 2^20 * 2: exact in int64 for every image up to 4096 x 4096
      const double var = (double)(n * S2 - S1 * S1) / ((double)n * (double)(n - 1));
      t = mean + num_stds * sqrt(var);
    }
    s_thr = t;
  }
  __syncthreads();
  thr = s_thr;
  s_m[k] = (hb[256 + k] != 0 && (double)k <= thr) ? k : 0;
  __syncthreads();
  for (int st = kT / 2; st > 0; st >>= 1) {
    if (k < st) s_m[k] = s_m[k] > s_m[k + st] ? s_m[k] : s_m[k + st];
    __syncthreads();
  }
  m = s_m[0] == 0 ? 1 : s_m[0];
}

template <bool F32>
__global__ __launch_bounds__(kT) void norm_kernel(const int64_t* __restrict__ offs, const int32_t* __restrict__ dims, int max_h, int max_w,
                                                  long long elems, uint8_t* __restrict__ img, float* __restrict__ imgf,
                                                  const uint32_t* __restrict__ hist, double num_stds) {
  const int b = blockIdx.y;
  const Sample s = sample_of(dims, offs, b, max_h, max_w, elems);
  if (!s.ok) return;
  const int npx = s.h * s.w;
  if ((long long)blockIdx.x * kT >= npx) return;
  double thr;
  int m;
  hist_stats(hist + (size_t)b * 512, num_stds, thr, m);
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= npx) return;
  uint8_t* px = img + s.off;
  int v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = px[(size_t)c * npx + p];
  if ((double)(v[0] > v[2] ? v[0] : v[2]) > thr) v[0] = v[2] = 0;
  const float fm = (float)m;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float q = (float)v[c] / fm;               // IEEE division (-fno-fast-math), then the multiply: two roundings
    const float r = q * 255.f;
    if (F32) imgf[s.off + (size_t)c * npx + p] = r;
    else px[(size_t)c * npx + p] = (uint8_t)(int)r;
  }
}

struct Crop { int top, left, flip, vh, vw; };

__device__ __forceinline__ Crop crop_of(const int32_t* crop, int b, const Sample& s, int crop_h, int crop_w) {
  Crop c;
  c.top = crop ? crop[3 * b] : 0;
  c.left = crop ? crop[3 * b + 1] : 0;
  c.flip = crop ? crop[3 * b + 2] != 0 : 0;
  c.top = c.top < 0 ? 0 : (c.top > s.h - 1 ? s.h - 1 : c.top);
  c.left = c.left < 0 ? 0 : (c.left > s.w - 1 ? s.w - 1 : c.left);
  c.vh = s.h - c.top < crop_h ? s.h - c.top : crop_h;      // rows / columns of the window that the image covers
  c.vw = s.w - c.left < crop_w ? s.w - c.left : crop_w;
  return c;
}

// F.interpolate(mode='bilinear', align_corners=False): the source position (in / out) (i + 0.5) - 0.5, clamped at 0, as the
// exact rational ((2 i + 1) in - out) / (2 out).  aten's area_pixel_compute_source_index evaluates it in the tensor's
// precision; in fp32 its position is off by up to in * 2^-23, which the weight inherits ABSOLUTELY (640 * 2^-23 * 255 = 0.02 in
// the output).  Here the tap is an integer division and the weight its remainder, rounded once.
__device__ __forceinline__ void net_taps(int i, int n_in, int n_out, int& i0, int& i1, float& w1) {
  int num = (2 * i + 1) * n_in - n_out;             // |num| < 2^31: n_in, n_out <= 4096
  const int den = 2 * n_out;
  if (num < 0) num = 0;
  i0 = num / den;                                   // <= n_in - 1
  i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
  w1 = (float)(num - i0 * den) / (float)den;
}

template <bool F32>
__global__ __launch_bounds__(kT) void geom_image_kernel(const int64_t* __restrict__ offs, const int32_t* __restrict__ dims, int max_h,
                                                        int max_w, long long elems, const uint8_t* __restrict__ img,
                                                        const float* __restrict__ imgf, const int32_t* __restrict__ crop, int crop_h,
                                                        int crop_w, int net_h, int net_w, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= net_h * net_w) return;
  float* o = out + (size_t)b * 3 * net_h * net_w + p;
  const Sample s = sample_of(dims, offs, b, max_h, max_w, elems);
  if (!s.ok) {
    for (int c = 0; c < 3; ++c) o[(size_t)c * net_h * net_w] = 0.f;
    return;
  }
  const Crop cr = crop_of(crop, b, s, crop_h, crop_w);
  const int oy = p / net_w, ox = p - oy * net_w;
  int y0, y1, x0, x1;
  float wy1, wx1;
  net_taps(oy, crop_h, net_h, y0, y1, wy1);
  net_taps(ox, crop_w, net_w, x0, x1, wx1);
  const float wy0 = 1.f - wy1, wx0 = 1.f - wx1;
  const int npx = s.h * s.w;
  const int ys[2] = {y0, y1}, xs[2] = {x0, x1};
  long long idx[2][2];                              // element of channel 0 behind tap (j, i), -1: padding
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int py = ys[j], pxx = xs[i];
      if (py >= cr.vh || pxx >= cr.vw) { idx[j][i] = -1; continue; }
      const int sx = cr.flip ? cr.vw - 1 - pxx : pxx;
      idx[j][i] = (long long)(cr.top + py) * s.w + cr.left + sx;
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t base = (size_t)s.off + (size_t)(2 - c) * npx;      // to_rgb: channels 0 and 2 swap
    float t[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i)
        t[j][i] = idx[j][i] < 0 ? 0.f : (F32 ? imgf[base + idx[j][i]] : (float)img[base + idx[j][i]]);
    o[(size_t)c * net_h * net_w] = wy0 * (wx0 * t[0][0] + wx1 * t[0][1]) + wy1 * (wx0 * t[1][0] + wx1 * t[1][1]);
  }
}

__global__ __launch_bounds__(kT) void geom_label_kernel(const uint8_t* __restrict__ labels, int H, int W, const int64_t* __restrict__ offs,
                                                        const int32_t* __restrict__ dims, int max_h, int max_w, long long elems,
                                                        const int32_t* __restrict__ crop, int crop_h, int crop_w,
                                                        uint8_t* __restrict__ out) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= crop_h * crop_w) return;
  uint8_t* o = out + (size_t)b * crop_h * crop_w + p;
  const Sample s = sample_of(dims, offs, b, max_h, max_w, elems);
  if (!s.ok) { *o = 255; return; }
  const Crop cr = crop_of(crop, b, s, crop_h, crop_w);
  const int y = p / crop_w, x = p - y * crop_w;
  if (y >= cr.vh || x >= cr.vw) { *o = 255; return; }
  const int ry = cr.top + y, rx = cr.left + (cr.flip ? cr.vw - 1 - x : x);
  int sy = (int)((long long)ry * H / s.h), sx = (int)((long long)rx * W / s.w);
  if (sy > H - 1) sy = H - 1;
  if (sx > W - 1) sx = W - 1;
  *o = labels[((size_t)b * H + sy) * W + sx];
}

int check_common(const memhip_segdata_args_t* a, const char* who) {
  MEMHIP_REQUIRE(a, "%s: null args", who);
  MEMHIP_REQUIRE(a->B >= 0 && a->B <= 65535, "%s: B=%d must be 0 .. 65535", who, a->B);
  MEMHIP_REQUIRE(a->max_h >= 1 && a->max_h <= 4096 && a->max_w >= 1 && a->max_w <= 4096,
                 "%s: max_h=%d max_w=%d must be 1 .. 4096", who, a->max_h, a->max_w);
  MEMHIP_REQUIRE(a->img_elems >= 0, "%s: img_elems=%lld must be >= 0", who, (long long)a->img_elems);
  if (a->B > 0) MEMHIP_REQUIRE(a->offs && a->dims, "%s: offs and dims must be given", who);
  return MEMHIP_OK;
}

}  // namespace

extern "C" int memhip_segdata_resize_hist(const memhip_segdata_args_t* a, memhip_stream_t stream) {
  if (int rc = check_common(a, "segdata_resize_hist")) return rc;
  MEMHIP_REQUIRE(a->H >= 1 && a->H <= 4096 && a->W >= 1 && a->W <= 4096, "segdata_resize_hist: H=%d W=%d must be 1 .. 4096", a->H, a->W);
  if (a->B == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(a->planes && a->img_u8 && a->hist, "segdata_resize_hist: planes, img_u8 and hist must be given");
  MEMHIP_HIP(hipMemsetAsync(a->hist, 0, (size_t)a->B * 512 * sizeof(uint32_t), as_stream(stream)));
  hipLaunchKernelGGL(resize_hist_kernel, dim3(cdiv((long long)a->max_h * a->max_w, kT), a->B), dim3(kT), 0, as_stream(stream),
                     a->planes, a->H, a->W, a->offs, a->dims, a->max_h, a->max_w, (long long)a->img_elems, a->img_u8, a->hist);
  return check_launch("segdata_resize_hist");
}

extern "C" int memhip_segdata_norm(const memhip_segdata_args_t* a, memhip_stream_t stream) {
  if (int rc = check_common(a, "segdata_norm")) return rc;
  MEMHIP_REQUIRE(a->out_f32 == 0 || a->out_f32 == 1, "segdata_norm: out_f32=%d must be 0 or 1", a->out_f32);
  MEMHIP_REQUIRE(a->num_stds >= 0.0, "segdata_norm: num_stds=%g must be >= 0", a->num_stds);
  if (a->B == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(a->img_u8 && a->hist, "segdata_norm: img_u8 and hist must be given");
  MEMHIP_REQUIRE(!a->out_f32 || a->img_f32, "segdata_norm: out_f32 needs img_f32");
  const dim3 grid(cdiv((long long)a->max_h * a->max_w, kT), a->B);
  if (a->out_f32)
    hipLaunchKernelGGL(norm_kernel<true>, grid, dim3(kT), 0, as_stream(stream), a->offs, a->dims, a->max_h, a->max_w,
                       (long long)a->img_elems, a->img_u8, a->img_f32, a->hist, a->num_stds);
  else
    hipLaunchKernelGGL(norm_kernel<false>, grid, dim3(kT), 0, as_stream(stream), a->offs, a->dims, a->max_h, a->max_w,
                       (long long)a->img_elems, a->img_u8, a->img_f32, a->hist, a->num_stds);
  return check_launch("segdata_norm");
}

extern "C" int memhip_segdata_geom(const memhip_segdata_args_t* a, memhip_stream_t stream) {
  if (int rc = check_common(a, "segdata_geom")) return rc;
  MEMHIP_REQUIRE(a->crop_h >= 1 && a->crop_h <= 4096 && a->crop_w >= 1 && a->crop_w <= 4096,
                 "segdata_geom: crop_h=%d crop_w=%d must be 1 .. 4096", a->crop_h, a->crop_w);
  MEMHIP_REQUIRE(a->in_f32 == 0 || a->in_f32 == 1, "segdata_geom: in_f32=%d must be 0 or 1", a->in_f32);
  if (a->out) {
    MEMHIP_REQUIRE(a->net_h >= 1 && a->net_h <= 4096 && a->net_w >= 1 && a->net_w <= 4096,
                   "segdata_geom: net_h=%d net_w=%d must be 1 .. 4096", a->net_h, a->net_w);
  }
  if (a->label_out) {
    MEMHIP_REQUIRE(a->H >= 1 && a->H <= 4096 && a->W >= 1 && a->W <= 4096, "segdata_geom: H=%d W=%d must be 1 .. 4096", a->H, a->W);
  }
  MEMHIP_REQUIRE(a->out || a->label_out, "segdata_geom: neither out nor label_out");
  if (a->B == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(!a->out || (a->in_f32 ? a->img_f32 != nullptr : a->img_u8 != nullptr),
                 "segdata_geom: the image buffer in_f32 selects is NULL");
  MEMHIP_REQUIRE(!a->label_out || a->labels, "segdata_geom: label_out needs labels");
  if (a->out) {
    const dim3 grid(cdiv((long long)a->net_h * a->net_w, kT), a->B);
    if (a->in_f32)
      hipLaunchKernelGGL(geom_image_kernel<true>, grid, dim3(kT), 0, as_stream(stream), a->offs, a->dims, a->max_h, a->max_w,
                         (long long)a->img_elems, a->img_u8, a->img_f32, a->crop, a->crop_h, a->crop_w, a->net_h, a->net_w, a->out);
    else
      hipLaunchKernelGGL(geom_image_kernel<false>, grid, dim3(kT), 0, as_stream(stream), a->offs, a->dims, a->max_h, a->max_w,
                         (long long)a->img_elems, a->img_u8, a->img_f32, a->crop, a->crop_h, a->crop_w, a->net_h, a->net_w, a->out);
    if (int rc = check_launch("segdata_geom (image)")) return rc;
  }
  if (a->label_out) {
    hipLaunchKernelGGL(geom_label_kernel, dim3(cdiv((long long)a->crop_h * a->crop_w, kT), a->B), dim3(kT), 0, as_stream(stream),
                       a->labels, a->H, a->W, a->offs, a->dims, a->max_h, a->max_w, (long long)a->img_elems, a->crop, a->crop_h,
                       a->crop_w, a->label_out);
    if (int rc = check_launch("segdata_geom (label)")) return rc;
  }
  return MEMHIP_OK;
}
