// Which kernels take a memhip_conv2d_nhwc_bf16 / _f32 / _f32_dyn / _f16x2 call, with which grids, workgroup sizes and LDS
// bytes: conv_geom is the one place that derives a layer's geometry, conv_validate the one place that accepts or rejects a
// call, conv_plan (conv_plan.cpp) the one place that decides the dispatch -- once per call, from the geometry, the flags of
// the call, the device's CU count and a snapshot of the options.  Host arithmetic only: memhip_conv_plan returns the same
// plan without a device (tests/test_conv_plan_cpu.py checks it against the cascades it replaced).
#pragma once
#include <cstdint>
#include "../../include/memhip.h"

namespace memhip {

// ---- tiles, workgroup sizes and dynamic LDS bytes of the convolution kernels (each file asserts them against its own
// constants): rows x columns of outputs per workgroup
constexpr int kConvTileM = 128, kConvTileN = 128;      // conv.hip, conv_f32.hip, conv_f16x2.hip <4> / <8> / first layer
constexpr int kConvF32SmallM = 32;                     // conv_gemm_f32_m32_kernel
constexpr int kConvWideM = 256;                        // conv_gemm_f16x2_wide_kernel
constexpr int kConvBK16 = 64, kConvBK32 = 32;          // k-tile of the 16-bit modes / of the fp32 mode
constexpr int kConvLdsBf16 = 65536, kConvLdsF32 = 69632, kConvLdsF32M32 = 43520;
constexpr int kConvLdsF16x2 = 131072, kConvLdsF16x2Wide = 147456, kConvLdsF16x2First = 135168;

// Geometry of one layer on the one-pixel-border NHWC layout: padded input Hp x Wp, output Ho x Wo, GEMM depth K,
// first tap off = 1 - pad, GEMM rows M.  Needs stride >= 1 (conv_validate checks it before it calls this).
struct ConvGeom {
  int B, Cin, Cout, ksize, stride;
  int Hp, Wp, Ho, Wo, K, off;
  int64_t M;
};
inline ConvGeom conv_geom(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad) {
  ConvGeom g;
  g.B = B; g.Cin = Cin; g.Cout = Cout; g.ksize = ksize; g.stride = stride;
  g.Hp = H + 2; g.Wp = W + 2;
  g.Ho = (H + 2 * pad - ksize) / stride + 1; g.Wo = (W + 2 * pad - ksize) / stride + 1;
  g.K = ksize * ksize * Cin;
  g.off = 1 - pad;
  g.M = (int64_t)B * g.Ho * g.Wo;
  return g;
}

// what a call brings besides its shape
struct ConvFlags { bool has_add, out_f32, out_padded, dynamic; };
// the option the plan reads, taken once per call
struct ConvOptions { int conv_waves; };

// The plan is the ABI's memhip_conv_plan_t: the geometry and the ordered launches (kernel MEMHIP_CONV_K_*, grid, workgroup
// size, dynamic LDS bytes, and the live-sample range [dyn_lo, dyn_hi) in which a dynamic-batch launch works).
typedef memhip_conv_launch_t ConvLaunch;
typedef memhip_conv_plan_t ConvPlan;

// Accepts or rejects a call like the parent launchers did, per mode and word for word; *g is filled on MEMHIP_OK (g->M == 0
// for an empty batch: nothing to launch).  ptrs_ok: in, weight and out are non-null (the plan query has no pointers: true).
int conv_validate(int mode, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad, const ConvFlags& f,
                  bool ptrs_ok, ConvGeom* g);

// device_cus: max_cus().  mode MEMHIP_CONV_*; a geometry conv_validate accepted.
ConvPlan conv_plan(int mode, const ConvGeom& g, const ConvFlags& f, const ConvOptions& o, int device_cus);

}  // namespace memhip
