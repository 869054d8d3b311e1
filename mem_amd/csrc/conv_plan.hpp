// Which kernels take a memhip_conv2d_nhwc call, with which grids, workgroup sizes and LDS bytes: conv_geom is the one place
// that derives a layer's geometry, conv_validate the one place that reads a memhip_conv_args_t and accepts or rejects it,
// conv_plan (conv_plan.cpp) the one place that decides the dispatch -- once per call, from the geometry, the flags of the
// call, the device's CU count and a snapshot of the options.  Host arithmetic only: memhip_conv_plan takes the struct of the
// call and returns the same plan without a device (tests/test_conv_plan_cpu.py checks it against the cascades it replaced).
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
inline ConvGeom conv_geom(const memhip_conv_args_t& a) {
  ConvGeom g;
  g.B = a.B; g.Cin = a.Cin; g.Cout = a.Cout; g.ksize = a.ksize; g.stride = a.stride;
  g.Hp = a.H + 2; g.Wp = a.W + 2;
  g.Ho = (a.H + 2 * a.pad - a.ksize) / a.stride + 1; g.Wo = (a.W + 2 * a.pad - a.ksize) / a.stride + 1;
  g.K = a.ksize * a.ksize * a.Cin;
  g.off = 1 - a.pad;
  g.M = (int64_t)a.B * g.Ho * g.Wo;
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

// The one reader of the struct, for the call and for the plan query: accepts or rejects it like the parent launchers did, per
// mode and word for word, and rejects a field the mode does not have; *f and *g are filled on MEMHIP_OK (g->M == 0 for an
// empty batch: nothing to launch).  query: in, weight and out may be null (the query dereferences nothing).
int conv_validate(const memhip_conv_args_t* a, bool query, ConvFlags* f, ConvGeom* g);

// device_cus: max_cus().  mode MEMHIP_CONV_*; a geometry conv_validate accepted.
ConvPlan conv_plan(int mode, const ConvGeom& g, const ConvFlags& f, const ConvOptions& o, int device_cus);

// The launchers, one of each per mode in MEMHIP_CONV_* order (conv.hip, conv_f32.hip, conv_f16x2.hip); their arguments are
// validated by the entry points (conv_entry.cpp), so a mode ignores what it does not have.  conv: fill the kernel arguments
// from the struct and its geometry and launch what the plan names (plan.count >= 1); to_nhwc4: the input conversion; argmax_rows.
typedef int ConvLaunchFn(const memhip_conv_args_t& a, const ConvGeom& g, const ConvPlan& plan, memhip_stream_t stream);
typedef int ToNhwc4LaunchFn(const float* x, int B, int C, int H, int W, const float* mean, const float* stdv, void* out,
                            int64_t out_plane, memhip_stream_t stream);
typedef int ArgmaxLaunchFn(const void* logits, int64_t ld, int M, int N, int64_t* ids, float* top2_gap, float* row_rms,
                           const int32_t* n_samples, int rows_per_sample, memhip_stream_t stream);
ConvLaunchFn conv_bf16_launch, conv_f32_launch, conv_f16x2_launch;
ToNhwc4LaunchFn to_nhwc4_bf16_launch, to_nhwc4_f32_launch, to_nhwc4_f16x2_launch;
ArgmaxLaunchFn argmax_rows_bf16_launch, argmax_rows_f32_launch;

// ---- the decoder's transposed convolution, ConvTranspose2d(4, stride 2, pad 1) as four 2x2 phase GEMMs (convt.hip; plain
// arguments: memhip_convt2d_nhwc and memhip_convt_plan).  convt_validate is the one reader of the arguments for the call and
// the query (ptrs_ok: the query dereferences nothing), convt_plan the one place that decides the launch; the launcher obeys.
int convt_validate(int B, int H, int W, int Cin, int Cout, bool ptrs_ok);
ConvPlan convt_plan(int B, int H, int W, int Cin, int Cout);
int convt_bf16_launch(const void* in, const void* weight, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                      int relu, const ConvPlan& plan, memhip_stream_t stream);
int kl_uniform_rows_launch(const void* logits, int mode, int64_t ld, int M, int N, float* row_kl, memhip_stream_t stream);

}  // namespace memhip
