// The tokenizer's entry points: each validates, decides once and hands over to the launcher of the mode's file (conv.hip:
// bf16, conv_f32.hip: fp32, conv_f16x2.hip: two fp16 planes).  conv_plan.cpp holds the convolution's rules.
#include "common.h"
#include "conv_plan.hpp"

using namespace memhip;

static_assert(MEMHIP_CONV_BF16 == 0 && MEMHIP_CONV_F32 == 1 && MEMHIP_CONV_F16X2 == 2, "the launcher tables are in this order");

// validate -> plan -> launch.  Only the fp16x2 plan depends on the option and the device.
extern "C" int memhip_conv2d_nhwc(const memhip_conv_args_t* args, memhip_stream_t stream) {
  ConvFlags f;
  ConvGeom g;
  if (int rc = conv_validate(args, false, &f, &g)) return rc;
  if (g.M == 0) return MEMHIP_OK;
  const bool f16x2 = args->mode == MEMHIP_CONV_F16X2;
  const ConvPlan plan = conv_plan(args->mode, g, f, ConvOptions{f16x2 ? opt(OPT_CONV_WAVES) : 0}, f16x2 ? max_cus() : 0);
  static ConvLaunchFn* const launch[] = {conv_bf16_launch, conv_f32_launch, conv_f16x2_launch};
  return launch[args->mode](*args, g, plan, stream);
}

extern "C" int memhip_nchw_to_padded_nhwc4(const float* x, int B, int C, int H, int W, const float* mean, const float* stdv,
                                           void* out, int64_t out_plane, int mode, memhip_stream_t stream) {
  MEMHIP_REQUIRE(mode == MEMHIP_CONV_BF16 || mode == MEMHIP_CONV_F32 || mode == MEMHIP_CONV_F16X2,
                 "nchw_to_padded_nhwc4: unknown mode %d", mode);
  MEMHIP_REQUIRE(mode == MEMHIP_CONV_F16X2 || !out_plane, "nchw_to_padded_nhwc4: out_plane is an argument of the fp16x2 mode");
  MEMHIP_REQUIRE(B >= 0 && C >= 1 && C <= 4 && H > 0 && W > 0, "nchw_to_padded_nhwc4: bad shape");
  if (B == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(x && out && (!mean == !stdv), "nchw_to_padded_nhwc4: null pointer");
  static ToNhwc4LaunchFn* const launch[] = {to_nhwc4_bf16_launch, to_nhwc4_f32_launch, to_nhwc4_f16x2_launch};
  return launch[mode](x, B, C, H, W, mean, stdv, out, out_plane, stream);
}

extern "C" int memhip_argmax_rows(const void* logits, int mode, int64_t ld, int M, int N, int64_t* ids, float* top2_gap,
                                  float* row_rms, const int32_t* n_samples, int rows_per_sample, memhip_stream_t stream) {
  MEMHIP_REQUIRE(mode == MEMHIP_CONV_BF16 || mode == MEMHIP_CONV_F32, "argmax_rows: the logits are bf16 or fp32, mode %d", mode);
  if (mode == MEMHIP_CONV_BF16) {
    MEMHIP_REQUIRE(M >= 0 && N > 0 && N % 8 == 0 && ld % 8 == 0, "argmax_rows: N and ld must be multiples of 8");
    MEMHIP_REQUIRE(!top2_gap && !row_rms && !n_samples, "argmax_rows: top2_gap, row_rms and n_samples go with fp32 logits");
  } else {
    MEMHIP_REQUIRE(M >= 0 && N > 0 && N % 4 == 0 && ld % 4 == 0, "argmax_rows_f32: N and ld must be multiples of 4");
    MEMHIP_REQUIRE(!n_samples || rows_per_sample > 0, "argmax_rows_f32: rows_per_sample");
  }
  if (M == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(logits && ids, "argmax_rows: null pointer");
  static ArgmaxLaunchFn* const launch[] = {argmax_rows_bf16_launch, argmax_rows_f32_launch};
  return launch[mode](logits, ld, M, N, ids, top2_gap, row_rms, n_samples, rows_per_sample, stream);
}

// The decoder: validate -> plan -> launch, like the convolutions above (the rules are convt_validate / convt_plan in conv_plan.cpp).
extern "C" int memhip_convt2d_nhwc(const void* in, const void* weight, const float* bias, void* out, int B, int H, int W, int Cin,
                                   int Cout, int relu, memhip_stream_t stream) {
  if (int rc = convt_validate(B, H, W, Cin, Cout, in && weight && out)) return rc;
  if (B == 0) return MEMHIP_OK;
  return convt_bf16_launch(in, weight, bias, out, B, H, W, Cin, Cout, relu, convt_plan(B, H, W, Cin, Cout), stream);
}

extern "C" int memhip_kl_uniform_rows(const void* logits, int mode, int64_t ld, int M, int N, float* row_kl, memhip_stream_t stream) {
  MEMHIP_REQUIRE(mode == MEMHIP_CONV_BF16 || mode == MEMHIP_CONV_F32, "kl_uniform_rows: the logits are bf16 or fp32, mode %d", mode);
  const int vec = mode == MEMHIP_CONV_BF16 ? 8 : 4;
  MEMHIP_REQUIRE(M >= 0 && N > 0 && N % vec == 0 && ld >= N && ld % vec == 0, "kl_uniform_rows: N and ld must be multiples of %d", vec);
  if (M == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(logits && row_kl, "kl_uniform_rows: null pointer");
  return kl_uniform_rows_launch(logits, mode, ld, M, N, row_kl, stream);
}
