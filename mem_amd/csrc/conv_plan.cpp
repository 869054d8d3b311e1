// The dispatch policy of the tokenizer convolutions (memhip_conv2d_nhwc, one memhip_conv_args_t for the three modes): what a
// call must look like (conv_validate) and which kernels it gets (conv_plan).  Every shape test, option test and grid formula
// of the three launchers is here, once; the launchers obey.
#include "conv_plan.hpp"
#include "common.h"

namespace memhip {
namespace {

void push(ConvPlan& a, int kernel, int grid, int block, int lds, int dyn_lo = 0, int dyn_hi = 1 << 30) {
  a.l[a.count++] = ConvLaunch{kernel, grid, block, lds, dyn_lo, dyn_hi};
}

// ---- validation.  The modes differ, and the differences are kept:
//   bf16, f16x2: only the encoder's three shapes (4x4/s2/p1, 3x3/s1/p1, 1x1/s1/p0) -- their outputs are never empty;
//                C_in = 4 (first layer, 4x4) or a multiple of 64 (a 64-deep k-tile lies inside one tap); C_out % 8
//                (16-byte stores of 16-bit values); f16x2 alone: the fp32 output is the dense logit matrix.
//   f32:         any kernel size 1..4, stride >= 1, pad 0 / 1; C_in % 4 and C_out % 4 (16-byte chunks of floats); the only
//                mode that can be asked for an empty output, and checks for it; K % 32.
int validate16(const char* name, bool f16x2, const memhip_conv_args_t& a, const ConvFlags& f, bool ptrs_ok, ConvGeom* g) {
  MEMHIP_REQUIRE(a.B >= 0 && a.H > 0 && a.W > 0 && a.Cin > 0 && a.Cout > 0, "%s: bad shape", name);
  if (a.B == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(ptrs_ok, "%s: null pointer", name);
  MEMHIP_REQUIRE((a.ksize == 4 && a.stride == 2 && a.pad == 1) || (a.ksize == 3 && a.stride == 1 && a.pad == 1) ||
                     (a.ksize == 1 && a.stride == 1 && a.pad == 0),
                 "%s: only the encoder's shapes (4x4/s2/p1, 3x3/s1/p1, 1x1) are provided", name);
  MEMHIP_REQUIRE(a.Cin == 4 ? (a.ksize == 4) : (a.Cin % 64 == 0), "%s: C_in must be 4 (first layer, 4x4) or a multiple of 64", name);
  MEMHIP_REQUIRE(a.Cout % 8 == 0, "%s: C_out must be a multiple of 8", name);
  if (f16x2) MEMHIP_REQUIRE(!(f.out_f32 && f.out_padded), "%s: the fp32 output is the dense token-logit matrix", name);
  *g = conv_geom(a);
  MEMHIP_REQUIRE(g->K % kConvBK16 == 0, "%s: K = %d must be a multiple of 64", name, g->K);
  MEMHIP_REQUIRE(g->M < (1LL << 31), "%s: too many output pixels", name);
  return MEMHIP_OK;
}

int validate_f32(const memhip_conv_args_t& a, bool ptrs_ok, ConvGeom* g) {
  MEMHIP_REQUIRE(a.B >= 0 && a.H > 0 && a.W > 0 && a.Cin > 0 && a.Cout > 0, "conv2d_f32: bad shape");
  if (a.B == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(ptrs_ok, "conv2d_f32: null pointer");
  MEMHIP_REQUIRE(a.ksize >= 1 && a.ksize <= 4 && a.stride >= 1 && a.pad >= 0 && a.pad <= 1,
                 "conv2d_f32: kernel size 1..4, padding 0 or 1 (one-pixel border layout)");
  MEMHIP_REQUIRE(a.Cin % 4 == 0 && a.Cout % 4 == 0, "conv2d_f32: C_in and C_out must be multiples of 4");
  *g = conv_geom(a);
  MEMHIP_REQUIRE(g->Ho > 0 && g->Wo > 0, "conv2d_f32: empty output");
  MEMHIP_REQUIRE(g->K % kConvBK32 == 0, "conv2d_f32: K = %d must be a multiple of %d", g->K, kConvBK32);
  MEMHIP_REQUIRE(g->M < (1LL << 31), "conv2d_f32: too many output pixels");
  return MEMHIP_OK;
}

}  // namespace

int conv_validate(const memhip_conv_args_t* a, bool query, ConvFlags* f, ConvGeom* g) {
  *f = ConvFlags{};
  *g = ConvGeom{};
  MEMHIP_REQUIRE(a, "conv2d: null args");
  const int mode = a->mode;
  MEMHIP_REQUIRE(mode == MEMHIP_CONV_BF16 || mode == MEMHIP_CONV_F32 || mode == MEMHIP_CONV_F16X2, "conv2d: unknown mode %d", mode);
  MEMHIP_REQUIRE(!a->n_active || mode == MEMHIP_CONV_F32, "conv2d: only the fp32 mode has a dynamic batch (n_active)");
  MEMHIP_REQUIRE(!a->out_f32 || mode == MEMHIP_CONV_F16X2, "conv2d: out_f32 is a flag of the fp16x2 mode");
  MEMHIP_REQUIRE(mode == MEMHIP_CONV_F16X2 || !(a->in_plane || a->w_plane || a->add_plane || a->out_plane),
                 "conv2d: plane strides are fields of the fp16x2 mode");
  *f = ConvFlags{a->add != nullptr, a->out_f32 != 0, a->out_padded != 0, a->n_active != nullptr};
  const bool ptrs_ok = query || (a->in && a->weight && a->out);
  if (mode == MEMHIP_CONV_F32) return validate_f32(*a, ptrs_ok, g);
  const bool f16x2 = mode == MEMHIP_CONV_F16X2;
  return validate16(f16x2 ? "conv2d_f16x2" : "conv2d", f16x2, *a, *f, ptrs_ok, g);
}

ConvPlan conv_plan(int mode, const ConvGeom& g, const ConvFlags& f, const ConvOptions& o, int device_cus) {
  ConvPlan a = {};
  a.Hp = g.Hp; a.Wp = g.Wp; a.Ho = g.Ho; a.Wo = g.Wo; a.K = g.K; a.off = g.off; a.M = g.M;
  if (g.M == 0) return a;
  const int ntn = cdiv(g.Cout, kConvTileN);
  const int grid = cdiv(g.M, kConvTileM) * ntn;        // one 128 x 128 tile per workgroup
  if (mode == MEMHIP_CONV_BF16) {
    push(a, MEMHIP_CONV_K_BF16, grid, 256, kConvLdsBf16);
    return a;
  }
  if (mode == MEMHIP_CONV_F32) {
    if (!f.dynamic) {
      push(a, MEMHIP_CONV_K_F32, grid, 256, kConvLdsF32);
      return a;
    }
    // dynamic batch: BOTH tile forms are launched with fixed grids of persistent workgroups; the device-side count selects
    // one (fewer than `sw` live samples: 32-row tiles, a layer is otherwise one under-filled round of 128-row tiles; from
    // `sw` on: the 128-row tiles at their better rate per FLOP).  The other launch returns at its first instruction.
    // Per layer: the 128-row form pays once its live tiles fill the chip's 2 x 256 workgroup slots -- 7 samples at the
    // 56 x 56 level, 112 (= ceil(65536 / 588)) at the 14 x 14 level, both with 384 output channels.
    const long long per_sample = (long long)g.Ho * g.Wo * ntn;
    int sw = (int)((512LL * kConvTileM + per_sample - 1) / per_sample);
    sw = sw < 1 ? 1 : sw;
    const int grid_s = cdiv(g.M, kConvF32SmallM) * ntn;
    push(a, MEMHIP_CONV_K_F32_M32, grid_s > 2048 ? 2048 : grid_s, 256, kConvLdsF32M32, 0, sw);
    push(a, MEMHIP_CONV_K_F32, grid > 1024 ? 1024 : grid, 256, kConvLdsF32, sw, 1 << 30);
    return a;
  }
  // ---- fp16x2.  conv_waves: 4 = four waves per workgroup; 8 = eight waves, 128 x 128 tiles only; 16 (default) = eight waves,
  // the persistent first-layer kernel and the 256 x 128 tile where they apply; 32 = the wide tile at any size (tests).
  const bool cin4 = g.Cin == 4;
  if (cin4 && o.conv_waves >= 16 && g.K == kConvBK16 && !f.has_add && !f.out_f32 && g.M % kConvTileM == 0 &&
      g.Cout % kConvTileN == 0) {
    // the first layer, persistent: one workgroup per CU, `cols` of them per column tile of the weights (whole tiles only:
    // every lane then issues every store, which the kernel's counted waits rely on)
    const int full = g.Cout / kConvTileN, nmt = (int)(g.M / kConvTileM);
    int cols = device_cus / full;
    cols = cols < 1 ? 1 : cols;
    cols = cols > nmt ? nmt : cols;
    push(a, MEMHIP_CONV_K_F16X2_FIRST, cols * full, 512, kConvLdsF16x2First);
    return a;
  }
  // the 256 x 128 tile where its grid is at least two full rounds of the chip: every layer of the encoder at batch 256 but
  // the first (the 14 x 14 layers are 588 workgroups = 2.3 rounds and still gain: forward 18.55 -> 18.30 ms against the
  // finer 128 x 128 tiles)
  const int wgrid = cdiv(g.M, kConvWideM) * ntn;
  if (!cin4 && (o.conv_waves == 32 || (o.conv_waves == 16 && wgrid >= 2 * device_cus)))
    push(a, MEMHIP_CONV_K_F16X2_WIDE, wgrid, 512, kConvLdsF16x2Wide);
  else if (o.conv_waves == 4)
    push(a, MEMHIP_CONV_K_F16X2_W4, grid, 256, kConvLdsF16x2);
  else
    push(a, MEMHIP_CONV_K_F16X2_W8, grid, 512, kConvLdsF16x2);
  return a;
}

// ---- the transposed convolution of the decoder (bf16 only): Cin % 64 (a 64-deep k-tile lies inside one of the 2x2 taps),
// Cout % 8 (16-byte stores); 4 M output pixels
int convt_validate(int B, int H, int W, int Cin, int Cout, bool ptrs_ok) {
  MEMHIP_REQUIRE(B >= 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "convt2d: bad shape");
  if (B == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(ptrs_ok, "convt2d: null pointer");
  MEMHIP_REQUIRE(Cin % 64 == 0, "convt2d: C_in must be a multiple of 64");
  MEMHIP_REQUIRE(Cout % 8 == 0, "convt2d: C_out must be a multiple of 8");
  MEMHIP_REQUIRE(4 * (int64_t)B * H * W < (1LL << 31), "convt2d: too many output pixels");
  return MEMHIP_OK;
}

ConvPlan convt_plan(int B, int H, int W, int Cin, int Cout) {
  ConvPlan a = {};
  a.Hp = H + 2; a.Wp = W + 2; a.Ho = 2 * H; a.Wo = 2 * W; a.K = 4 * Cin; a.off = 0; a.M = (int64_t)B * H * W;
  if (a.M == 0) return a;
  // one launch for the four phases: (row tile, phase, column tile), one 128 x 128 tile per workgroup
  const long long grid = 4LL * cdiv(a.M, kConvTileM) * cdiv(Cout, kConvTileN);
  push(a, MEMHIP_CONV_K_BF16_T, (int)grid, 256, kConvLdsBf16);
  return a;
}

}  // namespace memhip

extern "C" int memhip_convt_plan(int B, int H, int W, int Cin, int Cout, int device_cus, memhip_conv_plan_t* out) {
  using namespace memhip;
  MEMHIP_REQUIRE(out, "convt_plan: null pointer");
  if (int rc = convt_validate(B, H, W, Cin, Cout, true)) return rc;
  (void)device_cus;                                     // the one form does not depend on the device
  *out = convt_plan(B, H, W, Cin, Cout);
  return MEMHIP_OK;
}

extern "C" int memhip_conv_plan(const memhip_conv_args_t* args, int device_cus, memhip_conv_plan_t* out) {
  using namespace memhip;
  MEMHIP_REQUIRE(out, "conv_plan: null pointer");
  ConvFlags f;
  ConvGeom g;
  if (int rc = conv_validate(args, true, &f, &g)) return rc;
  *out = conv_plan(args->mode, g, f, ConvOptions{opt(OPT_CONV_WAVES)}, device_cus >= 0 ? device_cus : max_cus());
  return MEMHIP_OK;
}
