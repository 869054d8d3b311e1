// Shared by the tokenizer convolution files (conv.hip: bf16, conv_f32.hip: fp32, conv_f16x2.hip: two fp16 planes): the device
// helpers all of them spell the same way, and the host side of validate -> plan -> launch (conv_plan.hpp decides; the
// launchers fill their kernel arguments from its geometry and launch what it names).  Everything has internal linkage.
#pragma once
#include "common.h"
#include "conv_plan.hpp"

namespace {

using namespace memhip;

// ---- device
// LDS slot of 16-byte chunk `chunk` of row `row` of a [rows][64] 16-bit tile: 128-byte rows, chunk position XOR-swizzled
__device__ __forceinline__ int swz_slot(int row, int chunk) { return row * 8 + (chunk ^ ((row >> 1) & 7)); }
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}
// torch.argmax's order: a NaN is greater than every number, ties (and several NaNs) go to the smallest index; so a row of
// all -inf gives 0 and a row with a NaN gives the first NaN's index -- always a valid id (it is used as a label next).
__device__ __forceinline__ bool argmax_better(float a, int ai, float b, int bi) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an && (!bn || ai < bi);
  return a > b || (a == b && ai < bi);
}

// ---- host
// the geometry fields every ConvArgs* struct has
template <typename P>
void fill_geom(P& p, const ConvGeom& g) {
  p.B = g.B; p.Hp = g.Hp; p.Wp = g.Wp; p.Cin = g.Cin; p.Ho = g.Ho; p.Wo = g.Wo; p.Cout = g.Cout;
  p.kw = g.ksize; p.stride = g.stride; p.off = g.off; p.K = g.K;
}

// Launch Kernel as the plan's launch `l` says; its dynamic-LDS limit is raised once per kernel, on first use.
template <auto Kernel, typename P>
int conv_launch(const ConvLaunch& l, hipStream_t s, const P& p) {
  static bool attr_done = false;
  if (!attr_done) {
    MEMHIP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, l.lds));
    attr_done = true;
  }
  hipLaunchKernelGGL(Kernel, dim3(l.grid), dim3(l.block), l.lds, s, p);
  return MEMHIP_OK;
}

}  // namespace
