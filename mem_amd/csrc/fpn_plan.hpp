// The host side of the UPerNet head's FPN part (memhip_fpn_topdown_fwd / _concat_fwd / _resize_bwd / _bn_bwd_sums /
// _bn_bwd_apply, one memhip_fpn_args_t for the five): the validation of a call and its grids.  Host arithmetic only:
// memhip_fpn_plan runs without a device (tests/test_uper_head_cpu.py).  The constants are read by the kernels (fpn.hip) and by
// the plan alike.
#pragma once
#include "common.h"

namespace memhip {
namespace fpn {

constexpr int kThreads = 256;
constexpr int kChunk = 64;                     // channels per tile: 8 lanes x 16 bytes of bf16
constexpr int kPixels = 64;                    // pixels per tile of _topdown_fwd, _concat_fwd and _bn_bwd_apply: two per 8 lanes
constexpr int kRows = 32;                      // destination pixels per tile of _resize_bwd, row lanes of _bn_bwd_sums
constexpr int kMaxC = 512;
constexpr int kGroups = MEMHIP_BN_GROUPS;
constexpr int kSumsLdsBytes = 2 * kRows * kChunk * 4;

}  // namespace fpn

enum { FPN_QUERY, FPN_TOPDOWN, FPN_CONCAT, FPN_RESIZE, FPN_SUMS, FPN_APPLY };     // who asks: the pointers that must be there
int fpn_plan(const memhip_fpn_args_t* a, int who, memhip_fpn_plan_t* p);

}  // namespace memhip
