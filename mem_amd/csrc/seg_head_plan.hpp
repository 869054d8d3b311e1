// The host side of the FCN decode head's fused tail (memhip_bnhead_fwd / _bwd_sums / _bwd_apply, one memhip_bnhead_args_t
// for the three): the validation of a call and its grids, LDS and workspace.  Host arithmetic only: memhip_bnhead_plan runs
// without a device (tests/test_seg_head_cpu.py).  The constants are read by the kernels (seg_head.hip) and by the plan alike.
#pragma once
#include <cstdint>
#include "../../include/memhip.h"

namespace memhip {
namespace seghead {

constexpr int kThreads = 256;
constexpr int kChunk = 64;                     // channels per chunk: 8 lanes x 16 bytes of bf16
constexpr int kFwdPixels = 32;                 // pixels per tile of the forward and of _bwd_apply: one per 8 lanes
constexpr int kBwdPixels = 64;                 // pixels per tile of _bwd_sums
constexpr int kFwdMaxGrid = 512;               // the forward strides over the tiles beyond this many workgroups
constexpr int kGroups = MEMHIP_BN_GROUPS;      // the most partials per output of a two-stage sum
constexpr int kMaxK = 32;
constexpr int kMaxC = 512;
constexpr int kLdsLimit = 64 * 1024;

// the classifier rows held per thread: K rounded up to 8, 16, 24 or 32 (the rows behind K are zero)
inline int padded_classes(int K) { return (K + 7) & ~7; }
// forward: the whole classifier weight [KP, C]
inline int fwd_lds_bytes(int KP, int C) { return KP * C * 4; }
// _bwd_sums: the weight's chunk [KP, 64], the gradient tile [64, KP + 1], the z tile [64, 65] (also the fold's scratch)
inline int sums_lds_bytes(int KP) { return (KP * kChunk + kBwdPixels * (KP + 1) + kBwdPixels * (kChunk + 1)) * 4; }
// _bwd_apply: the weight's chunk and the gradient tile [32, KP + 1]
inline int apply_lds_bytes(int KP) { return (KP * kChunk + kFwdPixels * (KP + 1)) * 4; }

}  // namespace seghead

enum { BNHEAD_QUERY, BNHEAD_FWD, BNHEAD_SUMS, BNHEAD_APPLY };     // who asks: the pointers that must be there
int bnhead_plan(const memhip_bnhead_args_t* a, int who, memhip_bnhead_plan_t* p);

}  // namespace memhip
