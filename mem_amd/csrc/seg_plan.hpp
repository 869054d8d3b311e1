// The host side of the segmentation loss (memhip_seg_ce / memhip_seg_confusion, one memhip_seg_args_t for both): the bilinear
// axis tables, the validation of a call and its tiles, grid, LDS and workspace.  Host arithmetic only: memhip_seg_axis_table
// and memhip_seg_plan run without a device (tests/test_seg_loss_cpu.py).  The constants are read by the kernels
// (seg_loss.hip) and by the plan alike.
#pragma once
#include <cstdint>
#include "../../include/memhip.h"

namespace memhip {
namespace seg {

constexpr int kThreads = 256;
constexpr int kTile = 8;                       // low-resolution pixels per workgroup and axis
constexpr int kHalo = kTile + 2;               // the tile and one pixel around it: what its footprint reads
constexpr int kChunk = kThreads;               // outputs of the footprint per pass, one per thread
constexpr int kMaxC = 32;
constexpr int kLdsLimit = 64 * 1024;
constexpr int kConfThreads = 256;
constexpr int kConfMaxGrid = 2048;             // the confusion kernel strides over the pixels beyond this many workgroups
constexpr int kMaxSide = 32768;                // H, W

// a workgroup's contribution, folded by the finish kernel in workgroup order (kept: memhip_seg_ce_w's n_kept, else 0)
struct Partial { double loss; int32_t valid, correct, bad, kept; };

// the kernel is instantiated for 8, 12, .. 32 channels (a thread gathers channels t / 64 + 4k; the workgroup's fold needs the
// 5 KiB that eight channels of q give)
inline int padded_channels(int C) { return C <= 8 ? 8 : (C + 3) & ~3; }
// LDS of the training kernel without the tables: the logits of the halo tile (pitch CP + 1) and one chunk of q, all channels
inline int lds_fixed_bytes(int CP) { return (kHalo * kHalo * (CP + 1) + CP * kChunk) * 4; }


// memhip_seg_ohem_select: a radix select on the 31 value bits of the keys that count; word bits 31..21 / 20..10 / 9..0 per pass
constexpr int kSelThreads = 256;
constexpr int kSelBins = 2048;
constexpr int kSelPasses = 3;
constexpr int kSelMaxGrid = 1024;              // the passes stride over the keys beyond this many workgroups
constexpr long long kMaxMinKept = 1LL << 40;   // K = min_kept * B stays far inside an int64
// the selection's part of the workspace: the three global histograms, then what the scans hand on
struct SelState { unsigned long long n, r, kept; uint32_t prefix, none, arrived, pad; };
inline uint64_t select_ws_bytes() { return (uint64_t)kSelPasses * kSelBins * 8 + sizeof(SelState); }

}  // namespace seg

int seg_axis_table(int in, int out, int align_corners, int32_t* i0, float* w1, int32_t* lo, int32_t* hi);

enum { SEG_QUERY, SEG_CE, SEG_CONFUSION, SEG_INPUTS };     // who asks: the pointers that must be there
// extra_lds: bytes the training kernel keeps beside its own (the staged class weights); check_ws = false leaves the
// workspace's size to the caller (seg_ohem_plan, whose workspace holds more)
int seg_plan(const memhip_seg_args_t* a, int who, memhip_seg_plan_t* p, int extra_lds = 0, bool check_ws = true);

enum { OHEM_QUERY, OHEM_KEYS, OHEM_SELECT, OHEM_CE };
int seg_ohem_plan(const memhip_segohem_args_t* a, int who, memhip_segohem_plan_t* p);

}  // namespace memhip
