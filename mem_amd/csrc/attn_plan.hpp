// Which kernels take a memhip_attn_fwd / memhip_attn_bwd call, with which template arguments, grids and LDS sizes:
// attn_plan_fwd / attn_plan_bwd (attn_plan.cpp) are the one place that decides, once per call, from the shape, the flags of
// the call, the stream's CU count and a snapshot of the options.  Host arithmetic only: memhip_attn_plan_fwd / _bwd return
// the same plan without a device (tests/test_attn_plan_cpu.py checks the DESIGN.md table through them).
#pragma once
#include <cstdint>
#include "../../include/memhip.h"

namespace memhip {

constexpr int kMaxLds = 160 * 1024;   // bytes of LDS one workgroup may use on gfx950

// ---- geometry the plan shares with the kernels (pure arithmetic: usable on both sides)
// extended relative-position table of attn.hip / attn_stream.hip (layout: attn_common.hpp)
struct RelGeom { int off, len; };
constexpr RelGeom rel_geom(int Wh, int Ww) {
  const int off = (Wh - 1) * (2 * Ww - 1) + (Ww - 1);
  return RelGeom{off, (5 * off + 4 + 3) & ~3};   // padded to 16 bytes: the arrays laid out behind it are read as b128
}

// slot layout of attn_win.hip for windows WW tokens wide
template <int WW> struct WinGeo {
  static constexpr int WS = (WW + 7) & ~7;        // slots per grid row
  static constexpr int CT = 128;                   // slots per chunk
  static constexpr int RPC = CT / WS;              // grid rows per chunk
  static constexpr int PAD0 = RPC * WS;            // first padding slot of a chunk (the cls token in chunk 0)
  static constexpr int P = 2 * WW - 1;
  static_assert(PAD0 < CT && PAD0 % 8 == 0, "the window width needs at least one padding slot per chunk");
  static constexpr int CLS_KB = PAD0 / 32, CLS_G = (PAD0 % 32) / 8;
  static constexpr int CQ = ((RPC - 1) * P + WS + 8 + 3) & ~3;     // floats of the constant strip of the cls row
  // (slot s of a chunk, s a multiple of 4) -> constant part of the bucket index; s + 4 stays in the same grid row
  static constexpr int imm(int s) { return (s / WS) * P + (s % WS); }
  static constexpr bool valid(int s) { return s < PAD0 && (s % WS) < WW; }
  static constexpr int row(int s) { return s / WS; }
};

// attn16.hip: workgroup sizes and LDS bytes of its two kernels (the file asserts them against its own carve-up)
constexpr int kAttn16ThreadsFwd = 512, kAttn16ThreadsBwd = 448, kAttn16LdsFwd = 152176, kAttn16LdsBwd = 160016;

// (row, head) pairs per workgroup of attn_delta_kernel: 32
inline int attn_delta_grid(int64_t rows, int heads) { return (int)((rows * heads + 31) / 32); }

// The plan is the ABI's memhip_attn_plan_t: family MEMHIP_ATTN_*, template choices, samples-per-workgroup numbers and the
// ordered launches (kernel MEMHIP_ATTN_K_*, grid, workgroup size, dynamic LDS bytes).
typedef memhip_attn_launch_t AttnLaunch;
typedef memhip_attn_plan_t AttnPlan;

struct AttnShape { int B, T, heads, window_h, window_w; };
// what a backward call brings: which optional gradients / inputs are given, and the caller's workspace
struct AttnBwdFlags {
  bool has_dtable, has_dv_bias, has_out;
  bool ws_ok;            // ws is non-null and 16-byte aligned
  int64_t ws_bytes;
};
// the options the plan reads, taken once per call (attn16_stagger / attn16_stagger_fwd are launch arguments, read by the
// launchers)
struct AttnOptions { int attn16, attn_win; };

// stream_cus: usable_cus(stream).  count == 0 with lds_over > 0: no family fits (`family` names the last one tried).
AttnPlan attn_plan_fwd(const AttnShape& p, int stream_cus, const AttnOptions& o);
AttnPlan attn_plan_bwd(const AttnShape& p, const AttnBwdFlags& f, int stream_cus, const AttnOptions& o);
// bytes of the dS workspace the dS-storing backward wants (0: no such form for this window)
int64_t attn_bwd_win_workspace(int B, int T, int heads, int window_h, int window_w);

// the pointers and strides of one call, forward or backward (fields the direction does not use: null / 0)
struct AttnArgs {
  const void* qkv; int64_t ldqkv;
  const float* table;
  void* out; int64_t ldout;        // forward: written; backward from the forward output: read (null: `delta` is filled)
  float* lse;
  const void* dout; int64_t ldo;
  float* delta;
  float* stats;                    // the last 4 * heads floats of the delta workspace
  float scale;
  void* dqkv; int64_t lddqkv;
  float* dtable; float* dq_bias; float* dv_bias;
  void* ws;
  int B, T, D, heads, window_h, window_w;
};

}  // namespace memhip
