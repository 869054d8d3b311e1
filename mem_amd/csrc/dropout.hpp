// Element-wise dropout of the finetuning model (nn.Dropout: pos_drop, Attention.proj_drop, Mlp.drop,
// mem/modeling_finetune.py:64,70,125-126,155,271,343) from a counter-based generator: the keep mask of an
// element is a pure function of (key, site, row, col), so the backward regenerates it and nothing is stored.
// The contract (include/memhip.h, memhip_dropout_t) lives in one place: every kernel that applies a mask and the
// memhip_dropout_mask export call dropout_keep8.
#pragma once
#include "common.h"

namespace memhip {

// memhip_dropout_t, by value (kernel arguments: the key is a per-step host value)
struct DropParams {
  unsigned key0, key1, site, thr;
  float scale;
  int row0;
};

inline DropParams drop_params(const memhip_dropout_t& d) {
  return DropParams{d.key0, d.key1, d.site, d.thr, d.scale, d.row0};
}

// Philox4x32-10 (Salmon et al., SC'11; the round function of at::Philox4_32 and Random123's philox4x32_10)
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
    const unsigned lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
    c = uint4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// Keep bits of the 8 columns 8*g .. 8*g+7 of residual-stream row `row` (bit j = column 8*g + j): one Philox call with
// counter (row, g, site, 0); column j takes 16-bit half (j & 1) of word (j >> 1), low half first, and is kept iff that
// half >= thr.
__device__ __forceinline__ unsigned dropout_keep8(const DropParams& d, unsigned row, unsigned g) {
  const uint4 w = philox4x32_10(uint4{row, g, d.site, 0u}, d.key0, d.key1);
  const unsigned ws[4] = {w.x, w.y, w.z, w.w};
  unsigned bits = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned h = (ws[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    bits |= (h >= d.thr ? 1u : 0u) << j;
  }
  return bits;
}

// the multiplier of column j of a keep word: scale (kept) or 0 (dropped)
__device__ __forceinline__ float dropout_mul(const DropParams& d, unsigned bits, int j) {
  return ((bits >> j) & 1u) ? d.scale : 0.f;
}

}  // namespace memhip
