// The bilinear axis tables of the segmentation loss and the one place that reads a memhip_seg_args_t, accepts or rejects it
// and sizes the launches of memhip_seg_ce / memhip_seg_confusion; the launchers (seg_loss.hip) obey.  seg_ohem_plan does the
// same for the memhip_segohem_args_t of memhip_seg_ohem_keys / _select (seg_ohem.hip) and memhip_seg_ce_w (seg_loss.hip).
#include "seg_plan.hpp"
#include <cmath>
#include <vector>
#include "common.h"

namespace memhip {
using namespace seg;

// torch's upsample_bilinear2d (area_pixel_compute_scale / _source_index), fp32, one multiply and one add at a time (this
// file is built without contraction)
int seg_axis_table(int in, int out, int align_corners, int32_t* i0, float* w1, int32_t* lo, int32_t* hi) {
  MEMHIP_REQUIRE(in >= 1 && out >= in && out <= kMaxSide, "seg_axis_table: bad shape in=%d out=%d (1 <= in <= out <= %d)", in, out,
                 kMaxSide);
  MEMHIP_REQUIRE(align_corners == 0 || align_corners == 1, "seg_axis_table: align_corners=%d must be 0 or 1", align_corners);
  MEMHIP_REQUIRE(i0 && w1 && lo && hi, "seg_axis_table: null pointer");
  const float scale = align_corners ? (out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f) : (float)in / (float)out;
  for (int i = 0; i < in; ++i) { lo[i] = out; hi[i] = -1; }
  for (int y = 0; y < out; ++y) {
    float src;
    if (align_corners) {
      src = scale * (float)y;
    } else {
      src = scale * ((float)y + 0.5f) - 0.5f;
      if (src < 0.f) src = 0.f;
    }
    int a = (int)src;                          // src >= 0: truncation is floor
    if (a > in - 1) a = in - 1;
    const int b = a + 1 < in ? a + 1 : in - 1;
    i0[y] = a;
    w1[y] = src - (float)a;
    if (y < lo[a]) lo[a] = y;
    if (y < lo[b]) lo[b] = y;
    hi[a] = y;                                 // y ascends
    hi[b] = y;
  }
  return MEMHIP_OK;
}

namespace {

// the largest footprint lo[first] .. hi[last] over the tiles of one axis
int max_footprint(int in, int out, int align_corners) {
  std::vector<int32_t> i0(out), lo(in), hi(in);
  std::vector<float> w1(out);
  seg_axis_table(in, out, align_corners, i0.data(), w1.data(), lo.data(), hi.data());
  int m = 0;
  for (int first = 0; first < in; first += kTile) {
    const int last = first + kTile < in ? first + kTile - 1 : in - 1;
    const int f = hi[last] - lo[first] + 1;
    if (f > m) m = f;
  }
  return m;
}

}  // namespace

int seg_plan(const memhip_seg_args_t* a, int who, memhip_seg_plan_t* p, int extra_lds, bool check_ws) {
  *p = memhip_seg_plan_t{};
  MEMHIP_REQUIRE(a, "seg: null args");
  const int B = a->B, C = a->C, h = a->h, w = a->w, H = a->H, W = a->W;
  MEMHIP_REQUIRE(B >= 1, "seg: bad shape B=%d (B >= 1)", B);
  MEMHIP_REQUIRE(C >= 2 && C <= kMaxC, "seg: bad shape C=%d (2 <= C <= %d)", C, kMaxC);
  MEMHIP_REQUIRE(h >= 1 && w >= 1, "seg: bad shape h=%d w=%d (the logits' size, positive)", h, w);
  MEMHIP_REQUIRE(H >= h && W >= w, "seg: bad shape H=%d W=%d for logits of %dx%d (H >= h and W >= w: the resize never shrinks)", H, W,
                 h, w);
  MEMHIP_REQUIRE(H <= kMaxSide && W <= kMaxSide && (long long)B * H * W <= (1LL << 36),
                 "seg: bad shape B=%d H=%d W=%d, too many pixels (H, W <= %d, B H W <= 2^36)", B, H, W, kMaxSide);
  MEMHIP_REQUIRE(a->ignore_index >= -1 && a->ignore_index <= 255, "seg: ignore_index=%d must be a label 0..255, or -1 for none",
                 a->ignore_index);
  MEMHIP_REQUIRE(a->align_corners == 0 || a->align_corners == 1, "seg: align_corners=%d must be 0 or 1", a->align_corners);
  MEMHIP_REQUIRE(a->avg_non_ignore == 0 || a->avg_non_ignore == 1, "seg: avg_non_ignore=%d must be 0 or 1", a->avg_non_ignore);
  const int tiles_y = cdiv(h, kTile), tiles_x = cdiv(w, kTile);
  MEMHIP_REQUIRE((long long)B * tiles_y * tiles_x <= 0x7fffffffLL, "seg: bad shape B=%d h=%d w=%d, too many tiles", B, h, w);
  if (who != SEG_QUERY) {                        // (SEG_INPUTS: these and nothing else)
    MEMHIP_REQUIRE(a->logits && a->labels, "seg: null pointer (logits, labels)");
    MEMHIP_REQUIRE(a->y_i0 && a->y_w1 && a->y_lo && a->y_hi && a->x_i0 && a->x_w1 && a->x_lo && a->x_hi,
                   "seg: null pointer (axis tables)");
  }
  if (who == SEG_CE) {
    MEMHIP_REQUIRE(a->dz && a->loss && a->stats && a->workspace, "seg_ce: null pointer (dz, loss, stats, workspace)");
    MEMHIP_REQUIRE(((uintptr_t)a->workspace & 7) == 0, "seg_ce: workspace is not 8-byte aligned");
    MEMHIP_REQUIRE(std::isfinite(a->loss_weight), "seg_ce: loss_weight is not finite");
  }
  if (who == SEG_CONFUSION) MEMHIP_REQUIRE(a->confusion, "seg_confusion: null pointer (confusion)");

  p->tile_h = p->tile_w = kTile;
  p->tiles_y = tiles_y;
  p->tiles_x = tiles_x;
  p->grid = B * tiles_y * tiles_x;
  p->block = kThreads;
  p->chunk = kChunk;
  p->max_fh = max_footprint(h, H, a->align_corners);
  p->max_fw = max_footprint(w, W, a->align_corners);
  const int fixed = lds_fixed_bytes(padded_channels(C)) + extra_lds;
  const int tables = (p->max_fh + p->max_fw) * 8;           // i0 and w1 of both axes
  p->tables_in_lds = fixed + tables <= kLdsLimit;
  p->lds_bytes = fixed + (p->tables_in_lds ? tables : 0);
  p->slot_bytes = (int)sizeof(Partial);
  p->ws_bytes = (uint64_t)p->grid * sizeof(Partial);
  const long long blocks = ((long long)B * H * W + kConfThreads - 1) / kConfThreads;
  p->conf_grid = (int)(blocks < kConfMaxGrid ? blocks : kConfMaxGrid);
  p->conf_block = kConfThreads;
  p->conf_lds_bytes = kMaxC * kMaxC * 4;
  if (check_ws && (who == SEG_CE || (who == SEG_QUERY && a->workspace)) && a->workspace_bytes < p->ws_bytes)
    return fail(MEMHIP_EWORKSPACE, "seg_ce: workspace %zu < %zu", a->workspace_bytes, (size_t)p->ws_bytes);
  return MEMHIP_OK;
}

// memhip_seg_ohem_keys / _select / memhip_seg_ce_w and their plan query: memhip_seg_args_t's rules first, then the sampler's
int seg_ohem_plan(const memhip_segohem_args_t* a, int who, memhip_segohem_plan_t* p) {
  *p = memhip_segohem_plan_t{};
  MEMHIP_REQUIRE(a, "seg: null args");
  const int base = who == OHEM_KEYS ? SEG_INPUTS : who == OHEM_CE ? SEG_CE : SEG_QUERY;
  if (int rc = seg_plan(&a->seg, base, &p->seg, kMaxC * 4, false)) return rc;
  MEMHIP_REQUIRE(a->sampler >= 0 && a->sampler <= 2, "seg_ohem: sampler=%d must be 0 (none), 1 (thresh) or 2 (top-k)", a->sampler);
  if (a->sampler == 1)
    MEMHIP_REQUIRE(a->thresh > 0.f && a->thresh <= 1.f, "seg_ohem: thresh=%g must lie in (0, 1]", (double)a->thresh);
  if (a->sampler != 0) {
    MEMHIP_REQUIRE(a->min_kept >= 0 && a->min_kept <= kMaxMinKept, "seg_ohem: min_kept=%lld must lie in 0 .. 2^40", (long long)a->min_kept);
    MEMHIP_REQUIRE(a->keys && a->threshold, "seg_ohem: null pointer (keys, threshold) with sampler=%d", a->sampler);
    MEMHIP_REQUIRE(((uintptr_t)a->keys & 3) == 0 && ((uintptr_t)a->threshold & 3) == 0, "seg_ohem: keys or threshold is not 4-byte aligned");
  }
  if (who == OHEM_KEYS || who == OHEM_SELECT)
    MEMHIP_REQUIRE(a->sampler != 0, "seg_ohem: sampler=0 has no keys (memhip_seg_ohem_keys and _select need sampler 1 or 2)");
  if (who == OHEM_SELECT) {
    MEMHIP_REQUIRE(a->seg.stats && a->seg.workspace, "seg_ohem_select: null pointer (stats, workspace)");
    MEMHIP_REQUIRE(((uintptr_t)a->seg.workspace & 7) == 0, "seg_ohem_select: workspace is not 8-byte aligned");
  }

  const long long total = (long long)a->seg.B * a->seg.H * a->seg.W;
  const long long blocks = (total + kConfThreads - 1) / kConfThreads;
  p->keys_grid = (int)(blocks < kConfMaxGrid ? blocks : kConfMaxGrid);
  p->keys_block = kConfThreads;
  const long long sblocks = (total + kSelThreads - 1) / kSelThreads;
  p->select_grid = (int)(sblocks < kSelMaxGrid ? sblocks : kSelMaxGrid);
  p->select_block = kSelThreads;
  p->select_passes = kSelPasses;
  p->select_bins = kSelBins;
  p->select_lds_bytes = kSelBins * 4;
  p->select_ws_offset = (p->seg.ws_bytes + 7) & ~(uint64_t)7;
  p->select_ws_bytes = a->sampler ? select_ws_bytes() : 0;
  p->ws_bytes = p->select_ws_offset + p->select_ws_bytes;
  if ((who == OHEM_SELECT || who == OHEM_CE || a->seg.workspace) && a->seg.workspace_bytes < p->ws_bytes)
    return fail(MEMHIP_EWORKSPACE, "seg_ohem: workspace %zu < %zu", a->seg.workspace_bytes, (size_t)p->ws_bytes);
  return MEMHIP_OK;
}

}  // namespace memhip

extern "C" int memhip_seg_axis_table(int in, int out, int align_corners, int32_t* i0, float* w1, int32_t* lo, int32_t* hi) {
  return memhip::seg_axis_table(in, out, align_corners, i0, w1, lo, hi);
}

extern "C" int memhip_seg_plan(const memhip_seg_args_t* args, memhip_seg_plan_t* out) {
  MEMHIP_REQUIRE(out, "seg_plan: null pointer");
  return memhip::seg_plan(args, memhip::SEG_QUERY, out);
}

extern "C" int memhip_seg_ohem_plan(const memhip_segohem_args_t* args, memhip_segohem_plan_t* out) {
  MEMHIP_REQUIRE(out, "seg_ohem_plan: null pointer");
  return memhip::seg_ohem_plan(args, memhip::OHEM_QUERY, out);
}
