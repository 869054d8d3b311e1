// memhip_seg_predict_plan: validation, cover check and launch sizes of memhip_seg_predict (seg_predict.hip).  Integer
// arithmetic only; the bilinear weights come from the tables of seg_plan.cpp.
#include "seg_predict_plan.hpp"
#include <algorithm>
#include "common.h"
#include "seg_plan.hpp"

namespace memhip {
using namespace segp;

namespace {

// sorted, distinct cut points of one axis: 0, n and both ends of every rectangle of the pass
int cuts_of(const int32_t* rects, int V, int f, int axis, int len, int n, int* out) {
  int m = 0;
  out[m++] = 0;
  out[m++] = n;
  for (int v = 0; v < V; ++v) {
    if (rects[3 * v + 2] != f) continue;
    out[m++] = rects[3 * v + axis];
    out[m++] = rects[3 * v + axis] + len;
  }
  std::sort(out, out + m);
  return (int)(std::unique(out, out + m) - out);
}

}  // namespace

int seg_predict_plan(const memhip_segpredict_args_t* a, bool query, memhip_segpredict_plan_t* p, int* passes) {
  *p = memhip_segpredict_plan_t{};
  *passes = 0;
  MEMHIP_REQUIRE(a, "seg_predict: null args");
  const int V = a->V, B = a->B, C = a->C, h = a->h, w = a->w, hc = a->hc, wc = a->wc, H = a->H, W = a->W;
  MEMHIP_REQUIRE(B >= 0, "seg_predict: bad shape B=%d (B >= 0)", B);
  if (B == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(V >= 1 && V <= kMaxViews, "seg_predict: bad shape V=%d (1 <= V <= %d views)", V, kMaxViews);
  MEMHIP_REQUIRE(C >= 2 && C <= seg::kMaxC, "seg_predict: bad shape C=%d (2 <= C <= %d)", C, seg::kMaxC);
  MEMHIP_REQUIRE(h >= 1 && w >= 1 && hc >= h && wc >= w,
                 "seg_predict: bad shape window %dx%d for logits of %dx%d (hc >= h >= 1 and wc >= w >= 1: the resize never shrinks)",
                 hc, wc, h, w);
  MEMHIP_REQUIRE(hc <= H && wc <= W, "seg_predict: bad shape window %dx%d on a canvas of %dx%d (hc <= H and wc <= W)", hc, wc, H, W);
  MEMHIP_REQUIRE(H <= seg::kMaxSide && W <= seg::kMaxSide, "seg_predict: bad shape H=%d W=%d (H, W <= %d)", H, W, seg::kMaxSide);
  MEMHIP_REQUIRE(a->align_corners == 0 || a->align_corners == 1, "seg_predict: align_corners=%d must be 0 or 1", a->align_corners);
  MEMHIP_REQUIRE(a->ignore_index >= -1 && a->ignore_index <= 255,
                 "seg_predict: ignore_index=%d must be a label 0..255, or -1 for none", a->ignore_index);
  const int tiles_y = cdiv(H, kTileH), tiles_x = cdiv(W, kTileW);
  MEMHIP_REQUIRE((long long)B * tiles_y * tiles_x <= 0x7fffffffLL, "seg_predict: bad shape B=%d H=%d W=%d, too many tiles", B, H, W);
  MEMHIP_REQUIRE(a->rects, "seg_predict: null pointer (rects)");
  for (int v = 0; v < V; ++v) {
    const int y1 = a->rects[3 * v], x1 = a->rects[3 * v + 1], f = a->rects[3 * v + 2];
    MEMHIP_REQUIRE(f == 0 || f == 1, "seg_predict: view %d has flip=%d, must be 0 or 1", v, f);
    MEMHIP_REQUIRE(y1 >= 0 && x1 >= 0 && y1 <= H - hc && x1 <= W - wc,
                   "seg_predict: view %d at (%d, %d) with a window of %dx%d leaves the canvas of %dx%d", v, y1, x1, hc, wc, H, W);
    *passes |= 1 << f;
  }
  // every pixel of every pass present is covered: between two neighbouring cut points of an axis no rectangle begins or
  // ends, so one corner stands for its cell
  int max_count = 0;
  int ys[2 * kMaxViews + 2], xs[2 * kMaxViews + 2];
  for (int f = 0; f < 2; ++f) {
    if (!(*passes >> f & 1)) continue;
    const int ny = cuts_of(a->rects, V, f, 0, hc, H, ys), nx = cuts_of(a->rects, V, f, 1, wc, W, xs);
    for (int i = 0; i + 1 < ny; ++i)
      for (int j = 0; j + 1 < nx; ++j) {
        int n = 0;
        for (int v = 0; v < V; ++v) {
          const int y1 = a->rects[3 * v], x1 = a->rects[3 * v + 1];
          n += a->rects[3 * v + 2] == f && ys[i] >= y1 && ys[i] < y1 + hc && xs[j] >= x1 && xs[j] < x1 + wc;
        }
        MEMHIP_REQUIRE(n >= 1, "seg_predict: pixel (%d, %d) of the pass with flip=%d is covered by no view", ys[i], xs[j], f);
        max_count = std::max(max_count, n);
      }
  }
  MEMHIP_REQUIRE((a->labels != nullptr) == (a->confusion != nullptr),
                 "seg_predict: labels and confusion go together (both set or both NULL)");
  MEMHIP_REQUIRE(a->pred || a->prob || a->confusion, "seg_predict: no output (pred, prob, or labels with confusion)");
  if (!query) {
    MEMHIP_REQUIRE(a->logits, "seg_predict: null pointer (logits)");
    MEMHIP_REQUIRE(a->y_i0 && a->y_w1 && a->x_i0 && a->x_w1, "seg_predict: null pointer (axis tables)");
  }
  p->tile_h = kTileH;
  p->tile_w = kTileW;
  p->tiles_y = tiles_y;
  p->tiles_x = tiles_x;
  p->grid = B * tiles_y * tiles_x;
  p->block = kThreads;
  p->lds_bytes = seg::kMaxC * seg::kMaxC * 4;
  p->pixels_per_thread = kPx;
  p->padded_classes = seg::padded_channels(C);
  p->passes = (*passes & 1) + (*passes >> 1 & 1);
  p->max_count = max_count;
  p->pred_dwords = a->pred && W % 4 == 0 && ((uintptr_t)a->pred & 3) == 0;
  return MEMHIP_OK;
}

}  // namespace memhip

extern "C" int memhip_seg_predict_plan(const memhip_segpredict_args_t* args, memhip_segpredict_plan_t* out) {
  MEMHIP_REQUIRE(out, "seg_predict_plan: null pointer");
  int passes;
  return memhip::seg_predict_plan(args, true, out, &passes);
}
