// Host-only exercise of seg_predict_plan.cpp for the sanitizers: memhip_seg_predict_plan over a few hundred thousand
// memhip_segpredict_args_t with up to 64 (and more) rectangles, accepted and rejected; the cover verdict and the largest
// count are compared with a brute-force count map of the canvas.  The one variable of core.cpp it needs is defined here;
// no device:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/seg_predict_plan_sanitize.cpp mem_amd/csrc/seg_predict_plan.cpp -o seg_predict_plan_sanitize && ./seg_predict_plan_sanitize
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../mem_amd/csrc/common.h"
#include "../mem_amd/csrc/seg_plan.hpp"
#include "../mem_amd/csrc/seg_predict_plan.hpp"

namespace memhip {
thread_local char g_err[512];
}  // namespace memhip

static unsigned long long g_state = 20262;
static int rnd(int lo, int hi) {   // inclusive
  g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return lo + (int)((g_state >> 33) % (unsigned long long)(hi - lo + 1));
}
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::abort(); } } while (0)

int main() {
  using namespace memhip::segp;
  void* const P = (void*)0x1000;
  long long ok = 0, rejected = 0, uncovered = 0;
  memhip_segpredict_plan_t plan;
  CHECK(memhip_seg_predict_plan(nullptr, &plan) == MEMHIP_EINVAL);
  for (int it = 0; it < 200000; ++it) {
    memhip_segpredict_args_t a = {};
    a.B = rnd(0, 29) ? rnd(1, 16) : rnd(-1, 0);
    a.C = rnd(0, 29) ? rnd(2, 32) : rnd(-1, 40);
    a.H = rnd(1, 40);
    a.W = rnd(1, 70);
    a.hc = rnd(0, 29) ? rnd(1, a.H) : a.H + 1;
    a.wc = rnd(0, 29) ? rnd(1, a.W) : a.W + 1;
    a.h = rnd(0, 29) ? rnd(1, a.hc) : a.hc + 1;
    a.w = rnd(0, 29) ? rnd(1, a.wc) : rnd(-1, 0);
    a.align_corners = rnd(0, 39) ? rnd(0, 1) : 2;
    a.ignore_index = rnd(0, 39) ? 255 : rnd(-2, 257);
    const int V = rnd(0, 19) ? rnd(1, kMaxViews) : rnd(0, 1) * (kMaxViews + 1);
    a.V = V;
    std::vector<int32_t> rects(3 * (size_t)V);              // exactly V records: a read past them is caught
    const bool two = rnd(0, 1);
    const bool inside = a.hc <= a.H && a.wc <= a.W;
    for (int v = 0; v < V; ++v) {
      // mostly a grid that covers, sometimes anywhere, rarely outside
      const int gy = inside ? a.H - a.hc : 0, gx = inside ? a.W - a.wc : 0;
      rects[3 * v] = rnd(0, 99) ? rnd(0, gy) : rnd(-1, gy + 1);
      rects[3 * v + 1] = rnd(0, 99) ? rnd(0, gx) : rnd(-1, gx + 1);
      if (rnd(0, 2) == 0) rects[3 * v] = rnd(0, 1) ? 0 : gy;
      if (rnd(0, 2) == 0) rects[3 * v + 1] = rnd(0, 1) ? 0 : gx;
      rects[3 * v + 2] = rnd(0, 199) ? (two ? v & 1 : 0) : 2;
    }
    a.rects = V ? rects.data() : (rnd(0, 1) ? nullptr : reinterpret_cast<const int32_t*>(P));
    const int outs = rnd(0, 15);
    if (outs & 1) a.pred = static_cast<uint8_t*>(P);
    if (outs & 2) a.prob = static_cast<float*>(P);
    if (outs & 4) { a.labels = static_cast<const uint8_t*>(P); a.confusion = static_cast<int64_t*>(P); }
    if (outs == 8) a.labels = static_cast<const uint8_t*>(P);
    const int rc = memhip_seg_predict_plan(&a, &plan);
    // the verdict by brute force
    bool fits = a.B >= 0;
    if (a.B == 0) { CHECK(rc == MEMHIP_OK); ++ok; continue; }
    fits = fits && V >= 1 && V <= kMaxViews && a.C >= 2 && a.C <= 32 && a.h >= 1 && a.w >= 1 && a.hc >= a.h && a.wc >= a.w && inside;
    fits = fits && (a.align_corners == 0 || a.align_corners == 1) && a.ignore_index >= -1 && a.ignore_index <= 255;
    int max_count = 0, passes = 0;
    bool covered = true;
    if (fits) {
      for (int v = 0; v < V; ++v) {
        const int y1 = rects[3 * v], x1 = rects[3 * v + 1], f = rects[3 * v + 2];
        fits = fits && (f == 0 || f == 1) && y1 >= 0 && x1 >= 0 && y1 + a.hc <= a.H && x1 + a.wc <= a.W;
      }
    }
    if (fits) {
      for (int f = 0; f < 2; ++f) {
        std::vector<int> cnt((size_t)a.H * a.W, 0);
        bool present = false;
        for (int v = 0; v < V; ++v) {
          if (rects[3 * v + 2] != f) continue;
          present = true;
          for (int y = rects[3 * v]; y < rects[3 * v] + a.hc; ++y)
            for (int x = rects[3 * v + 1]; x < rects[3 * v + 1] + a.wc; ++x) cnt[(size_t)y * a.W + x] += 1;
        }
        if (!present) continue;
        passes += 1;
        for (int c : cnt) {
          covered = covered && c >= 1;
          if (c > max_count) max_count = c;
        }
      }
      if (!covered) ++uncovered;
    }
    fits = fits && covered && (a.labels != nullptr) == (a.confusion != nullptr) && (a.pred || a.prob || a.confusion);
    CHECK((rc == MEMHIP_OK) == fits);
    if (rc != MEMHIP_OK) { CHECK(rc == MEMHIP_EINVAL && memhip::g_err[0]); ++rejected; continue; }
    CHECK(plan.tile_h == kTileH && plan.tile_w == kTileW && plan.block == kThreads && plan.pixels_per_thread == kPx);
    CHECK(plan.tiles_y == (a.H + kTileH - 1) / kTileH && plan.tiles_x == (a.W + kTileW - 1) / kTileW);
    CHECK(plan.grid == a.B * plan.tiles_y * plan.tiles_x && plan.grid >= 1);
    CHECK(plan.passes == passes && plan.max_count == max_count && plan.max_count >= 1 && plan.max_count <= V);
    CHECK(plan.padded_classes >= a.C && plan.padded_classes <= 32 && plan.padded_classes % 4 == 0 && plan.lds_bytes >= a.C * a.C * 4);
    CHECK(plan.pred_dwords == (a.pred != nullptr && a.W % 4 == 0));
    ++ok;
  }
  std::printf("seg_predict_plan_sanitize: %lld plans accepted, %lld rejected (%lld for an uncovered pixel)\n", ok, rejected, uncovered);
  CHECK(ok > 10000 && rejected > 10000 && uncovered > 1000);
  return 0;
}
