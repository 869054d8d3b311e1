// Host-only exercise of seg_plan.cpp for the sanitizers: memhip_seg_axis_table over every (in, out, align_corners) up to a
// few hundred outputs with its arrays allocated at their exact sizes, and memhip_seg_plan over a few hundred thousand
// memhip_seg_args_t, accepted and rejected, with the invariants the launcher and the kernel rely on checked on the way; then
// memhip_seg_ohem_plan over a hundred thousand memhip_segohem_args_t in the same way.
// The one variable of core.cpp it needs is defined here; no device:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/seg_plan_sanitize.cpp mem_amd/csrc/seg_plan.cpp -o seg_plan_sanitize && ./seg_plan_sanitize
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../mem_amd/csrc/common.h"
#include "../mem_amd/csrc/seg_plan.hpp"

namespace memhip {
thread_local char g_err[512];
}  // namespace memhip

static unsigned long long g_state = 20261;
static int rnd(int lo, int hi) {   // inclusive
  g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return lo + (int)((g_state >> 33) % (unsigned long long)(hi - lo + 1));
}
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::abort(); } } while (0)

int main() {
  using namespace memhip::seg;
  long long tables = 0, ok = 0, rejected = 0;
  for (int in = 1; in <= 40; ++in)
    for (int out = in; out <= 6 * in + 3; ++out)
      for (int align = 0; align < 2; ++align) {
        std::vector<int32_t> i0(out), lo(in), hi(in);
        std::vector<float> w1(out);
        CHECK(memhip_seg_axis_table(in, out, align, i0.data(), w1.data(), lo.data(), hi.data()) == MEMHIP_OK);
        for (int y = 0; y < out; ++y) {
          CHECK(i0[y] >= 0 && i0[y] < in && w1[y] >= 0.f && w1[y] <= 1.f + 1e-6f);
          CHECK(y == 0 || (i0[y] >= i0[y - 1] && i0[y] <= i0[y - 1] + 1));
        }
        for (int i = 0; i < in; ++i) {
          CHECK(lo[i] >= 0 && lo[i] <= hi[i] && hi[i] < out);
          CHECK(i == 0 || (lo[i] >= lo[i - 1] && hi[i] >= hi[i - 1]));
        }
        ++tables;
      }
  CHECK(memhip_seg_axis_table(0, 4, 0, nullptr, nullptr, nullptr, nullptr) == MEMHIP_EINVAL);
  void* const P = (void*)0x1000;
  memhip_seg_plan_t plan;
  CHECK(memhip_seg_plan(nullptr, &plan) == MEMHIP_EINVAL);
  for (int it = 0; it < 300000; ++it) {
    memhip_seg_args_t a = {};
    a.B = rnd(0, 29) ? rnd(1, 64) : rnd(-1, 0);
    a.C = rnd(0, 19) ? rnd(2, 32) : rnd(-1, 40);
    a.h = rnd(0, 29) ? rnd(1, 130) : rnd(-1, 0);
    a.w = rnd(0, 29) ? rnd(1, 130) : rnd(-1, 0);
    a.H = rnd(0, 19) ? a.h * rnd(1, 5) + rnd(0, 3) : rnd(-1, a.h > 0 ? a.h : 1);
    a.W = rnd(0, 19) ? a.w * rnd(1, 5) + rnd(0, 3) : rnd(-1, a.w > 0 ? a.w : 1);
    if (!rnd(0, 199)) a.H = 4096 + rnd(0, 40000);
    a.ignore_index = rnd(0, 19) ? 255 : rnd(-2, 257);
    a.align_corners = rnd(0, 29) ? rnd(0, 1) : rnd(-1, 2);
    a.avg_non_ignore = rnd(0, 29) ? rnd(0, 1) : 2;
    a.loss_weight = 1.f;
    if (rnd(0, 1)) { a.workspace = P; a.workspace_bytes = (size_t)rnd(0, 1 << 20); }
    const int rc = memhip_seg_plan(&a, &plan);
    if (rc == MEMHIP_EINVAL) { ++rejected; continue; }
    const bool fits = a.B >= 1 && a.C >= 2 && a.C <= kMaxC && a.h >= 1 && a.w >= 1 && a.H >= a.h && a.W >= a.w;
    CHECK(fits);
    CHECK(plan.tile_h == kTile && plan.tile_w == kTile && plan.block == kThreads && plan.chunk == kChunk);
    CHECK(plan.tiles_y == (a.h + kTile - 1) / kTile && plan.tiles_x == (a.w + kTile - 1) / kTile);
    CHECK(plan.grid == a.B * plan.tiles_y * plan.tiles_x && plan.grid >= 1);
    CHECK(plan.max_fh >= 1 && plan.max_fh <= a.H && plan.max_fw >= 1 && plan.max_fw <= a.W);
    CHECK(plan.lds_bytes > 0 && plan.lds_bytes <= kLdsLimit && plan.lds_bytes % 8 == 0);
    CHECK(plan.lds_bytes >= lds_fixed_bytes(padded_channels(a.C)) + (plan.tables_in_lds ? (plan.max_fh + plan.max_fw) * 8 : 0));
    CHECK(plan.ws_bytes == (uint64_t)plan.grid * sizeof(Partial) && plan.slot_bytes == (int)sizeof(Partial));
    CHECK(plan.conf_grid >= 1 && plan.conf_grid <= kConfMaxGrid && plan.conf_lds_bytes >= a.C * a.C * 4);
    CHECK(rc == MEMHIP_OK || (rc == MEMHIP_EWORKSPACE && a.workspace && a.workspace_bytes < plan.ws_bytes));
    ++ok;
  }
  // memhip_seg_ohem_plan: the same struct as the first member, the sampler's fields behind it
  long long ok_w = 0, rejected_w = 0;
  memhip_segohem_plan_t wplan;
  CHECK(memhip_seg_ohem_plan(nullptr, &wplan) == MEMHIP_EINVAL);
  for (int it = 0; it < 100000; ++it) {
    memhip_segohem_args_t a = {};
    a.seg.B = rnd(1, 64); a.seg.C = rnd(0, 19) ? rnd(2, 32) : rnd(-1, 40);
    a.seg.h = rnd(1, 130); a.seg.w = rnd(1, 130);
    a.seg.H = a.seg.h * rnd(1, 5) + rnd(0, 3); a.seg.W = a.seg.w * rnd(1, 5) + rnd(0, 3);
    a.seg.ignore_index = 255; a.seg.loss_weight = 1.f;
    a.sampler = rnd(0, 19) ? rnd(0, 2) : rnd(-1, 3);
    a.thresh = rnd(0, 9) ? 0.7f : (float)rnd(-1, 2);
    a.min_kept = rnd(0, 19) ? rnd(0, 200000) : -1;
    if (rnd(0, 9)) { a.keys = (float*)P; a.threshold = (float*)P; }
    if (rnd(0, 1)) { a.seg.workspace = P; a.seg.workspace_bytes = (size_t)rnd(0, 1 << 20); }
    const int rc = memhip_seg_ohem_plan(&a, &wplan);
    if (rc == MEMHIP_EINVAL) { ++rejected_w; continue; }
    CHECK(a.sampler >= 0 && a.sampler <= 2 && (a.sampler == 0 || (a.keys && a.threshold && a.min_kept >= 0)));
    CHECK(a.sampler != 1 || (a.thresh > 0.f && a.thresh <= 1.f));
    const memhip_seg_plan_t& q = wplan.seg;
    CHECK(q.grid == a.seg.B * q.tiles_y * q.tiles_x && q.lds_bytes <= kLdsLimit && q.lds_bytes % 8 == 0);
    CHECK(q.lds_bytes >= lds_fixed_bytes(padded_channels(a.seg.C)) + kMaxC * 4 + (q.tables_in_lds ? (q.max_fh + q.max_fw) * 8 : 0));
    CHECK(wplan.keys_grid >= 1 && wplan.keys_grid <= kConfMaxGrid && wplan.select_grid >= 1 && wplan.select_grid <= kSelMaxGrid);
    CHECK(wplan.select_bins == kSelBins && wplan.select_lds_bytes == kSelBins * 4 && wplan.select_passes == kSelPasses);
    CHECK(wplan.select_ws_offset % 8 == 0 && wplan.select_ws_offset >= q.ws_bytes && wplan.select_ws_offset < q.ws_bytes + 8);
    CHECK(wplan.select_ws_bytes == (a.sampler ? select_ws_bytes() : 0) && wplan.ws_bytes == wplan.select_ws_offset + wplan.select_ws_bytes);
    CHECK(rc == MEMHIP_OK || (rc == MEMHIP_EWORKSPACE && a.seg.workspace && a.seg.workspace_bytes < wplan.ws_bytes));
    ++ok_w;
  }
  std::printf("seg_plan_sanitize: %lld tables, %lld plans accepted, %lld rejected; ohem: %lld accepted, %lld rejected\n", tables, ok,
              rejected, ok_w, rejected_w);
  CHECK(ok > 100000 && rejected > 10000 && ok_w > 30000 && rejected_w > 3000);
  return 0;
}
