// The one place that reads a memhip_bnhead_args_t, accepts or rejects it and sizes the launches of memhip_bnhead_fwd /
// _bwd_sums / _bwd_apply; the launchers (seg_head.hip) obey.
#include "seg_head_plan.hpp"
#include <cmath>
#include "common.h"

namespace memhip {
using namespace seghead;

namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

int bnhead_plan(const memhip_bnhead_args_t* a, int who, memhip_bnhead_plan_t* p) {
  *p = memhip_bnhead_plan_t{};
  MEMHIP_REQUIRE(a, "bnhead: null args");
  const int B = a->B, C = a->C, K = a->K, h = a->h, w = a->w;
  MEMHIP_REQUIRE(B >= 0 && h >= 1 && w >= 1, "bnhead: bad shape B=%d h=%d w=%d (B >= 0, h and w positive)", B, h, w);
  MEMHIP_REQUIRE(C > 0 && C % kChunk == 0 && C <= kMaxC, "bnhead: bad shape C=%d (a positive multiple of 64, at most %d)", C, kMaxC);
  MEMHIP_REQUIRE(K >= 2 && K <= kMaxK, "bnhead: bad shape K=%d (2 <= K <= %d)", K, kMaxK);
  const long long R = (long long)B * h * w;
  MEMHIP_REQUIRE((long long)h * w <= (1 << 24) && R <= (1LL << 30), "bnhead: bad shape B=%d h=%d w=%d, too many pixels", B, h, w);
  if (who == BNHEAD_FWD || a->ld != 0)
    MEMHIP_REQUIRE(a->ld >= K, "bnhead_fwd: ld=%lld < K=%d", (long long)a->ld, K);
  if (a->dropout)
    MEMHIP_REQUIRE(a->dropout->thr < 65536u && std::isfinite(a->dropout->scale) && a->dropout->row0 >= 0,
                   "bnhead: bad dropout (thr=%u < 65536, a finite scale, row0 >= 0)", a->dropout->thr);

  const int KP = padded_classes(K);
  p->R = R;
  p->kp = KP;
  p->block = kThreads;
  const long long tiles32 = (R + kFwdPixels - 1) / kFwdPixels, tiles64 = (R + kBwdPixels - 1) / kBwdPixels;
  p->fwd_grid = (int)(tiles32 < kFwdMaxGrid ? tiles32 : kFwdMaxGrid);
  p->fwd_lds_bytes = fwd_lds_bytes(KP, C);
  p->sums_grid_x = (int)(tiles64 < kGroups ? tiles64 : kGroups);
  p->sums_grid_y = C / kChunk;
  p->sums_lds_bytes = sums_lds_bytes(KP);
  p->apply_grid_x = (int)tiles32;
  p->apply_grid_y = C / kChunk;
  p->apply_lds_bytes = apply_lds_bytes(KP);
  p->slot_floats = 2 * C + K * C + K;
  p->fold_grid = cdiv(p->slot_floats, kThreads);
  p->ws_bytes = (uint64_t)p->sums_grid_x * p->slot_floats * sizeof(float);
  if (R == 0) return MEMHIP_OK;

  if (who != BNHEAD_QUERY) {
    MEMHIP_REQUIRE(a->y && a->mean && a->rstd && a->gamma && a->beta && a->wcls,
                   "bnhead: null pointer (y, mean, rstd, gamma, beta, wcls)");
    MEMHIP_REQUIRE(aligned16(a->y) && aligned16(a->mean) && aligned16(a->rstd) && aligned16(a->gamma) && aligned16(a->beta) &&
                       aligned16(a->wcls),
                   "bnhead: y, mean, rstd, gamma, beta or wcls is not 16-byte aligned");
  }
  if (who == BNHEAD_FWD) MEMHIP_REQUIRE(a->logits, "bnhead_fwd: null pointer (logits)");
  if (who == BNHEAD_SUMS || who == BNHEAD_APPLY) MEMHIP_REQUIRE(a->dlogit, "bnhead_bwd: null pointer (dlogit)");
  if (who == BNHEAD_SUMS) {
    MEMHIP_REQUIRE(a->sums && a->dwcls && a->dbias && a->workspace, "bnhead_bwd_sums: null pointer (sums, dwcls, dbias, workspace)");
    MEMHIP_REQUIRE(aligned16(a->workspace), "bnhead_bwd_sums: workspace is not 16-byte aligned");
  }
  if (who == BNHEAD_APPLY) {
    MEMHIP_REQUIRE(a->dy_out && aligned16(a->dy_out), "bnhead_bwd_apply: dy_out is null or not 16-byte aligned");
    if (a->tot) MEMHIP_REQUIRE(a->inv_n > 0.f && std::isfinite(a->inv_n), "bnhead_bwd_apply: inv_n=%g must be positive (1 / elements per channel)", (double)a->inv_n);
  }
  if ((who == BNHEAD_SUMS || (who == BNHEAD_QUERY && a->workspace)) && a->workspace_bytes < p->ws_bytes)
    return fail(MEMHIP_EWORKSPACE, "bnhead_bwd_sums: workspace %zu < %zu", a->workspace_bytes, (size_t)p->ws_bytes);
  return MEMHIP_OK;
}

}  // namespace memhip

extern "C" int memhip_bnhead_plan(const memhip_bnhead_args_t* args, memhip_bnhead_plan_t* out) {
  MEMHIP_REQUIRE(out, "bnhead_plan: null pointer");
  return memhip::bnhead_plan(args, memhip::BNHEAD_QUERY, out);
}
