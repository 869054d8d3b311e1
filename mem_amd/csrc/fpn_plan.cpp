// The one place that reads a memhip_fpn_args_t, accepts or rejects it and sizes the launches of memhip_fpn_topdown_fwd /
// _concat_fwd / _resize_bwd / _bn_bwd_sums / _bn_bwd_apply; the launchers (fpn.hip) obey.
#include "fpn_plan.hpp"
#include <algorithm>
#include <cmath>

namespace memhip {
using namespace fpn;

namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

int fpn_plan(const memhip_fpn_args_t* a, int who, memhip_fpn_plan_t* p) {
  *p = memhip_fpn_plan_t{};
  MEMHIP_REQUIRE(a, "fpn: null args");
  const int B = a->B, C = a->C, L = a->L, lv = a->level;
  MEMHIP_REQUIRE(B >= 0, "fpn: bad shape B=%d (B >= 0)", B);
  MEMHIP_REQUIRE(C > 0 && C % kChunk == 0 && C <= kMaxC, "fpn: bad shape C=%d (a positive multiple of 64, at most %d)", C, kMaxC);
  MEMHIP_REQUIRE(L >= 2 && L <= MEMHIP_FPN_MAX_LEVELS, "fpn: bad shape L=%d levels (2 <= L <= %d)", L, MEMHIP_FPN_MAX_LEVELS);
  for (int l = 0; l < L; ++l) {
    MEMHIP_REQUIRE(a->h[l] >= 1 && a->w[l] >= 1, "fpn: bad shape of level %d: %dx%d (h and w positive)", l, a->h[l], a->w[l]);
    if (l)
      MEMHIP_REQUIRE(a->h[l] <= a->h[l - 1] && a->w[l] <= a->w[l - 1],
                     "fpn: level %d of %dx%d above level %d of %dx%d (the resize never shrinks: sizes are non-increasing)", l, a->h[l],
                     a->w[l], l - 1, a->h[l - 1], a->w[l - 1]);
  }
  MEMHIP_REQUIRE((long long)a->h[0] * a->w[0] <= (1 << 24) && (long long)B * a->h[0] * a->w[0] <= (1LL << 30),
                 "fpn: bad shape B=%d h=%d w=%d, too many pixels", B, a->h[0], a->w[0]);
  MEMHIP_REQUIRE(lv >= 0 && lv < L, "fpn: bad level %d (0 <= level < L=%d)", lv, L);

  p->block = kThreads;
  p->ct = L * C;
  p->grid_y = C / kChunk;
  for (int l = 0; l < L; ++l) {
    const long long R = (long long)B * a->h[l] * a->w[l];
    p->R[l] = R;
    p->topdown_grid_x[l] = l < L - 1 ? cdiv(R, kPixels) : 0;
    p->resize_grid_x[l] = cdiv(R, kRows);
    p->sums_grid_x[l] = (int)std::min<long long>(cdiv(R, kRows), kGroups);
    p->apply_grid_x[l] = cdiv(R, kPixels);
  }
  p->concat_grid_x = cdiv(p->R[0], kPixels);
  p->concat_grid_y = L * (C / kChunk);
  p->sums_lds_bytes = kSumsLdsBytes;
  p->slot_floats = 2 * C;
  p->fold_grid = cdiv(p->slot_floats, kThreads);
  p->ws_bytes = (uint64_t)kGroups * p->slot_floats * sizeof(float);
  if (B == 0) return MEMHIP_OK;
  if (a->workspace && (who == FPN_QUERY || who == FPN_SUMS))
    MEMHIP_REQUIRE(a->workspace_bytes >= p->ws_bytes, "fpn_bn_bwd_sums: workspace of %zu bytes, %llu needed", a->workspace_bytes,
                   (unsigned long long)p->ws_bytes);
  if (who == FPN_QUERY) return MEMHIP_OK;

  if (who != FPN_RESIZE) {
    MEMHIP_REQUIRE(a->mean && a->rstd && a->gamma && a->beta, "fpn: null pointer (mean, rstd, gamma, beta)");
    MEMHIP_REQUIRE(aligned16(a->mean) && aligned16(a->rstd) && aligned16(a->gamma) && aligned16(a->beta),
                   "fpn: mean, rstd, gamma or beta is not 16-byte aligned");
  }
  auto need_y = [&](int l) {
    MEMHIP_REQUIRE(a->Y[l] && aligned16(a->Y[l]), "fpn: Y[%d] is null or not 16-byte aligned", l);
    return MEMHIP_OK;
  };
  if (who == FPN_TOPDOWN) {
    MEMHIP_REQUIRE(lv <= L - 2, "fpn_topdown_fwd: bad level %d (the coarsest level %d has no source)", lv, L - 1);
    if (int rc = need_y(lv)) return rc;
    if (!a->src) {
      MEMHIP_REQUIRE(lv == L - 2, "fpn_topdown_fwd: null pointer (src) at level %d: only level %d reads Y[%d] in place of it", lv, L - 2, L - 1);
      if (int rc = need_y(lv + 1)) return rc;
    }
    MEMHIP_REQUIRE(aligned16(a->src), "fpn_topdown_fwd: src is not 16-byte aligned");
    MEMHIP_REQUIRE(a->T && aligned16(a->T), "fpn_topdown_fwd: T is null or not 16-byte aligned");
    MEMHIP_REQUIRE(a->ty_i0[lv] && a->ty_w1[lv] && a->tx_i0[lv] && a->tx_w1[lv], "fpn_topdown_fwd: null pointer (axis tables t of level %d)", lv);
  }
  if (who == FPN_CONCAT) {
    for (int l = 0; l < L; ++l) {
      if (int rc = need_y(l)) return rc;
      MEMHIP_REQUIRE(a->cy_i0[l] && a->cy_w1[l] && a->cx_i0[l] && a->cx_w1[l], "fpn_concat_fwd: null pointer (axis tables c of level %d)", l);
    }
    MEMHIP_REQUIRE(a->xcat && aligned16(a->xcat), "fpn_concat_fwd: xcat is null or not 16-byte aligned");
  }
  if (who == FPN_RESIZE) {
    MEMHIP_REQUIRE(a->rows && aligned16(a->rows), "fpn_resize_bwd: rows is null or not 16-byte aligned");
    MEMHIP_REQUIRE(a->own || a->dxcat || a->fine_rows, "fpn_resize_bwd: null pointer (own, dxcat and fine_rows: no term)");
    MEMHIP_REQUIRE(aligned16(a->own) && aligned16(a->dxcat) && aligned16(a->fine_rows), "fpn_resize_bwd: own, dxcat or fine_rows is not 16-byte aligned");
    if (a->dxcat) {
      MEMHIP_REQUIRE(a->slice >= 0 && a->slice < L, "fpn_resize_bwd: bad slice %d (0 <= slice < L=%d)", a->slice, L);
      MEMHIP_REQUIRE(a->cy_i0[lv] && a->cy_w1[lv] && a->cy_lo[lv] && a->cy_hi[lv] && a->cx_i0[lv] && a->cx_w1[lv] && a->cx_lo[lv] && a->cx_hi[lv],
                     "fpn_resize_bwd: null pointer (axis tables c of level %d)", lv);
    }
    if (a->fine_rows) {
      MEMHIP_REQUIRE(lv >= 1, "fpn_resize_bwd: fine_rows at level 0 (there is no finer level)");
      const int k = lv - 1;
      MEMHIP_REQUIRE(a->ty_i0[k] && a->ty_w1[k] && a->ty_lo[k] && a->ty_hi[k] && a->tx_i0[k] && a->tx_w1[k] && a->tx_lo[k] && a->tx_hi[k],
                     "fpn_resize_bwd: null pointer (axis tables t of level %d)", k);
    }
  }
  if (who == FPN_SUMS || who == FPN_APPLY) {
    if (int rc = need_y(lv)) return rc;
    MEMHIP_REQUIRE(a->rows && aligned16(a->rows), "fpn: rows is null or not 16-byte aligned");
  }
  if (who == FPN_SUMS) {
    MEMHIP_REQUIRE(a->sums, "fpn_bn_bwd_sums: null pointer (sums)");
    MEMHIP_REQUIRE(a->workspace && aligned16(a->workspace), "fpn_bn_bwd_sums: workspace is null or not 16-byte aligned");
  }
  if (who == FPN_APPLY) {
    MEMHIP_REQUIRE(a->dY && aligned16(a->dY), "fpn_bn_bwd_apply: dY is null or not 16-byte aligned");
    if (a->tot) {
      MEMHIP_REQUIRE(aligned16(a->tot), "fpn_bn_bwd_apply: tot is not 16-byte aligned");
      MEMHIP_REQUIRE(a->inv_n > 0.f && std::isfinite(a->inv_n), "fpn_bn_bwd_apply: inv_n=%g must be positive (1 / elements per channel)",
                     (double)a->inv_n);
    }
  }
  return MEMHIP_OK;
}

}  // namespace memhip

extern "C" int memhip_fpn_plan(const memhip_fpn_args_t* args, memhip_fpn_plan_t* out) {
  MEMHIP_REQUIRE(out, "fpn_plan: null pointer");
  return memhip::fpn_plan(args, memhip::FPN_QUERY, out);
}
