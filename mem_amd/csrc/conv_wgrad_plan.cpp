// The rules of memhip_conv_wgrad_nhwc: what it accepts, and how it cuts the work (conv_wgrad_plan.hpp).
#include "common.h"
#include "conv_wgrad_plan.hpp"

namespace memhip {

int wgrad_validate(const memhip_conv_wgrad_args_t* a, bool query, WgradGeom* g) {
  MEMHIP_REQUIRE(a, "conv_wgrad: null args");
  MEMHIP_REQUIRE(a->B >= 0 && a->Hs > 0 && a->Ws > 0 && a->C > 0 && a->N > 0, "conv_wgrad: bad shape B=%d Hs=%d Ws=%d C=%d N=%d",
                 a->B, a->Hs, a->Ws, a->C, a->N);
  const bool f4 = a->ksize == 4 && a->stride == 2 && a->pad == 1, f3 = a->ksize == 3 && a->stride == 1 && a->pad == 1,
             f1 = a->ksize == 1 && a->stride == 1 && a->pad == 0;
  MEMHIP_REQUIRE(f4 || f3 || f1, "conv_wgrad: only the forms (4, 2, 1), (3, 1, 1), (1, 1, 0) are provided, got (%d, %d, %d)",
                 a->ksize, a->stride, a->pad);
  MEMHIP_REQUIRE(a->C % 8 == 0 || (a->C == 4 && f4), "conv_wgrad: C must be 4 (first layer, 4x4) or a multiple of 8, got %d", a->C);
  MEMHIP_REQUIRE(a->N % 8 == 0, "conv_wgrad: N must be a multiple of 8, got %d", a->N);
  MEMHIP_REQUIRE(a->small_padded == 0 || a->small_padded == 1, "conv_wgrad: small_padded is 0 or 1");
  MEMHIP_REQUIRE(a->accumulate == 0 || a->accumulate == 1, "conv_wgrad: accumulate is 0 or 1");
  *g = wgrad_geom(*a);
  MEMHIP_REQUIRE(g->M <= (int64_t)1 << 30 && (int64_t)a->B * g->Hbp * g->Wbp <= (int64_t)1 << 31 &&
                     (int64_t)a->ksize * a->ksize * a->C <= 1 << 24 && a->N <= 1 << 24,
                 "conv_wgrad: too many pixels or channels");
  if (query || g->M == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(a->small && a->big && a->grad, "conv_wgrad: null pointer");
  MEMHIP_REQUIRE(((uintptr_t)a->small & 15) == 0 && ((uintptr_t)a->big & 15) == 0, "conv_wgrad: small and big must be 16-byte aligned");
  return MEMHIP_OK;
}

WgradPlan wgrad_plan(const WgradGeom& g, int device_cus) {
  WgradPlan p = {};
  p.M = g.M;
  p.K = g.K;
  p.Hbp = g.Hbp;
  p.Wbp = g.Wbp;
  if (g.M == 0) return p;
  p.tiles_n = cdiv(g.N, kWgTile);
  p.tiles_k = cdiv(g.K, kWgTile);
  const int tiles = p.tiles_n * p.tiles_k;
  // two workgroups fit a CU: as many slices as fill those slots ONCE (one slice more would add a second, nearly empty round of
  // workgroups that each still walk a whole slice)
  const WgradSlices s = wgrad_slices(g.M, 2 * (device_cus > 0 ? device_cus : 1) / tiles);
  p.splits = s.splits;
  p.rows_per_split = s.rows_per_split;
  p.grid = tiles * s.splits;
  p.block = kWgThreads;
  p.lds_bytes = kWgLdsBytes;
  if (s.splits > 1) {
    p.ws_bytes = (int64_t)s.splits * g.N * g.K * (int64_t)sizeof(float);
    p.fold_grid = cdiv((int64_t)g.N * g.K, 256);
  }
  return p;
}

}  // namespace memhip
