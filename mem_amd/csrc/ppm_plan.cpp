// The one place that reads a memhip_ppm_args_t, accepts or rejects it and sizes the launches of memhip_ppm_pool / _concat_fwd /
// _concat_bwd_sums / _bwd_apply / _dmap; the launchers (ppm.hip) obey.
#include "ppm_plan.hpp"
#include <cmath>

namespace memhip {
using namespace ppm;

namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

int ppm_plan(const memhip_ppm_args_t* a, int who, memhip_ppm_plan_t* p) {
  *p = memhip_ppm_plan_t{};
  MEMHIP_REQUIRE(a, "ppm: null args");
  const int B = a->B, Cin = a->Cin, C = a->C, h = a->h, w = a->w, n = a->n;
  MEMHIP_REQUIRE(B >= 0 && h >= 1 && w >= 1, "ppm: bad shape B=%d h=%d w=%d (B >= 0, h and w positive)", B, h, w);
  MEMHIP_REQUIRE(Cin > 0 && Cin % kChunk == 0, "ppm: bad shape Cin=%d (a positive multiple of 64)", Cin);
  MEMHIP_REQUIRE(C > 0 && C % kChunk == 0 && C <= kMaxC, "ppm: bad shape C=%d (a positive multiple of 64, at most %d)", C, kMaxC);
  MEMHIP_REQUIRE(n >= 1 && n <= MEMHIP_PPM_MAX_SCALES, "ppm: bad shape n=%d pool scales (1 <= n <= %d)", n, MEMHIP_PPM_MAX_SCALES);
  const long long R = (long long)B * h * w;
  MEMHIP_REQUIRE((long long)h * w <= (1 << 24) && R <= (1LL << 30), "ppm: bad shape B=%d h=%d w=%d, too many pixels", B, h, w);
  int bins = 0, tiles = 0;
  for (int i = 0; i < n; ++i) {
    const int s = a->scales[i];
    MEMHIP_REQUIRE(s >= 1 && s <= MEMHIP_PPM_MAX_SCALE, "ppm: bad pool scale %d (1 <= s <= %d)", s, MEMHIP_PPM_MAX_SCALE);
    MEMHIP_REQUIRE(s <= h && s <= w, "ppm: pool scale %d on a map of %dx%d (the resize never shrinks: s <= min(h, w))", s, h, w);
    MEMHIP_REQUIRE((long long)B * s * s <= (1LL << 24), "ppm: bad shape B=%d, too many rows at pool scale %d", B, s);
    bins += s * s;
    p->rows[i] = B * s * s;
    p->row_tile0[i] = tiles;
    tiles += cdiv(p->rows[i], kRows);
  }
  MEMHIP_REQUIRE(pool_lds_bytes(bins) <= kLdsLimit, "ppm: pool scales with %d bins need %d bytes of LDS, more than %d", bins,
                 pool_lds_bytes(bins), kLdsLimit);
  MEMHIP_REQUIRE((long long)B * (Cin / kChunk) <= 0x7fffffffLL && Cin / kChunk + n * (C / kChunk) <= 65535,
                 "ppm: bad shape B=%d Cin=%d C=%d, too many workgroups", B, Cin, C);

  p->R = R;
  p->block = kThreads;
  p->ct = Cin + n * C;
  p->bins = bins;
  p->pool_grid = B * (Cin / kChunk);
  p->pool_lds_bytes = pool_lds_bytes(bins);
  p->concat_grid_x = cdiv(R, kPixels);
  p->concat_grid_y = Cin / kChunk + n * (C / kChunk);
  p->gather_grid_x = tiles;
  p->gather_grid_y = C / kChunk;
  p->sums_grid_x = n;
  p->sums_grid_y = C / kChunk;
  p->dmap_grid_x = cdiv(R, kPixels);
  p->dmap_grid_y = Cin / kChunk;
  p->tile_lds_bytes = kTileLdsBytes;
  p->ws_bytes = 0;
  if (R == 0 || who == PPM_QUERY) return MEMHIP_OK;

  const bool bn = who == PPM_CONCAT || who == PPM_SUMS || who == PPM_APPLY;
  if (who == PPM_POOL || who == PPM_CONCAT) MEMHIP_REQUIRE(a->map, "ppm: null pointer (map)");
  if (bn) {
    MEMHIP_REQUIRE(a->mean && a->rstd && a->gamma && a->beta, "ppm: null pointer (mean, rstd, gamma, beta)");
    MEMHIP_REQUIRE(aligned16(a->mean) && aligned16(a->rstd) && aligned16(a->gamma) && aligned16(a->beta),
                   "ppm: mean, rstd, gamma or beta is not 16-byte aligned");
  }
  if (who == PPM_CONCAT) MEMHIP_REQUIRE(a->xcat && aligned16(a->xcat), "ppm_concat_fwd: xcat is null or not 16-byte aligned");
  if (who == PPM_SUMS || who == PPM_DMAP) MEMHIP_REQUIRE(a->dxcat && aligned16(a->dxcat), "ppm: dxcat is null or not 16-byte aligned");
  if (who == PPM_SUMS) MEMHIP_REQUIRE(a->sums, "ppm_concat_bwd_sums: null pointer (sums)");
  if (who == PPM_APPLY && a->tot) MEMHIP_REQUIRE(aligned16(a->tot), "ppm_bwd_apply: tot is not 16-byte aligned");
  if (who == PPM_DMAP) MEMHIP_REQUIRE(a->dmap, "ppm_dmap: null pointer (dmap)");
  for (int i = 0; i < n; ++i) {
    if (who == PPM_POOL) MEMHIP_REQUIRE(a->P[i] && aligned16(a->P[i]), "ppm_pool: P[%d] is null or not 16-byte aligned", i);
    if (bn) MEMHIP_REQUIRE(a->Y[i] && aligned16(a->Y[i]), "ppm: Y[%d] is null or not 16-byte aligned", i);
    if (who == PPM_CONCAT || who == PPM_SUMS)
      MEMHIP_REQUIRE(a->y_i0[i] && a->y_w1[i] && a->y_lo[i] && a->y_hi[i] && a->x_i0[i] && a->x_w1[i] && a->x_lo[i] && a->x_hi[i],
                     "ppm: null pointer (axis tables of scale %d)", i);
    if (who == PPM_SUMS || who == PPM_APPLY) MEMHIP_REQUIRE(a->g[i] && aligned16(a->g[i]), "ppm: g[%d] is null or not 16-byte aligned", i);
    if (who == PPM_APPLY) {
      MEMHIP_REQUIRE(a->dY[i] && aligned16(a->dY[i]), "ppm_bwd_apply: dY[%d] is null or not 16-byte aligned", i);
      if (a->tot)
        MEMHIP_REQUIRE(a->inv_n[i] > 0.f && std::isfinite(a->inv_n[i]), "ppm_bwd_apply: inv_n[%d]=%g must be positive (1 / elements per channel)",
                       i, (double)a->inv_n[i]);
    }
    if (who == PPM_DMAP) MEMHIP_REQUIRE(a->dP[i] && aligned16(a->dP[i]), "ppm_dmap: dP[%d] is null or not 16-byte aligned", i);
  }
  return MEMHIP_OK;
}

}  // namespace memhip

extern "C" int memhip_ppm_plan(const memhip_ppm_args_t* args, memhip_ppm_plan_t* out) {
  MEMHIP_REQUIRE(out, "ppm_plan: null pointer");
  return memhip::ppm_plan(args, memhip::PPM_QUERY, out);
}

extern "C" int memhip_ppm_bins(int n, int s, int32_t* start, int32_t* end) {
  MEMHIP_REQUIRE(n >= 1 && s >= 1 && s <= n && n <= (1 << 24) / (s + 1), "ppm_bins: bad shape n=%d s=%d (1 <= s <= n)", n, s);
  MEMHIP_REQUIRE(start && end, "ppm_bins: null pointer");
  for (int i = 0; i < s; ++i) {
    start[i] = memhip::ppm::bin_start(i, n, s);
    end[i] = memhip::ppm::bin_end(i, n, s);
  }
  return MEMHIP_OK;
}
