// The dispatch policy of the event rasterizer (memhip_rasterize, one memhip_raster_args_t for every form): what a call must
// look like, which of the four kernel families it gets, the bands, the grids, the workspace layout and what is cleared in
// front of the launches.  Every shape test, option test and grid formula is here, once; the launcher (raster.hip) obeys.
#include "raster_plan.hpp"
#include "common.h"

namespace memhip {
namespace {
using namespace raster;

uint64_t align16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

void push(memhip_raster_plan_t& p, int kernel, int grid_x, int grid_y, int block, int lds) {
  p.l[p.count++] = memhip_raster_launch_t{kernel, grid_x, grid_y, block, lds};
}

// bands of whole pixels (not rows): band_px pixels each, the last one shorter, none empty
bool bin_geometry(long long HW, int* band_px, int* nb, int want_nb) {
  long long n = (HW + kBinBandPixels - 1) / kBinBandPixels;
  if (want_nb > n && want_nb <= kBinMaxBands) n = want_nb;
  if (n > kBinMaxBands) return false;
  long long px = (HW + n - 1) / n;
  px = (px + 3) & ~3ll;                     // 4-pixel aligned bands keep the u32 output stores
  if (px > kBinBandPixels) px = kBinBandPixels;
  n = (HW + px - 1) / px;                   // the bands the rounded width needs: a small canvas has fewer than asked for
  if (n > kBinMaxBands) return false;
  *band_px = (int)px;
  *nb = (int)n;
  return true;
}

// Bands per sample for a batch of B samples.  Pass 2 runs one workgroup per (sample, band); a workgroup with > 80 KB of counters has a
// CU to itself and takes ~0.22 us per 1000 pixels of its band (launch, clearing and writing its planes) + ~220 us per million events /
// bands (its keys), so what the pass costs is set by how many ROUNDS of workgroups the chip needs.  480 x 640 needs eight bands of
// 38 400 pixels: 32 samples are 256 workgroups = one round (36.9 us under rocprofv3; the ten 15-bit-key bands of the first half of
// round 6 were 320 workgroups = two rounds, 44.3 us), 64 samples two rounds (72 us; twelve bands = three rounds of smaller workgroups:
// 68 us -- the model calls them equal).  The candidates run from the fewest bands the LDS allows to twice that; more bands cost pass 1
// padding and shorter segments, so a larger count has to promise 10 % and batches that fit one round keep the fewest bands.
int choose_bands(long long HW, int B, long long n_events, int forced, int device_cus) {
  if (forced > 0) return forced;
  const int nmin = (int)((HW + kBinBandPixels - 1) / kBinBandPixels);
  int cus = device_cus >= 0 ? device_cus : max_cus();
  if (cus <= 0) cus = 256;
  if ((long long)B * nmin <= cus) return nmin;                                  // one round either way
  int best = nmin;
  double best_cost = 0.0;
  for (int nbv = nmin; nbv <= 2 * nmin + 4 && nbv <= kBinMaxBands; ++nbv) {
    const long long px = ((HW + nbv - 1) / nbv + 3) & ~3ll;
    const int per_cu = (size_t)px * 4 * 2 + 1024 <= 160 * 1024 ? 2 : 1;       // 1024-thread workgroups: two per CU at most
    const long long rounds = ((long long)B * nbv + (long long)cus * per_cu - 1) / ((long long)cus * per_cu);
    const double cost = (double)rounds * (0.22e-3 * (double)px + 220.0e-6 * ((double)n_events / B) / nbv) * (per_cu == 2 ? 2.0 : 1.0);
    if (nbv == nmin || cost < best_cost * 0.9) { best = nbv; best_cost = cost; }
  }
  return best;
}

}  // namespace

int raster_plan(const memhip_raster_args_t* a, bool query, const RasterOptions& o, int device_cus, memhip_raster_plan_t* p) {
  *p = memhip_raster_plan_t{};
  MEMHIP_REQUIRE(a, "rasterize: null args");
  const int B = a->B, H = a->H, W = a->W;
  MEMHIP_REQUIRE(B >= 0 && H > 0 && W > 0, "rasterize: bad shape B=%d H=%d W=%d", B, H, W);
  MEMHIP_REQUIRE(a->n_events >= 0, "rasterize: n_events=%lld must not be negative", (long long)a->n_events);
  const int form = a->form;
  MEMHIP_REQUIRE(form == MEMHIP_RASTER_AUTO || form == MEMHIP_RASTER_SINGLE || form == MEMHIP_RASTER_BINNED,
                 "rasterize: unknown form %d", form);
  const bool ts = a->time_surface != 0, var = a->dims != nullptr;
  MEMHIP_REQUIRE(form != MEMHIP_RASTER_BINNED || (!ts && !var),
                 "rasterize: the binned form has no time surface and no per-sample canvases (dims)");
  if (B == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(query || (a->ev && a->offsets && a->out && a->status && a->workspace), "rasterize: null pointer");
  MEMHIP_REQUIRE(((uintptr_t)a->ev & 15) == 0, "rasterize: ev must be 16-byte aligned");
  const long long HW = (long long)H * W;
  const bool out4 = ((uintptr_t)a->out & 3) == 0;
  const uint64_t status_bytes = (uint64_t)B * sizeof(int32_t);

  if (form == MEMHIP_RASTER_BINNED ||
      (form == MEMHIP_RASTER_AUTO && !ts && !var && HW <= (long long)kBinMaxBands * kBinBandPixels)) {
    // ---- two passes: keys sorted by (band, polarity) per chunk of kBinChunk events, then LDS counters per (sample, band).
    // Nothing is cleared: pass 1 writes every header and slot pass 2 reads, pass 2 writes status and every pixel.
    MEMHIP_REQUIRE(out4, "rasterize: out must be 4-byte aligned for the binned form");
    int band_px = 0, nb = 0;
    if (!bin_geometry(HW, &band_px, &nb, choose_bands(HW, B, a->n_events, o.raster_bands, device_cus)))
      return fail(MEMHIP_EUNSUPPORTED, "rasterize: %dx%d canvas needs more than %d bands", H, W, kBinMaxBands);
    p->family = MEMHIP_RASTER_BINNED;
    p->band_px = band_px; p->nb = nb;
    const uint64_t chunks = (uint64_t)a->n_events / kBinChunk + (uint64_t)B + 1;     // every sample starts a chunk of its own
    p->off_keys = 0;
    p->off_hdr = align16(chunks * kBinSlots * sizeof(unsigned short));
    p->off_bad_slots = p->off_hdr + chunks * kBinHdr * sizeof(unsigned int);
    p->ws_bytes = p->off_bad_slots + ((uint64_t)kBinKeyGrid + (uint64_t)B) * sizeof(int32_t);   // one slot per pass-1 workgroup
    // chunks per sample are only known on the device: enough workgroups per sample to fill the chip at small B, grid-stride
    // beyond (4096 workgroups in all: 64 x 1 M events 462 -> 454 us against 2048, 470 with 1024; 32 x 1 M: 241 / 241 / 246 /
    // 249 us with 4096 / 2048 / 1024 / 512)
    const long long avg_chunks = a->n_events / ((long long)B * kBinChunk) + 1;
    long long bx = (kBinKeyGrid + B - 1) / B;                                    // (bx * B <= kBinKeyGrid + B slots)
    if (bx > 4 * avg_chunks) bx = 4 * avg_chunks;
    if (bx < 1) bx = 1;
    p->bx = (int)bx;
    push(*p, MEMHIP_RASTER_K_BIN_KEYS, (int)bx, B, kBinThreads, 0);
    push(*p, MEMHIP_RASTER_K_BIN_ACCUM, nb, B, kAccThreads, band_px * 4);
  } else {
    // ---- one pass.  The workspace is sized for the global-atomic form whichever family runs.
    p->off_bins = 0;
    p->off_tstat = align16((uint64_t)B * 3 * HW * sizeof(unsigned int));
    p->ws_bytes = p->off_tstat + (uint64_t)B * 2 * sizeof(unsigned long long);
    p->clear_status_bytes = status_bytes;
    // privatised counters (raster_lds_kernel): small canvas, no time surface
    int rpb = kBandPixels / W;
    const int bands = rpb > 0 ? cdiv(H, rpb) : kMaxBands + 1;
    if (o.raster_lds != 0 && !ts && !var && bands <= kMaxBands && out4) {
      rpb = cdiv(H, bands);                              // even bands
      p->family = MEMHIP_RASTER_LDS;
      p->rows_per_band = rpb; p->bands = bands;
      push(*p, MEMHIP_RASTER_K_LDS, bands, B, kLdsThreads, 2 * rpb * W * 4);
    } else {
      p->family = var ? MEMHIP_RASTER_GLOBAL_VAR : MEMHIP_RASTER_GLOBAL;
      p->clear_ws_bytes = p->ws_bytes;
      if (var) p->clear_out_bytes = (uint64_t)B * 3 * HW;   // the rest of every slot reads zero
      // enough blocks per sample to fill the chip at small B, grid-stride beyond
      const int bx = B >= 256 ? 8 : (B >= 32 ? 32 : 256);
      push(*p, MEMHIP_RASTER_K_COUNT, bx, B, kThreads, 0);
      long long fx = (HW + kThreads - 1) / kThreads;
      if (fx > 64) fx = 64;
      push(*p, MEMHIP_RASTER_K_FINALIZE, (int)fx, B, kThreads, 0);
    }
  }
  if ((!query || a->workspace) && a->workspace_bytes < p->ws_bytes)
    return fail(MEMHIP_EWORKSPACE, "rasterize: workspace %zu < %zu", a->workspace_bytes, (size_t)p->ws_bytes);
  return MEMHIP_OK;
}

}  // namespace memhip

extern "C" int memhip_rasterize_plan(const memhip_raster_args_t* args, int device_cus, memhip_raster_plan_t* out) {
  using namespace memhip;
  MEMHIP_REQUIRE(out, "rasterize_plan: null pointer");
  return raster_plan(args, true, RasterOptions{opt(OPT_RASTER_LDS), opt(OPT_RASTER_BANDS)}, device_cus, out);
}
