// Host-only exercise of raster_plan.cpp for the sanitizers: memhip_rasterize_plan over a few hundred thousand
// memhip_raster_args_t -- every form and unknown ones, accepted and rejected shapes, time surface and per-sample canvases, null
// and misaligned addresses (the query reads no pointer), both options, 0..304 CUs -- with the invariants the launcher and the
// kernels rely on checked on the way.  The three functions of core.cpp it needs are stubbed here; no device:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/raster_plan_sanitize.cpp mem_amd/csrc/raster_plan.cpp -o raster_plan_sanitize && ./raster_plan_sanitize
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../mem_amd/csrc/common.h"
#include "../mem_amd/csrc/raster_plan.hpp"

static int g_lds = 1, g_bands = 0;
namespace memhip {
thread_local char g_err[512];
int opt(int id) { return id == OPT_RASTER_LDS ? g_lds : id == OPT_RASTER_BANDS ? g_bands : 0; }
int max_cus() { return 256; }
}  // namespace memhip

static unsigned long long g_state = 20261;
static int rnd(int lo, int hi) {   // inclusive
  g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return lo + (int)((g_state >> 33) % (unsigned long long)(hi - lo + 1));
}
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::abort(); } } while (0)

int main() {
  using namespace memhip::raster;
  static const int bands[] = {0, 0, 0, 1, 2, 10, 13, 16, 40, 64, 65, -1};
  long long ok = 0, rejected = 0, launches = 0, family[6] = {};
  memhip_raster_plan_t plan;
  CHECK(memhip_rasterize_plan(nullptr, 256, &plan) == MEMHIP_EINVAL);
  CHECK(memhip_rasterize_plan(nullptr, 256, nullptr) == MEMHIP_EINVAL);
  for (int it = 0; it < 400000; ++it) {
    g_lds = rnd(0, 3) != 0;
    g_bands = bands[rnd(0, 11)];
    memhip_raster_args_t a = {};
    a.B = rnd(0, 29) ? rnd(1, 320) : rnd(-1, 0);
    a.H = rnd(0, 29) ? rnd(1, rnd(0, 3) ? 700 : 40) : rnd(-3, 0);
    a.W = rnd(0, 29) ? rnd(1, rnd(0, 3) ? 1000 : 40) : rnd(-3, 0);
    if (!rnd(0, 15)) { a.H = rnd(1500, 1700); a.W = rnd(1500, 1700); }          // around the band limit of 64 x 40 000 pixels
    if (!rnd(0, 15)) { a.H = 1; a.W = rnd(14000, 15000); }                       // around one row of LDS counters
    a.time_surface = rnd(0, 3) == 0;
    a.form = rnd(0, 19) ? rnd(0, 2) : rnd(-1, 6);
    a.n_events = rnd(0, 19) ? (int64_t)rnd(0, 4) * rnd(0, 1 << 20) * (rnd(0, 1) ? a.B : 1) : -1;
    if (a.n_events < -1) a.n_events = 0;
    const uintptr_t P = 0x1000;
    if (rnd(0, 1)) { a.ev = (const double*)P; a.offsets = (const int64_t*)P; a.status = (int32_t*)P; }
    if (rnd(0, 1)) a.out = (uint8_t*)(P + (rnd(0, 3) ? 0 : rnd(1, 3)));
    if (!rnd(0, 19)) a.ev = (const double*)(P + 8);
    if (!rnd(0, 5)) a.dims = (const int32_t*)P;
    if (rnd(0, 3) == 0) a.aug = (const memhip_event_aug_t*)P;
    if (rnd(0, 1)) { a.workspace = (void*)P; a.workspace_bytes = rnd(0, 3) ? (size_t)1 << 40 : (size_t)rnd(0, 1 << 20); }
    const int cus = 8 * rnd(0, 38);
    const int rc = memhip_rasterize_plan(&a, rnd(0, 9) ? cus : -1, &plan);
    CHECK(rc == MEMHIP_OK || rc == MEMHIP_EINVAL || rc == MEMHIP_EUNSUPPORTED || rc == MEMHIP_EWORKSPACE);
    if (rc != MEMHIP_OK) { ++rejected; CHECK(memhip::g_err[0]); continue; }
    ++ok;
    CHECK(plan.family >= 0 && plan.family < 6);
    ++family[plan.family];
    CHECK((plan.family == 0) == (a.B == 0) && (plan.count == 0) == (a.B == 0));
    if (a.B == 0) continue;
    const long long HW = (long long)a.H * a.W;
    CHECK(!a.workspace || a.workspace_bytes >= plan.ws_bytes);
    if (plan.family == MEMHIP_RASTER_BINNED) {
      CHECK(!a.time_surface && !a.dims && a.form != MEMHIP_RASTER_SINGLE && ((uintptr_t)a.out & 3) == 0);
      CHECK(plan.count == 2 && plan.l[0].kernel == MEMHIP_RASTER_K_BIN_KEYS && plan.l[1].kernel == MEMHIP_RASTER_K_BIN_ACCUM);
      CHECK(plan.band_px % 4 == 0 && plan.band_px > 0 && plan.band_px <= kBinBandPixels && plan.nb >= 1 && plan.nb <= kBinMaxBands);
      CHECK((long long)(plan.nb - 1) * plan.band_px < HW && HW <= (long long)plan.nb * plan.band_px);   // no empty band; they tile
      CHECK(plan.l[1].grid_x == plan.nb && plan.l[1].lds == plan.band_px * 4 && plan.l[0].grid_x == plan.bx);
      CHECK(plan.bx >= 1 && (long long)plan.bx * a.B <= kBinKeyGrid + a.B);
      const uint64_t chunks = (uint64_t)a.n_events / kBinChunk + (uint64_t)a.B + 1;
      // keys: 16-byte loads; headers: at a 16-byte boundary; the per-workgroup int32 slots follow 129-word headers: 4 bytes
      CHECK(plan.off_keys == 0 && plan.off_hdr % 16 == 0 && plan.off_bad_slots % 4 == 0);
      CHECK(plan.off_hdr >= chunks * kBinSlots * 2 && plan.off_bad_slots - plan.off_hdr >= chunks * kBinHdr * 4);
      CHECK(plan.ws_bytes >= plan.off_bad_slots + (uint64_t)plan.bx * a.B * 4);
      CHECK(!plan.clear_ws_bytes && !plan.clear_status_bytes && !plan.clear_out_bytes);
    } else {
      CHECK(a.form != MEMHIP_RASTER_BINNED);
      CHECK(plan.off_bins == 0 && plan.off_tstat % 16 == 0 && plan.off_tstat >= (uint64_t)a.B * 3 * HW * 4);
      CHECK(plan.ws_bytes >= plan.off_tstat + (uint64_t)a.B * 16 && plan.clear_status_bytes == (uint64_t)a.B * 4);
      if (plan.family == MEMHIP_RASTER_LDS) {
        CHECK(g_lds && !a.time_surface && !a.dims && ((uintptr_t)a.out & 3) == 0);
        CHECK(plan.count == 1 && plan.l[0].kernel == MEMHIP_RASTER_K_LDS && plan.l[0].grid_x == plan.bands);
        CHECK(plan.bands >= 1 && plan.bands <= kMaxBands && (long long)plan.rows_per_band * a.W <= kBandPixels);
        CHECK((plan.bands - 1) * plan.rows_per_band < a.H && a.H <= plan.bands * plan.rows_per_band);
        CHECK(plan.l[0].lds == 2 * plan.rows_per_band * a.W * 4 && !plan.clear_ws_bytes && !plan.clear_out_bytes);
      } else {
        CHECK(plan.family == (a.dims ? MEMHIP_RASTER_GLOBAL_VAR : MEMHIP_RASTER_GLOBAL));
        CHECK(plan.count == 2 && plan.l[0].kernel == MEMHIP_RASTER_K_COUNT && plan.l[1].kernel == MEMHIP_RASTER_K_FINALIZE);
        CHECK(plan.clear_ws_bytes == plan.ws_bytes && plan.clear_out_bytes == (a.dims ? (uint64_t)a.B * 3 * HW : 0));
      }
    }
    for (int i = 0; i < plan.count; ++i) {
      const memhip_raster_launch_t& l = plan.l[i];
      CHECK(l.grid_x >= 1 && l.grid_y == a.B && (l.block == 256 || l.block == 512 || l.block == 1024) && l.lds >= 0 && l.lds <= 160 * 1024);
      ++launches;
    }
  }
  CHECK(ok > 100000 && rejected > 30000);
  for (int f = 2; f < 6; ++f) CHECK(family[f] > 5000);
  std::printf("raster_plan_sanitize: %lld plans (binned %lld, lds %lld, global %lld, global_var %lld), %lld launches, %lld rejected\n",
              ok, family[2], family[3], family[4], family[5], launches, rejected);
  return 0;
}
