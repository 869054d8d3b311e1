// Host-only exercise of conv_plan.cpp for the sanitizers: memhip_conv_plan over a few hundred thousand memhip_conv_args_t --
// every mode and unknown ones (and memhip_convt_plan over its plain arguments), accepted and rejected shapes, fields the mode does not have, null in / weight / out (the query
// reads no pointer), every conv_waves value, 8..304 CUs -- with the invariants a launcher relies on checked on the way.  The
// three functions of core.cpp it needs are stubbed here; no device:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/conv_plan_sanitize.cpp mem_amd/csrc/conv_plan.cpp -o conv_plan_sanitize && ./conv_plan_sanitize
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../mem_amd/csrc/common.h"
#include "../mem_amd/csrc/conv_plan.hpp"

static int g_waves = 16;
namespace memhip {
thread_local char g_err[512];
int opt(int id) { return id == OPT_CONV_WAVES ? g_waves : 0; }
int max_cus() { return 256; }
}  // namespace memhip

static unsigned long long g_state = 20261;
static int rnd(int lo, int hi) {   // inclusive
  g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return lo + (int)((g_state >> 33) % (unsigned long long)(hi - lo + 1));
}
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::abort(); } } while (0)

int main() {
  static const int cins[] = {4, 64, 128, 384, 8, 12, 96, 0}, waves[] = {4, 8, 16, 32};
  void* const P = (void*)0x1000;
  long long ok = 0, rejected = 0, launches = 0;
  memhip_conv_plan_t plan;
  CHECK(memhip_conv_plan(nullptr, 256, &plan) == MEMHIP_EINVAL);
  for (int it = 0; it < 300000; ++it) {
    g_waves = waves[it % 4];
    memhip_conv_args_t a = {};
    a.mode = rnd(0, 19) ? rnd(0, 2) : rnd(-1, 3);
    a.B = rnd(0, 29) ? rnd(1, 256) : rnd(-1, 0);
    a.H = rnd(0, 29) ? rnd(7, 224) : rnd(-3, 2);
    a.W = rnd(0, 3) ? a.H : rnd(7, 224);
    a.Cin = cins[rnd(0, 7)];
    a.Cout = rnd(0, 1) ? 128 * rnd(1, 64) : 2 * rnd(0, 512);
    a.ksize = rnd(0, 5); a.stride = rnd(0, 2); a.pad = rnd(-1, 2);
    if (rnd(0, 3)) { const int s = rnd(0, 2); a.ksize = s == 0 ? 4 : s == 1 ? 3 : 1; a.stride = s == 0 ? 2 : 1; a.pad = s == 2 ? 0 : 1; }
    a.relu = rnd(0, 1); a.out_padded = rnd(0, 1);
    a.out_f32 = a.mode == MEMHIP_CONV_F16X2 ? rnd(0, 1) : !rnd(0, 19);
    if (rnd(0, 1)) a.add = P;
    if (a.mode == MEMHIP_CONV_F32 ? rnd(0, 1) : !rnd(0, 19)) a.n_active = (const int32_t*)P;
    if (a.mode == MEMHIP_CONV_F16X2 || !rnd(0, 19)) a.in_plane = a.w_plane = a.out_plane = 1 << 20;
    if (rnd(0, 1)) { a.in = a.weight = P; a.out = P; }
    const int cus = 8 * rnd(1, 38);
    const int rc = memhip_conv_plan(&a, rnd(0, 9) ? cus : -1, &plan);
    CHECK(rc == MEMHIP_OK || rc == MEMHIP_EINVAL);
    if (rc != MEMHIP_OK) { ++rejected; CHECK(memhip::g_err[0]); continue; }
    ++ok;
    CHECK(plan.count >= 0 && plan.count <= 2 && (plan.count == 0) == (plan.M == 0));
    CHECK(plan.count < 2 || (a.mode == MEMHIP_CONV_F32 && a.n_active && plan.l[0].dyn_hi == plan.l[1].dyn_lo));
    for (int i = 0; i < plan.count; ++i) {
      const memhip_conv_launch_t& l = plan.l[i];
      CHECK(l.grid >= 1 && (l.block == 256 || l.block == 512) && l.lds > 0 && l.lds <= 160 * 1024 && l.dyn_lo < l.dyn_hi);
      ++launches;
    }
  }
  CHECK(ok > 30000 && rejected > 30000);
  // memhip_convt_plan (the decoder's transposed convolution): plain arguments, one launch of 4 x tiles workgroups
  long long t_ok = 0, t_rejected = 0;
  CHECK(memhip_convt_plan(2, 3, 5, 64, 72, 256, nullptr) == MEMHIP_EINVAL);
  for (int it = 0; it < 100000; ++it) {
    const int B = rnd(0, 29) ? rnd(1, 256) : rnd(-1, 0), H = rnd(0, 29) ? rnd(1, 224) : rnd(-3, 0);
    const int W = rnd(0, 3) ? H : rnd(1, 4096), Cin = cins[rnd(0, 7)], Cout = rnd(0, 1) ? 128 * rnd(1, 8) : 2 * rnd(0, 512);
    const int rc = memhip_convt_plan(rnd(0, 99) ? B : 1 << 16, H, W, Cin, Cout, rnd(0, 9) ? 8 * rnd(1, 38) : -1, &plan);
    CHECK(rc == MEMHIP_OK || rc == MEMHIP_EINVAL);
    if (rc != MEMHIP_OK) { ++t_rejected; CHECK(memhip::g_err[0]); continue; }
    ++t_ok;
    CHECK(plan.count == (plan.M ? 1 : 0) && plan.K == 4 * Cin && plan.off == 0 && plan.Ho == 2 * H && plan.Wo == 2 * W);
    if (plan.count) {
      const memhip_conv_launch_t& l = plan.l[0];
      const long long tiles = (plan.M + 127) / 128 * ((Cout + 127) / 128);
      CHECK(l.kernel == MEMHIP_CONV_K_BF16_T && l.grid == 4 * tiles && l.grid >= 4 && l.block == 256 && l.lds > 0 && l.lds <= 160 * 1024);
      ++launches;
    }
  }
  CHECK(t_ok > 10000 && t_rejected > 10000);
  ok += t_ok; rejected += t_rejected;
  std::printf("conv_plan_sanitize: %lld plans, %lld launches, %lld rejected\n", ok, launches, rejected);
  return 0;
}
