// Host-only exercise of gemm_tn_plan.cpp for the sanitizers: tn_plan and both workspace computations over a few thousand
// shapes (1..4 products, R = 0 / 1 / ragged / 60 000, every workspace state, 0 and 8..256 CUs, all option settings), with
// the invariants a launcher relies on checked on the way.  Links nothing else and needs no device:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/tn_plan_sanitize.cpp mem_amd/csrc/gemm_tn_plan.cpp -o tn_plan_sanitize && ./tn_plan_sanitize
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../mem_amd/csrc/gemm_tn_plan.hpp"

using namespace memhip;

static unsigned long long g_state = 20261;
static int rnd(int lo, int hi) {   // inclusive
  g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return lo + (int)((g_state >> 33) % (unsigned long long)(hi - lo + 1));
}
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::abort(); } } while (0)

static void check_slices(int R, const TnPart& p) {
  CHECK(p.splits >= 1 && p.rows_per_split > 0 && p.tiles >= 1);
  CHECK((long long)p.rows_per_split * p.splits >= R && (long long)p.rows_per_split * (p.splits - 1) < R);   // no empty slice
}

int main() {
  static const int widths[] = {256, 512, 768, 1024, 2304, 3072};
  static const int rows[] = {0, 1, 63, 255, 2047, 2048, 2049, 4099, 50432, 60000};
  long long plans = 0, launches = 0, by_kind[4] = {0, 0, 0, 0};
  for (int it = 0; it < 6000; ++it) {
    const int count = it % 4 + 1;                                     // count 4 every fourth call
    const bool friendly = it / 4 % 2;                                 // every product fits the 256 x 256 kernel
    memhip_tn_problem_t pr[4] = {};
    for (int i = 0; i < count; ++i) {
      pr[i].R = friendly ? rows[rnd(5, 9)] : rnd(0, 3) ? rows[rnd(0, 9)] : rnd(0, 60000);
      pr[i].N = friendly || rnd(0, 1) ? widths[rnd(0, 5)] : 8 * rnd(1, 400);
      pr[i].K = friendly || rnd(0, 1) ? widths[rnd(0, 5)] : 8 * rnd(1, 400);
      pr[i].lda = pr[i].N, pr[i].ldb = pr[i].K;
      pr[i].ldo = pr[i].K + (rnd(0, friendly ? 39 : 9) ? 0 : 2);
      pr[i].A = pr[i].B = (const void*)0x10000;
      pr[i].out = (float*)(uintptr_t)(0x20000 + (rnd(0, friendly ? 39 : 9) ? 0 : 4));
    }
    const int cus = it % 7 == 0 ? 8 : (it % 11 == 0 ? 0 : 8 * rnd(1, 32));
    const size_t one = (size_t)pr[0].N * pr[0].K * 4;
    const size_t bytes[] = {0, one, SIZE_MAX};
    for (int w = 0; w < 3; ++w)
      for (int o = 0; o < 4; ++o) {
        const TnWorkspace ws = {w != 0, rnd(0, 15) != 0, bytes[w]};
        const int accumulate = rnd(0, 1);
        const TnPlan plan = tn_plan(pr, count, accumulate, ws, cus, TnOptions{o & 1, o >> 1});
        ++plans;
        CHECK(plan.count >= 0 && plan.count <= 4);
        int covered = 0;
        for (int li = 0; li < plan.count; ++li) {
          const TnLaunch& l = plan.l[li];
          ++launches;
          CHECK(l.kind >= 0 && l.kind <= 3 && l.count >= 1 && l.count <= 4 && l.grid >= 1);
          CHECK((l.kind == MEMHIP_TN_P8_GROUP) == (l.count > 1));
          ++by_kind[l.kind];
          long long wgs = 0;
          for (int i = 0; i < l.count; ++i) {
            const TnPart& p = l.p[i];
            CHECK(p.problem >= 0 && p.problem < count && pr[p.problem].R > 0);
            check_slices(pr[p.problem].R, p);
            CHECK(p.wg_begin == wgs);
            wgs += (long long)p.tiles * p.splits;
            if (l.ws_bytes)                                           // the product's slabs lie inside the workspace
              CHECK(((size_t)p.ws_offset + (size_t)p.splits * pr[p.problem].N * pr[p.problem].K) * 4 <= (size_t)l.ws_bytes);
            ++covered;
          }
          CHECK(wgs == l.grid);
          CHECK((size_t)l.ws_bytes <= ws.bytes && (l.ws_bytes == 0 || (ws.present && ws.aligned)));
          CHECK((l.reduce_grid > 0) == (l.kind >= MEMHIP_TN_P8_WS) && (l.ws_bytes > 0) == (l.reduce_grid > 0));
          if (l.reduce_grid) CHECK(!l.memset_first && !l.use_atomics);
          if (l.memset_first) CHECK(!accumulate && l.use_atomics);
        }
        int live = 0;
        for (int i = 0; i < count; ++i) live += pr[i].R > 0;
        CHECK(covered == live);
      }
    // the workspace computations: enough for every plan on every CU count a stream of that device can have
    const int dev = it % 5 == 0 ? 8 : 8 * rnd(1, 32);
    const size_t group_need = tn_group_workspace_bytes(pr, count, dev);
    for (int i = 0; i < count; ++i) CHECK(group_need >= tn_workspace_bytes(pr[i].R, pr[i].N, pr[i].K, dev));
    for (int cu = dev; cu >= 8; cu -= 8) {
      const TnPlan plan = tn_plan(pr, count, 0, TnWorkspace{true, true, group_need}, cu, TnOptions{1, 1});
      const TnPlan ample = tn_plan(pr, count, 0, TnWorkspace{true, true, SIZE_MAX}, cu, TnOptions{1, 1});
      CHECK(plan.count == ample.count);
      for (int li = 0; li < plan.count; ++li) CHECK(plan.l[li].kind == ample.l[li].kind && plan.l[li].ws_bytes == ample.l[li].ws_bytes);
    }
    CHECK(tn_workspace_bytes(pr[0].R, pr[0].N, pr[0].K, 0) == 0 && tn_group_workspace_bytes(pr, count, 0) == 0);
  }
  for (int R = 1; R <= 70000; R += R < 600 ? 1 : 97)
    for (int wanted = 0; wanted <= 300; wanted += wanted < 40 ? 1 : 37) {
      const TnSlices a = tn_p8_slices(R, wanted), b = tn_128_slices(R, wanted);
      CHECK(a.rows_per_split % 128 == 0 && b.rows_per_split % 64 == 0);
      CHECK((long long)a.rows_per_split * (a.splits - 1) < R && (long long)a.rows_per_split * a.splits >= R);
      CHECK((long long)b.rows_per_split * (b.splits - 1) < R && (long long)b.rows_per_split * b.splits >= R);
      CHECK(a.splits <= (wanted < 1 ? 1 : wanted) && b.splits <= (wanted < 1 ? 1 : wanted));
    }
  std::printf("tn_plan_sanitize ok: %lld plans, %lld launches (128: %lld, p8 atomic: %lld, p8 workspace: %lld, group: %lld)\n", plans,
              launches, by_kind[0], by_kind[1], by_kind[2], by_kind[3]);
  return 0;
}
