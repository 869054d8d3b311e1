// The dispatch policy of the weight-gradient GEMMs (DESIGN.md section 4 summarises it; tn_plan is the truth).
#include "gemm_tn_plan.hpp"
#include <cstdint>

namespace memhip {
namespace {

int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the reduction passes read and write `out` as float4: the pointer itself must be 16-byte aligned, not only ldo (a
// caller's 4-byte-aligned gradient view takes an atomic form)
bool reducible(const memhip_tn_problem_t& q) { return q.ldo % 4 == 0 && aligned16(q.out); }
int p8_tiles(const memhip_tn_problem_t& q) { return (q.N / kTnP8Tile) * (q.K / kTnP8Tile); }
size_t slab_floats(const memhip_tn_problem_t& q, int splits) { return (size_t)splits * q.N * q.K; }

// Product i on its own (R > 0), as memhip_gemm_bf16_tn runs it.
TnLaunch single(const memhip_tn_problem_t& q, int i, int accumulate, const TnWorkspace& ws, int cus, const TnOptions& o) {
  TnLaunch l = {};
  TnPart& p = l.p[0];
  l.count = 1;
  p.problem = i;
  TnSlices s;
  if (o.tn_p8 && cus > 0 && tn_p8_fits(q.R, q.N, q.K)) {
    p.tiles = p8_tiles(q);
    s = tn_p8_slices(q.R, cus / p.tiles);                   // tiles x slices fill the CUs once
    const size_t need = slab_floats(q, s.splits) * sizeof(float);
    // The workspace form wants something to reduce (splits > 1), room, and 16-byte accesses in the reduction pass.
    // Otherwise fp32 atomics -- and that form clears `out` whenever it overwrites, even with one slice.
    if (ws.present && ws.aligned && s.splits > 1 && ws.bytes >= need && reducible(q)) {
      l.kind = MEMHIP_TN_P8_WS;
      l.reduce_grid = cdiv((long long)q.N * q.K / 4, 256);
      l.ws_bytes = (int64_t)need;
    } else {
      l.kind = MEMHIP_TN_P8_ATOMIC;
      l.memset_first = !accumulate;
      l.use_atomics = 1;
    }
  } else {
    // the 128 x 128 kernel, ~3 workgroups per CU of a 256-CU device.  It clears `out` only in front of several slices;
    // one slice that overwrites uses plain stores.
    l.kind = MEMHIP_TN_128;
    p.tiles = cdiv(q.N, kTn128Tile) * cdiv(q.K, kTn128Tile);
    s = tn_128_slices(q.R, cdiv(768, p.tiles));
    l.memset_first = s.splits > 1 && !accumulate;
    l.use_atomics = s.splits > 1 || accumulate;
  }
  p.splits = s.splits;
  p.rows_per_split = s.rows_per_split;
  l.grid = p.tiles * s.splits;
  return l;
}

// All products as ONE grid with one common slice count, or false.  Every product has to fit the p8 kernel (so R > 0
// everywhere) and its reduction pass.  The common count is that of the first of 1..4 rounds (grids of `cus` workgroups)
// that keeps >= 80 % of the CUs busy, else of the best of the four, and never below 2: there is no grouped atomic form.
// (fc2 + fc1 of ViT-B, 72 tiles: ONE round of 216 workgroups with 3 row slices each -- 55 MB of slabs -- instead of two
// rounds with 7: in the step 34.35-34.39 ms against 34.59-34.83, and against 34.41-34.53 with fc2 / fc1 as single launches;
// the CUs such a round leaves idle take workgroups of the other stream.)
bool group(const memhip_tn_problem_t* pr, int count, int cus, TnLaunch& l) {
  int tiles_total = 0;
  for (int i = 0; i < count; ++i) {
    if (!tn_p8_fits(pr[i].R, pr[i].N, pr[i].K) || !reducible(pr[i])) return false;
    tiles_total += p8_tiles(pr[i]);
  }
  int common = 0;
  double best_eff = 0.0;
  for (int r = 1; r <= 4; ++r) {
    const int sp = (r * cus) / tiles_total;
    if (sp < 2) continue;
    const double eff = (double)tiles_total * sp / ((double)r * cus);
    if (eff > best_eff + 1e-9) { best_eff = eff; common = sp; }
    if (eff >= 0.80) break;
  }
  if (common < 2) return false;
  l = {};
  l.kind = MEMHIP_TN_P8_GROUP;
  l.count = count;
  int quads = 0;
  size_t floats = 0;
  for (int i = 0; i < count; ++i) {          // workgroup ids product after product, (slice, tile) inside a product
    TnPart& p = l.p[i];
    const TnSlices s = tn_p8_slices(pr[i].R, common);
    p.problem = i;
    p.tiles = p8_tiles(pr[i]);
    p.splits = s.splits;
    p.rows_per_split = s.rows_per_split;
    p.wg_begin = l.grid;
    p.quad_begin = quads;
    p.ws_offset = (int64_t)floats;
    l.grid += p.tiles * s.splits;
    quads += (int)(((long long)pr[i].N * pr[i].K / 4 + 255) / 256 * 256);      // whole blocks per product
    floats += slab_floats(pr[i], s.splits);
  }
  l.reduce_grid = quads / 256;
  l.ws_bytes = (int64_t)(floats * sizeof(float));
  return true;
}

const TnWorkspace kAmple = {true, true, SIZE_MAX};
const TnOptions kAllOn = {1, 1};

}  // namespace

TnSlices tn_p8_slices(int R, int wanted) {
  const int pair = 2 * kTnStageRows, pairs = cdiv(R, pair);
  int s = wanted < 1 ? 1 : wanted;
  if (s > pairs / 2) s = pairs / 2 > 0 ? pairs / 2 : 1;
  const int rows = cdiv(pairs, s) * pair;
  return {rows, cdiv(R, rows)};
}

TnSlices tn_128_slices(int R, int wanted) {
  const int stages = cdiv(R, kTnStageRows);
  int s = wanted;
  if (s > stages / 4) s = stages / 4;
  if (s < 1) s = 1;
  const int rows = cdiv(stages, s) * kTnStageRows;
  return {rows, cdiv(R, rows)};
}

TnPlan tn_plan(const memhip_tn_problem_t* pr, int count, int accumulate, const TnWorkspace& ws, int stream_cus,
               const TnOptions& o) {
  TnPlan plan = {};
  if (count > 1 && o.tn_p8 && o.tn_group && ws.present && ws.aligned && stream_cus > 0 &&
      group(pr, count, stream_cus, plan.l[0]) && (size_t)plan.l[0].ws_bytes <= ws.bytes) {
    plan.count = 1;
    return plan;
  }
  // a group that is not one grid: every product as a call of its own, in order.  R == 0: nothing to add, and `out` is
  // not touched even by a call that overwrites.
  for (int i = 0; i < count; ++i)
    if (pr[i].R > 0) plan.l[plan.count++] = single(pr[i], i, accumulate, ws, stream_cus, o);
  return plan;
}

// (the slice count is not monotone in the CU count, so every count a reservation can leave is planned; the caller's
// `out` plays no part for a single product: a view the reduction pass cannot take simply leaves the workspace unused)
size_t tn_workspace_bytes(int R, int N, int K, int device_cus) {
  if (!tn_p8_fits(R, N, K)) return 0;
  memhip_tn_problem_t q = {};
  q.R = R, q.N = N, q.K = K, q.ldo = K;
  size_t need = 0;
  for (int cu = device_cus; cu >= 8; cu -= 8) {
    const size_t b = (size_t)tn_plan(&q, 1, 0, kAmple, cu, kAllOn).l[0].ws_bytes;
    need = b > need ? b : need;
  }
  return need;
}

size_t tn_group_workspace_bytes(const memhip_tn_problem_t* pr, int count, int device_cus) {
  size_t need = 0;
  bool fit = count >= 2 && count <= kTnGroupMax;
  for (int i = 0; i < count; ++i) {                          // enough for the product-by-product plan ...
    const size_t one = tn_workspace_bytes(pr[i].R, pr[i].N, pr[i].K, device_cus);
    need = one > need ? one : need;
    fit = fit && tn_p8_fits(pr[i].R, pr[i].N, pr[i].K);
  }
  for (int cu = device_cus; fit && cu >= 8; cu -= 8) {       // ... and for the one-grid plan
    const TnLaunch l = tn_plan(pr, count, 0, kAmple, cu, kAllOn).l[0];
    if (l.kind == MEMHIP_TN_P8_GROUP && (size_t)l.ws_bytes > need) need = (size_t)l.ws_bytes;
  }
  return need;
}

}  // namespace memhip
