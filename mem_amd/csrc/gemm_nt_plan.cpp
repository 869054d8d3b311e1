// The dispatch policy of memhip_gemm_bf16_nt (DESIGN.md section 4 summarises it; this function is the truth).
#include "gemm_nt_plan.hpp"

namespace memhip {
namespace {

constexpr int kMinRows = 4096;     // below this the persistent forms do not pay: the 128x128 kernel takes the product

int cdiv(int a, int b) { return (a + b - 1) / b; }

// rows [row0, row0 + rows) on the persistent form `kind` (256 columns per tile; tile height 128 for P8_128), `cus` CUs
NtLaunch persistent(int kind, const GemmArgs& p, int row0, int rows, int cus) {
  NtLaunch l = {};
  l.kind = kind;
  l.row0 = row0;
  l.rows = rows;
  const int tiles = cdiv(rows, kind == MEMHIP_NT_P8_128 ? 128 : 256) * (p.N / 256);
  l.grid = tiles < cus ? tiles : cus;
  l.guard = kind == MEMHIP_NT_P8_128 && rows % 128 != 0;
  l.copy = kind != MEMHIP_NT_G256 && nt_p8_copy(p);
  return l;
}

NtLaunch nt128(const GemmArgs& p, int row0, int rows) {
  NtLaunch l = {};
  l.kind = MEMHIP_NT_128;
  l.row0 = row0;
  l.rows = rows;
  l.grid = cdiv(rows, 128) * cdiv(p.N, 128);
  return l;
}

NtPlan one(const NtLaunch& a) { return NtPlan{1, {a, {}}}; }
NtPlan two(const NtLaunch& a, const NtLaunch& b) { return NtPlan{2, {a, b}}; }

}  // namespace

NtPlan gemm_nt_plan(const GemmArgs& p, int stream_cus, int device_cus, const NtOptions& o) {
  const int M = p.M, epi = p.epilogue, ntn = p.N / 256;
  // every leading dimension the vector epilogues touch is a multiple of 8 elements (host twin of vec_ok, gemm_epilogue.hpp)
  const bool vec = ((p.ldo0 | p.ldo1 | p.ldr | p.ldaux | p.colscale_n) & 7) == 0;
  const bool copy = nt_p8_copy(p);

  // ---- the phase-interleaved persistent kernel (gemm_p8.hip) on `rows` rows that start m_base rows into the product.
  // Narrow outputs (N = 768) are taken too: the rows of a poorly filled last round go to finer tiles (below).
  //  * the residual epilogue of the 256-row kernel finds a row's sample without an integer division: rows below 2^21;
  //  * a 256-row tile touches at most four samples of a sample map: rows_per_sample >= 86.
  auto p8_fits = [&](int rows, int m_base) {
    const bool rows_ok = (!(p.rowmask || p.sample_map) || (long long)rows + m_base < (1 << 21)) &&
                         (!p.sample_map || p.rows_per_sample >= 86);
    return rows >= kMinRows && p.N >= o.gemm_p8_min_n && p.N % 256 == 0 && p.K % 128 == 0 && vec && rows_ok;
  };
  // (PATCH_EMBED has no p8 form at all, so it is never split either)
  if (o.gemm_p8 && stream_cus > 0 && nt_p8_has(epi, 128, false, copy) && p8_fits(M, p.m_base)) {
    // epilogues without a 256-row instantiation run the 128-row form on whole 256-row tiles as well
    const int big = nt_p8_has(epi, 256, false, copy) ? MEMHIP_NT_P8_256 : MEMHIP_NT_P8_128;
    // Rows for the 256-row tiles (0 = everything).  They take whole tiles only (no row guard in their epilogue), and when
    // the last round of tiles would be less than half full (N = 768: 591 tiles on 256 CUs) the full rounds only.
    int head = 0;
    if (o.gemm_split) {
      const int tiles = cdiv(M, 256) * ntn, rounds = tiles / stream_cus, rem = tiles % stream_cus;
      const int whole = M / 256 * 256;
      if (rounds < 1 || rem == 0 || rem * 2 > stream_cus) head = whole == M ? 0 : whole;
      else head = (rounds * stream_cus / ntn) * 256;
    }
    if (head > 0 && head < M) {
      const int tail = M - head;
      if (p8_fits(head, p.m_base)) {     // (a head that does not fit sends the WHOLE product on to the forms below)
        // one launch for both row ranges where the epilogue has a paired form: the kernel gives every XCD a contiguous
        // run of tiles per round, which needs a multiple of 8 workgroups
        if (o.gemm_p8_half && o.gemm_p8_pair && nt_pair_has(epi, copy) && tail >= 128 && stream_cus % 8 == 0) {
          NtLaunch l = persistent(MEMHIP_NT_P8_PAIR, p, 0, head, stream_cus);
          const NtLaunch t = persistent(MEMHIP_NT_P8_128, p, head, tail, stream_cus);
          l.tail_rows = tail;
          l.guard = t.guard;
          l.tail_grid = t.grid;
          return one(l);
        }
        // the left-over rows: the same phase structure on 128-row tiles, or the 128x128 kernel (2-3 workgroups per CU)
        return two(persistent(big, p, 0, head, stream_cus), o.gemm_p8_half && tail >= 128
                                                                ? persistent(MEMHIP_NT_P8_128, p, head, tail, stream_cus)
                                                                : nt128(p, head, tail));
      }
    } else if (M % 256 == 0) {
      return one(persistent(big, p, 0, M, stream_cus));
    }
  }
  // ---- the lockstep 256x256 kernel (gemm256.hip) takes wide products that the p8 forms do not (K a multiple of 64 but not
  // of 128, or gemm_p8 = 0).  N = 768 (3 tiles wide) leaves the third round of 591 tiles 31 % full on 256 CUs and measures
  // 5-10 % below the 128x128 kernel; wide N gains 12-25 % (gemm256_min_n).  K advances 32 at a time.
  if (o.gemm256 && device_cus > 0 && nt_g256_has(epi) && M >= kMinRows && p.N >= o.gemm256_min_n && p.N % 256 == 0 &&
      p.K % 32 == 0 && vec)
    return one(persistent(MEMHIP_NT_G256, p, 0, M, device_cus));
  return one(nt128(p, 0, M));
}

}  // namespace memhip
