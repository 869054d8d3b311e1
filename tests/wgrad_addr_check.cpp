// Stand-alone host check of the gather arithmetic of csrc/conv_wgrad.hip (tests/test_conv_wgrad_cpu.py builds and runs it).
// For every shape on the command line ("k,s,pad,B,Hs,Ws,C,N,small_padded") it enumerates every (pixel row, channel chunk of
// small, column chunk of grad) the kernel's LDS-DMA can issue through wgrad_gather and asserts that each 16-byte source
//   - lies inside its buffer and is 16-byte aligned (element offset % 8 == 0),
//   - holds, element by element, what the definition says:
//       small[b, y, x, n + e]  and  big_pad[b, s*y + ky + 1 - pad, s*x + kx + 1 - pad, c]  for column col + e = (ky, kx, c),
//     with (b, y, x) and (ky, kx, c) from nested loops here, not from the divisions under test,
//   - never touches small's ring;
// and that the slices of wgrad_slices cover [0, M) once in whole stages, the stage image is a permutation of a row's 16 chunks
// and the zero-page reads stay inside its 256 bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../mem_amd/csrc/conv_wgrad_plan.hpp"

using namespace memhip;

#define CHECK(cond, ...) \
  do { if (!(cond)) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

struct Tap { int ky, kx, c; };

static int check_shape(const char* spec) {
  memhip_conv_wgrad_args_t a = {};
  int k, s, pad, B, Hs, Ws, C, N, padded;
  CHECK(std::sscanf(spec, "%d,%d,%d,%d,%d,%d,%d,%d,%d", &k, &s, &pad, &B, &Hs, &Ws, &C, &N, &padded) == 9, "%s", spec);
  a.ksize = k; a.stride = s; a.pad = pad; a.B = B; a.Hs = Hs; a.Ws = Ws; a.C = C; a.N = N; a.small_padded = padded;
  const WgradGeom g = wgrad_geom(a);
  const int64_t small_elems = padded ? (int64_t)B * (Hs + 2) * (Ws + 2) * N : (int64_t)B * Hs * Ws * N;
  const int64_t big_elems = (int64_t)B * (s * Hs + 2) * (s * Ws + 2) * C;
  CHECK(g.K == k * k * C && g.M == (int64_t)B * Hs * Ws && g.Hbp == s * Hs + 2 && g.Wbp == s * Ws + 2, "geometry of %s", spec);
  CHECK(g.K % 8 == 0 && N % 8 == 0, "chunks of %s", spec);

  std::vector<Tap> colmap;
  for (int ky = 0; ky < k; ++ky)
    for (int kx = 0; kx < k; ++kx)
      for (int c = 0; c < C; ++c) colmap.push_back({ky, kx, c});
  CHECK((int)colmap.size() == g.K, "K of %s", spec);

  long long issued = 0;
  int m = 0;
  for (int b = 0; b < B; ++b)
    for (int y = 0; y < Hs; ++y)
      for (int x = 0; x < Ws; ++x, ++m) {
        for (int n = 0; n < N; n += 8) {
          const WgradAddr ad = wgrad_gather(g, m, n, 0);
          const int64_t want = padded ? (((int64_t)b * (Hs + 2) + (y + 1)) * (Ws + 2) + (x + 1)) * N + n : (int64_t)m * N + n;
          CHECK(ad.small == want, "%s small m=%d n=%d: %lld != %lld", spec, m, n, (long long)ad.small, (long long)want);
          CHECK(ad.small >= 0 && ad.small + 8 <= small_elems && ad.small % 8 == 0, "%s small m=%d n=%d leaves the buffer", spec, m, n);
          ++issued;
        }
        for (int col = 0; col < g.K; col += 8) {
          const WgradAddr ad = wgrad_gather(g, m, 0, col);
          CHECK(ad.big >= 0 && ad.big + 8 <= big_elems && ad.big % 8 == 0, "%s big m=%d col=%d: %lld leaves the buffer or is unaligned",
                spec, m, col, (long long)ad.big);
          for (int e = 0; e < 8; ++e) {
            const Tap t = colmap[col + e];
            const int py = s * y + t.ky + 1 - pad, px = s * x + t.kx + 1 - pad;
            CHECK(py >= 0 && py < s * Hs + 2 && px >= 0 && px < s * Ws + 2, "%s tap outside the padded image", spec);
            const int64_t want = (((int64_t)b * (s * Hs + 2) + py) * (s * Ws + 2) + px) * C + t.c;
            CHECK(ad.big + e == want, "%s big m=%d col=%d e=%d: %lld != %lld", spec, m, col, e, (long long)(ad.big + e), (long long)want);
          }
          ++issued;
        }
      }
  CHECK(m == g.M, "rows of %s", spec);

  // the slices: whole stages, every row once, none empty -- for every slice count a plan can ask for
  for (int wanted = 1; wanted <= 600; ++wanted) {
    const WgradSlices sl = wgrad_slices(g.M, wanted);
    CHECK(sl.splits >= 1 && sl.splits <= kWgMaxSplits && sl.rows_per_split % kWgStageRows == 0, "%s slices(%d)", spec, wanted);
    CHECK((int64_t)(sl.splits - 1) * sl.rows_per_split < g.M && (int64_t)sl.splits * sl.rows_per_split >= g.M, "%s slices(%d) cover", spec, wanted);
  }
  // the stage image (conv_wgrad.hip stage_rows): per row the 16 LDS positions hold the 16 chunks once; zero page in bounds
  for (int r = 0; r < kWgStageRows; ++r) {
    unsigned seen = 0;
    for (int cpos = 0; cpos < 16; ++cpos) {
      const int chunk = (((cpos >> 1) ^ (r & 7)) << 1) | (cpos & 1);
      CHECK(chunk >= 0 && chunk < 16 && cpos * 16 + 16 <= 256, "stage image");
      seen |= 1u << chunk;
    }
    CHECK(seen == 0xFFFFu, "stage image row %d", r);
  }
  std::printf("ok %s: M=%lld K=%d, %lld chunk addresses\n", spec, (long long)g.M, g.K, issued);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: %s k,s,pad,B,Hs,Ws,C,N,small_padded ...\n", argv[0]);
    return 2;
  }
  for (int i = 1; i < argc; ++i)
    if (check_shape(argv[i])) return 1;
  return 0;
}
