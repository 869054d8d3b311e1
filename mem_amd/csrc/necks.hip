// Feature-pyramid necks of the segmentation backbone (mem/semantic_segmentation/backbone/mem.py:331-346: fpn1 =
// ConvTranspose2d(2, 2) -> SyncBatchNorm -> GELU -> ConvTranspose2d(2, 2), fpn2 = ConvTranspose2d(2, 2)): the data movement
// around the GEMMs and the batch norm + GELU between the two products of fpn1.
//
// A ConvTranspose2d with kernel = stride = 2 has no overlap: out[b, co, 2y+i, 2x+j] = bias[co] + sum_ci in[b, ci, y, x] *
// W[ci, co, i, j], i.e. Y = X W with pixel rows X [R, D] and the weight read as the [D, 4D] matrix it is in memory, column
// 4 co + q, q = 2i + j.  A row of Y ("interleaved", [R, 4D]) holds the four output pixels of one input pixel; the same values
// as plain rows are Z [4R, D], Z[4r + q, co] = Y[r, 4 co + q] ("fine rows" z = 4r + q).  Two levels nest: fine row
// 16 r0 + 4 qa + qb of base pixel r0 = (b, y0, x0) is the pixel (4 y0 + 2 ia + ib, 4 x0 + 2 ja + jb).
//
// Every kernel moves tiles of 64 fine rows x 64 channels through one padded fp32 LDS tile (pitch 65 floats), 256 threads.
// A tile meets global memory on one of three sides, and on each a lane moves 16 bytes (8 at level 1 of the map side) and
// neighbouring lanes neighbouring addresses:
//   Z side  plain bf16 rows [nz, D]:          8 lanes x 16 B = the 128 bytes of a tile row; 32 rows per pass, 2 passes
//   I side  interleaved bf16 rows [R, 4D]:    a lane takes 2 channels x 4 q, 32 lanes the 512 contiguous bytes of one of the
//                                             tile's 16 rows r; 8 rows per pass, 2 passes
//   M side  fp32 maps [B, D, 2^k Hp, 2^k Wp]: k = 2: a tile is 4 base pixels x (4 x 4) outputs, a lane takes the 4 floats of
//           one output row of one base pixel (4 Wp floats per row: always 16-byte aligned), 4 lanes 4 neighbouring base pixels;
//           k = 1: 16 base pixels x (2 x 2), a lane takes 2 floats (8 bytes: a row has 2 Wp floats), 16 lanes 128 bytes;
//           k = 0: 64 pixels of [B, D, P], a lane takes 4 pixels of one channel when P % 4 == 0, single floats otherwise.
// Fine rows past the end (ragged last tile) are neither read nor written; D % 64 == 0, so channel tiles are whole.
// LDS accesses are 4-byte (ds_read_b32 / ds_write_b32, banks of a 32-lane half): the Z side and the I side are at worst
// 2-way conflicted, which a ds_write_b32 absorbs and costs a ds_read_b32 one extra cycle; the kernels are HBM-bound.
//
// The Z side, the k = 0 map side and the two-stage column sums (batch statistics, the two sums of the batch-norm backward: 8 row
// lanes per workgroup here) are bn_tile.hpp's, shared with seg_head.hip.
#include "common.h"
#include "bn_tile.hpp"
#include "gemm_epilogue.hpp"   // gelu_f / gelu_grad_f: the project's exact-erf GELU

namespace {

using namespace memhip;
using namespace memhip::bn;

struct Geom {
  int D, Hp, Wp;
  long long R0;      // base pixels: B * Hp * Wp
};

// ---------------------------------------------------------------- I side: interleaved bf16 rows [R, 4D]
// lane (row rl = t / 32 + 8 h of the tile's 16, channel pair cl = 2 (t % 32)): element e is channel cl + e / 4, q = e % 4,
// fine row 4 rl + q of the tile
__device__ __forceinline__ long long i_offset(long long r, int D, int c) { return r * 4 * D + 4 * c; }

__device__ __forceinline__ void i_load(const bf16_t* __restrict__ y, long long R, int D, long long z0, int c0, float* tile) {
  const int t = threadIdx.x, cl = 2 * (t & 31);
  us8 v[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const long long r = z0 / 4 + (t >> 5) + 8 * h;
    v[h] = 0;
    if (r < R) v[h] = *reinterpret_cast<const us8*>(y + i_offset(r, D, c0 + cl));
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int rl = (t >> 5) + 8 * h;
#pragma unroll
    for (int e = 0; e < 8; ++e) tile[(4 * rl + (e & 3)) * kPitch + cl + (e >> 2)] = bf2f(v[h][e]);
  }
}

__device__ __forceinline__ void i_store(bf16_t* __restrict__ y, long long R, int D, long long z0, int c0, const float* tile) {
  const int t = threadIdx.x, cl = 2 * (t & 31);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int rl = (t >> 5) + 8 * h;
    const long long r = z0 / 4 + rl;
    us8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = f2bf(tile[(4 * rl + (e & 3)) * kPitch + cl + (e >> 2)]);
    if (r < R) *reinterpret_cast<us8*>(y + i_offset(r, D, c0 + cl)) = v;
  }
}

// ---------------------------------------------------------------- M side: fp32 maps [B, D, 2^K Hp, 2^K Wp]
// LOAD: map -> tile, else tile -> map.  The fine rows of the tile are z0 .. z0 + 63 of R0 * 4^K.
template <int K, bool VEC, bool LOAD>
__device__ __forceinline__ void map_side(float* __restrict__ map, const Geom& g, long long z0, int c0, float* tile) {
  const int t = threadIdx.x;
  const int P = g.Hp * g.Wp;
  if constexpr (K == 2) {
    const int rl = t & 3, dy = (t >> 2) & 3;
    const long long r = z0 / 16 + rl;
    const bool ok = r < g.R0;
    const long long b = r / P;
    const int p = (int)(r % P), y0 = p / g.Wp, x0 = p % g.Wp;
    const int zb = 16 * rl + 8 * (dy >> 1) + 2 * (dy & 1);           // element e (= dx): fine row zb + 4 (e / 2) + e % 2
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int cl = (t >> 4) + 16 * h;
      float* ptr = map + ((b * g.D + c0 + cl) * (4 * g.Hp) + 4 * y0 + dy) * (4LL * g.Wp) + 4 * x0;
      if (LOAD) {
        f4 v = 0.f;
        if (ok) v = *reinterpret_cast<const f4*>(ptr);
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[(zb + 4 * (e >> 1) + (e & 1)) * kPitch + cl] = v[e];
      } else {
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tile[(zb + 4 * (e >> 1) + (e & 1)) * kPitch + cl];
        if (ok) *reinterpret_cast<f4*>(ptr) = v;
      }
    }
  } else if constexpr (K == 1) {
    const int rl = t & 15, i = (t >> 4) & 1;
    const long long r = z0 / 4 + rl;
    const bool ok = r < g.R0;
    const long long b = r / P;
    const int p = (int)(r % P), y0 = p / g.Wp, x0 = p % g.Wp;
    const int zb = 4 * rl + 2 * i;                                   // element e (= j): fine row zb + e
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const int cl = (t >> 5) + 8 * h;
      float* ptr = map + ((b * g.D + c0 + cl) * (2 * g.Hp) + 2 * y0 + i) * (2LL * g.Wp) + 2 * x0;
      if (LOAD) {
        f2 v = 0.f;
        if (ok) v = *reinterpret_cast<const f2*>(ptr);
        tile[zb * kPitch + cl] = v[0];
        tile[(zb + 1) * kPitch + cl] = v[1];
      } else {
        f2 v;
        v[0] = tile[zb * kPitch + cl];
        v[1] = tile[(zb + 1) * kPitch + cl];
        if (ok) *reinterpret_cast<f2*>(ptr) = v;
      }
    }
  } else {
    bn::map_side<VEC, LOAD>(map, g.D, P, g.R0, z0, c0, tile);      // the map itself: 64 pixels of [B, D, P]
  }
}

// fp32 map of level K -> bf16 rows: plain [R0, D] (K = 0), interleaved [R0 * 4^(K-1), 4D] (K = 1, 2)
template <int K, bool VEC>
__global__ __launch_bounds__(kT) void maps_to_rows_kernel(const float* __restrict__ map, Geom g, bf16_t* __restrict__ rows) {
  __shared__ float tile[kTile * kPitch];
  const long long z0 = (long long)blockIdx.x * kTile;
  const int c0 = blockIdx.y * kTile;
  const long long nz = g.R0 << (2 * K);
  map_side<K, VEC, true>(const_cast<float*>(map), g, z0, c0, tile);
  __syncthreads();
  if constexpr (K == 0) row_side<false>(rows, nz, PlainRows{g.D}, z0, c0, tile);
  else i_store(rows, nz / 4, g.D, z0, c0, tile);
}

template <int K, bool VEC>
__global__ __launch_bounds__(kT) void rows_to_maps_kernel(const bf16_t* __restrict__ rows, Geom g, float* __restrict__ map) {
  __shared__ float tile[kTile * kPitch];
  const long long z0 = (long long)blockIdx.x * kTile;
  const int c0 = blockIdx.y * kTile;
  const long long nz = g.R0 << (2 * K);
  if constexpr (K == 0) row_side<true>(rows, nz, PlainRows{g.D}, z0, c0, tile);
  else i_load(rows, nz / 4, g.D, z0, c0, tile);
  __syncthreads();
  map_side<K, VEC, false>(map, g, z0, c0, tile);
}

// ---------------------------------------------------------------- column sums (bn_tile.hpp: 8 row lanes x 2 channels per thread)
// per channel over y [R, 4D] interleaved: sum (x - s), sum (x - s)^2
__global__ __launch_bounds__(kT) void colstats_kernel(const bf16_t* __restrict__ y, long long R, int D,
                                                      const float* __restrict__ shift, float* __restrict__ ws) {
  __shared__ float red[2 * 8 * 64];
  const int t = threadIdx.x, c0 = blockIdx.y * kTile, cl = 2 * (t & 31);
  const float s[2] = {shift[c0 + cl], shift[c0 + cl + 1]};
  float a1[2] = {0.f, 0.f}, a2[2] = {0.f, 0.f};
#pragma unroll 4
  for (long long r = (long long)blockIdx.x * 8 + (t >> 5); r < R; r += 8LL * gridDim.x) {
    const us8 v = *reinterpret_cast<const us8*>(y + i_offset(r, D, c0 + cl));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = bf2f(v[e]) - s[e >> 2];
      a1[e >> 2] += d;
      a2[e >> 2] = fmaf(d, d, a2[e >> 2]);
    }
  }
  fold_rows_and_store<8, 2>(a1, a2, red, ws + (long long)blockIdx.x * 2 * D, D, c0);
}

// ---------------------------------------------------------------- batch norm + GELU
struct BnChan { float m[2], rs[2], ga[2], be[2]; };
__device__ __forceinline__ BnChan bn_chan(const BnParams& p, int c) {
  BnChan k;
#pragma unroll
  for (int i = 0; i < 2; ++i) { k.m[i] = p.mean[c + i]; k.rs[i] = p.rstd[c + i]; k.ga[i] = p.gamma[c + i]; k.be[i] = p.beta[c + i]; }
  return k;
}

// z [4R, D] = bf16(gelu(gamma * (y - mean) * rstd + beta)), y [R, 4D] interleaved
__global__ __launch_bounds__(kT) void bn_gelu_fwd_kernel(const bf16_t* __restrict__ y, long long R, int D, BnParams p,
                                                         bf16_t* __restrict__ z) {
  __shared__ float tile[kTile * kPitch];
  const int t = threadIdx.x, c0 = blockIdx.y * kTile, cl = 2 * (t & 31);
  const long long z0 = (long long)blockIdx.x * kTile;
  const BnChan k = bn_chan(p, c0 + cl);
  us8 v[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const long long r = z0 / 4 + (t >> 5) + 8 * h;
    v[h] = 0;
    if (r < R) v[h] = *reinterpret_cast<const us8*>(y + i_offset(r, D, c0 + cl));
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int rl = (t >> 5) + 8 * h;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = e >> 2;
      const float u = fmaf((bf2f(v[h][e]) - k.m[c]) * k.rs[c], k.ga[c], k.be[c]);
      tile[(4 * rl + (e & 3)) * kPitch + cl + c] = gelu_f(u);
    }
  }
  __syncthreads();
  row_side<false>(z, 4 * R, PlainRows{D}, z0, c0, tile);
}

// stage 1 of the backward sums: g = da * gelu'(u), per channel sum g and sum g * xhat; workgroup blockIdx.x takes the tiles
// blockIdx.x, blockIdx.x + G, ... of cdiv(4R, 64)
__global__ __launch_bounds__(kT) void bn_gelu_bwd_sums_kernel(const bf16_t* __restrict__ da, const bf16_t* __restrict__ y,
                                                              long long R, int D, BnParams p, float* __restrict__ ws) {
  __shared__ float tile[kTile * kPitch];
  const int t = threadIdx.x, c0 = blockIdx.y * kTile, cl = 2 * (t & 31);
  const BnChan k = bn_chan(p, c0 + cl);
  const long long tiles = (4 * R + kTile - 1) / kTile;
  float a1[2] = {0.f, 0.f}, a2[2] = {0.f, 0.f};
  for (long long ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const long long z0 = ti * kTile;
    __syncthreads();                                   // the previous tile's readers are done
    row_side<true>(da, 4 * R, PlainRows{D}, z0, c0, tile);   // zero past the end: those rows add nothing
    us8 v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long r = z0 / 4 + (t >> 5) + 8 * h;
      v[h] = 0;
      if (r < R) v[h] = *reinterpret_cast<const us8*>(y + i_offset(r, D, c0 + cl));
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int rl = (t >> 5) + 8 * h;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = e >> 2;
        const float xh = (bf2f(v[h][e]) - k.m[c]) * k.rs[c];
        const float g = tile[(4 * rl + (e & 3)) * kPitch + cl + c] * gelu_grad_f(fmaf(xh, k.ga[c], k.be[c]));
        a1[c] += g;
        a2[c] = fmaf(g, xh, a2[c]);
      }
    }
  }
  __syncthreads();
  fold_rows_and_store<8, 2>(a1, a2, tile, ws + (long long)blockIdx.x * 2 * D, D, c0);
}

// dy [R, 4D] interleaved = bf16(gamma * rstd * (g - sum_g / N - xhat * sum_gx / N))
__global__ __launch_bounds__(kT) void bn_gelu_bwd_apply_kernel(const bf16_t* __restrict__ da, const bf16_t* __restrict__ y,
                                                               long long R, int D, BnParams p, const float* __restrict__ sums,
                                                               float inv_n, bf16_t* __restrict__ dy) {
  __shared__ float tile[kTile * kPitch];
  const int t = threadIdx.x, c0 = blockIdx.y * kTile, cl = 2 * (t & 31);
  const long long z0 = (long long)blockIdx.x * kTile;
  const BnChan k = bn_chan(p, c0 + cl);
  const float m1[2] = {sums[c0 + cl] * inv_n, sums[c0 + cl + 1] * inv_n};
  const float m2[2] = {sums[D + c0 + cl] * inv_n, sums[D + c0 + cl + 1] * inv_n};
  row_side<true>(da, 4 * R, PlainRows{D}, z0, c0, tile);
  us8 v[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const long long r = z0 / 4 + (t >> 5) + 8 * h;
    v[h] = 0;
    if (r < R) v[h] = *reinterpret_cast<const us8*>(y + i_offset(r, D, c0 + cl));
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int rl = (t >> 5) + 8 * h;
    const long long r = z0 / 4 + rl;
    us8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = e >> 2;
      const float xh = (bf2f(v[h][e]) - k.m[c]) * k.rs[c];
      const float g = tile[(4 * rl + (e & 3)) * kPitch + cl + c] * gelu_grad_f(fmaf(xh, k.ga[c], k.be[c]));
      o[e] = f2bf(k.ga[c] * k.rs[c] * (g - m1[c] - xh * m2[c]));
    }
    if (r < R) *reinterpret_cast<us8*>(dy + i_offset(r, D, c0 + cl)) = o;
  }
}

// ---------------------------------------------------------------- host side
int check_geom(const char* what, int B, int D, int Hp, int Wp, int level, Geom& g) {
  MEMHIP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && D > 0 && D % kTile == 0 && D / kTile <= 65535,
                 "%s: bad shape B=%d D=%d Hp=%d Wp=%d (all positive, D a multiple of 64)", what, B, D, Hp, Wp);
  MEMHIP_REQUIRE(level >= 0 && level <= 2, "%s: bad level %d (0: the map itself, 1 / 2: upsampled once / twice)", what, level);
  const long long R0 = (long long)B * Hp * Wp;
  MEMHIP_REQUIRE((long long)Hp * Wp <= (1 << 24) && (R0 << (2 * level)) <= (1LL << 36),
                 "%s: bad shape, too many pixels (B=%d Hp=%d Wp=%d level=%d)", what, B, Hp, Wp, level);
  g = Geom{D, Hp, Wp, R0};
  return MEMHIP_OK;
}

int check_rows(const char* what, long long R, int D) {
  MEMHIP_REQUIRE(R > 0 && R <= (1LL << 34) && D > 0 && D % kTile == 0 && D / kTile <= 65535,
                 "%s: bad shape R=%lld D=%d (R positive, D a positive multiple of 64)", what, R, D);
  return MEMHIP_OK;
}

int groups_of(long long units) { return (int)(units < kGroups ? units : kGroups); }

}  // namespace

extern "C" int memhip_neck_maps_to_rows(const float* map, int B, int D, int Hp, int Wp, int level, void* rows,
                                        memhip_stream_t stream) {
  Geom g;
  if (int rc = check_geom("neck_maps_to_rows", B, D, Hp, Wp, level, g)) return rc;
  MEMHIP_REQUIRE(map && rows, "neck_maps_to_rows: null pointer");
  MEMHIP_REQUIRE(aligned(rows, 16), "neck_maps_to_rows: rows is not 16-byte aligned");
  MEMHIP_REQUIRE(aligned(map, level == 2 ? 16 : level == 1 ? 8 : 4), "neck_maps_to_rows: map is not aligned for level %d", level);
  const dim3 grid(cdiv(g.R0 << (2 * level), kTile), D / kTile);
  bf16_t* out = static_cast<bf16_t*>(rows);
  if (level == 2)
    hipLaunchKernelGGL((maps_to_rows_kernel<2, true>), grid, dim3(kT), 0, as_stream(stream), map, g, out);
  else if (level == 1)
    hipLaunchKernelGGL((maps_to_rows_kernel<1, true>), grid, dim3(kT), 0, as_stream(stream), map, g, out);
  else if ((Hp * Wp) % 4 == 0 && aligned(map, 16))
    hipLaunchKernelGGL((maps_to_rows_kernel<0, true>), grid, dim3(kT), 0, as_stream(stream), map, g, out);
  else
    hipLaunchKernelGGL((maps_to_rows_kernel<0, false>), grid, dim3(kT), 0, as_stream(stream), map, g, out);
  return check_launch("neck_maps_to_rows");
}

extern "C" int memhip_neck_rows_to_maps(const void* rows, int B, int D, int Hp, int Wp, int level, float* map,
                                        memhip_stream_t stream) {
  Geom g;
  if (int rc = check_geom("neck_rows_to_maps", B, D, Hp, Wp, level, g)) return rc;
  MEMHIP_REQUIRE(map && rows, "neck_rows_to_maps: null pointer");
  MEMHIP_REQUIRE(aligned(rows, 16), "neck_rows_to_maps: rows is not 16-byte aligned");
  MEMHIP_REQUIRE(aligned(map, level == 2 ? 16 : level == 1 ? 8 : 4), "neck_rows_to_maps: map is not aligned for level %d", level);
  const dim3 grid(cdiv(g.R0 << (2 * level), kTile), D / kTile);
  const bf16_t* in = static_cast<const bf16_t*>(rows);
  if (level == 2)
    hipLaunchKernelGGL((rows_to_maps_kernel<2, true>), grid, dim3(kT), 0, as_stream(stream), in, g, map);
  else if (level == 1)
    hipLaunchKernelGGL((rows_to_maps_kernel<1, true>), grid, dim3(kT), 0, as_stream(stream), in, g, map);
  else if ((Hp * Wp) % 4 == 0 && aligned(map, 16))
    hipLaunchKernelGGL((rows_to_maps_kernel<0, true>), grid, dim3(kT), 0, as_stream(stream), in, g, map);
  else
    hipLaunchKernelGGL((rows_to_maps_kernel<0, false>), grid, dim3(kT), 0, as_stream(stream), in, g, map);
  return check_launch("neck_rows_to_maps");
}

extern "C" size_t memhip_neck_sums_workspace(int D) { return D > 0 ? (size_t)kGroups * 2 * D * sizeof(float) : 0; }

extern "C" int memhip_neck_colstats(const void* y, int64_t R, int D, const float* shift, float* workspace,
                                    size_t workspace_bytes, float* out, memhip_stream_t stream) {
  if (int rc = check_rows("neck_colstats", R, D)) return rc;
  MEMHIP_REQUIRE(y && shift && workspace && out, "neck_colstats: null pointer");
  MEMHIP_REQUIRE(aligned(y, 16), "neck_colstats: y is not 16-byte aligned");
  MEMHIP_REQUIRE(workspace_bytes >= memhip_neck_sums_workspace(D), "neck_colstats: workspace of %zu bytes, %zu needed",
                 workspace_bytes, memhip_neck_sums_workspace(D));
  const int G = groups_of((R + 7) / 8);
  hipLaunchKernelGGL(colstats_kernel, dim3(G, D / kTile), dim3(kT), 0, as_stream(stream), static_cast<const bf16_t*>(y),
                     (long long)R, D, shift, workspace);
  launch_fold(workspace, G, 2 * D, fold_grid(2 * D), FoldOut{{out + D, nullptr, nullptr}, {2 * D, 0, 0}, out, D, (float)(4 * R)},
              as_stream(stream));
  return check_launch("neck_colstats");
}

extern "C" int memhip_neck_bn_gelu_fwd(const void* y, int64_t R, int D, const float* mean, const float* rstd,
                                       const float* gamma, const float* beta, void* z, memhip_stream_t stream) {
  if (int rc = check_rows("neck_bn_gelu_fwd", R, D)) return rc;
  if (int rc = check_bn("neck_bn_gelu_fwd", mean, rstd, gamma, beta)) return rc;
  MEMHIP_REQUIRE(y && z, "neck_bn_gelu_fwd: null pointer");
  MEMHIP_REQUIRE(aligned(y, 16) && aligned(z, 16), "neck_bn_gelu_fwd: y or z is not 16-byte aligned");
  hipLaunchKernelGGL(bn_gelu_fwd_kernel, dim3(cdiv(4 * R, kTile), D / kTile), dim3(kT), 0, as_stream(stream),
                     static_cast<const bf16_t*>(y), (long long)R, D, BnParams{mean, rstd, gamma, beta}, static_cast<bf16_t*>(z));
  return check_launch("neck_bn_gelu_fwd");
}

extern "C" int memhip_neck_bn_gelu_bwd_sums(const void* da, const void* y, int64_t R, int D, const float* mean,
                                            const float* rstd, const float* gamma, const float* beta, float* workspace,
                                            size_t workspace_bytes, float* out, memhip_stream_t stream) {
  if (int rc = check_rows("neck_bn_gelu_bwd_sums", R, D)) return rc;
  if (int rc = check_bn("neck_bn_gelu_bwd_sums", mean, rstd, gamma, beta)) return rc;
  MEMHIP_REQUIRE(da && y && workspace && out, "neck_bn_gelu_bwd_sums: null pointer");
  MEMHIP_REQUIRE(aligned(da, 16) && aligned(y, 16), "neck_bn_gelu_bwd_sums: da or y is not 16-byte aligned");
  MEMHIP_REQUIRE(workspace_bytes >= memhip_neck_sums_workspace(D), "neck_bn_gelu_bwd_sums: workspace of %zu bytes, %zu needed",
                 workspace_bytes, memhip_neck_sums_workspace(D));
  const int G = groups_of((4 * R + kTile - 1) / kTile);
  hipLaunchKernelGGL(bn_gelu_bwd_sums_kernel, dim3(G, D / kTile), dim3(kT), 0, as_stream(stream),
                     static_cast<const bf16_t*>(da), static_cast<const bf16_t*>(y), (long long)R, D,
                     BnParams{mean, rstd, gamma, beta}, workspace);
  launch_fold(workspace, G, 2 * D, fold_grid(2 * D), FoldOut{{out, nullptr, nullptr}, {2 * D, 0, 0}, nullptr, 0, 0.f}, as_stream(stream));
  return check_launch("neck_bn_gelu_bwd_sums");
}

extern "C" int memhip_neck_bn_gelu_bwd_apply(const void* da, const void* y, int64_t R, int D, const float* mean,
                                             const float* rstd, const float* gamma, const float* beta, const float* sums,
                                             float inv_n, void* dy, memhip_stream_t stream) {
  if (int rc = check_rows("neck_bn_gelu_bwd_apply", R, D)) return rc;
  if (int rc = check_bn("neck_bn_gelu_bwd_apply", mean, rstd, gamma, beta)) return rc;
  MEMHIP_REQUIRE(da && y && sums && dy, "neck_bn_gelu_bwd_apply: null pointer");
  MEMHIP_REQUIRE(aligned(da, 16) && aligned(y, 16) && aligned(dy, 16), "neck_bn_gelu_bwd_apply: da, y or dy is not 16-byte aligned");
  MEMHIP_REQUIRE(inv_n > 0.f, "neck_bn_gelu_bwd_apply: inv_n=%g must be positive (1 / elements per channel)", (double)inv_n);
  hipLaunchKernelGGL(bn_gelu_bwd_apply_kernel, dim3(cdiv(4 * R, kTile), D / kTile), dim3(kT), 0, as_stream(stream),
                     static_cast<const bf16_t*>(da), static_cast<const bf16_t*>(y), (long long)R, D,
                     BnParams{mean, rstd, gamma, beta}, sums, inv_n, static_cast<bf16_t*>(dy));
  return check_launch("neck_bn_gelu_bwd_apply");
}
