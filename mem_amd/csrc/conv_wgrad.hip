// dVAE tokenizer training: the weight gradient of every convolution of the model as ONE implicit TN GEMM, and the ReLU
// backward / bias gradient row kernel.  Reference op: autograd's weight gradients of the dVAE's layers
// (eventvae/vae/vae_model.py:29-41 the ResBlock's Conv2d(3,1,1) / Conv2d(1); :86-102 Conv2d(4,2,1), ConvTranspose2d(4,2,1) and
// the two 1x1 heads), which MIOpen computes per layer kind.
//
//   G[n, (ky, kx, c)] (+)= sum_{b,y,x} Small[b, y, x, n] * BigPad[b, s*y + ky + 1 - pad, s*x + kx + 1 - pad, c]
//
// The body is gemm_tn.hip's: both operands are pixel-major, so the tiles are staged row-major ([64 pixels][128 columns], 16 KiB
// each, LDS-DMA, the XOR swizzle applied through the SOURCE address) and the fragments are read down the columns with
// ds_read_b64_tr_b16.  What differs is where a row comes from: as in convt.hip the per-lane DMA source addresses are gathered.
// Row m = (b, y, x) of the Small tile is a pixel of the padded (or dense) Small buffer; the same row of the Big tile is, per
// 16-byte chunk, the tap (ky, kx) of that pixel's patch in the padded Big buffer -- a 128-column tile may span several taps, a
// chunk never does (C % 8 == 0; C == 4: two neighbouring taps of a 4x4 row are contiguous).  wgrad_gather (conv_wgrad_plan.hpp)
// is the one place that computes both offsets.  Rows beyond the slice and chunks beyond N / K come from a zero page: no load
// leaves its buffer, and Big's zero ring supplies the padding taps.
//
// The output is small and the reduction long: the grid is tiles x slices of the pixel range.  No atomics -- with more than one
// slice each workgroup stores its partial tile into the caller's workspace [splits][N][K] and wgrad_fold_kernel adds the slices
// in ascending order, so a call's bits do not depend on scheduling.
#include "common.h"
#include "conv_wgrad_plan.hpp"

namespace {

using namespace memhip;

constexpr int BM = kWgTile, BN = kWgTile, BR = kWgStageRows;
constexpr int kThreads = kWgThreads;
constexpr int kTileBytes = BR * 128 * 2;        // 16 KiB
constexpr int kStageBytes = 2 * kTileBytes;
static_assert(2 * kStageBytes == kWgLdsBytes, "conv_wgrad_plan.hpp: LDS bytes");

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __attribute__((aligned(256))) unsigned char g_wgrad_zero_page[256];   // zero-initialised

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

struct WgradArgs {
  const __bf16* small;
  const __bf16* big;
  float* out;               // grad (one slice) or the workspace (slice sp at out + sp * N * K)
  WgradGeom g;
  int splits, rows_per_split, accumulate;
};

// Stage 64 pixel rows [row0, row0 + 64) of both tiles: 16 wave-instructions of 1 KiB (4 rows) per tile.  LDS chunk position
// cpos (16 B) of row r holds global chunk ((cpos>>1) ^ (r&7))<<1 | (cpos&1) (gemm_tn.hip's image).
__device__ __forceinline__ void stage_rows(const WgradArgs& p, int row0, int rend, int n0, int k0, char* lds, int wave, int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int inst = wave * 4 + j;
    const int r = inst * 4 + (lane >> 4);
    const int cpos = lane & 15;
    const int chunk = (((cpos >> 1) ^ (r & 7)) << 1) | (cpos & 1);
    const int m = row0 + r, n = n0 + chunk * 8, col = k0 + chunk * 8;
    const bool rv = m < rend, nv = n < p.g.N, cv = col < p.g.K;
    const WgradAddr a = wgrad_gather(p.g, rv ? m : 0, nv ? n : 0, cv ? col : 0);
    const void* zero = (const void*)(g_wgrad_zero_page + cpos * 16);
    glds16(rv && nv ? (const void*)(p.small + a.small) : zero, lds + inst * 1024);
    glds16(rv && cv ? (const void*)(p.big + a.big) : zero, lds + kTileBytes + inst * 1024);
  }
}

// gemm_tn.hip's transposed fragment read: 8 bf16 of one column for the k-step `ks` (32 rows): rows 4g+q and 16+4g+q.
__device__ __forceinline__ bf16x8 read_frag_tr(const char* tile, int ks, int col0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int colb = col0 + 4 * p;
  const int seg = colb >> 4, inb = (colb & 15) * 2;
  const int r0 = ks * 32 + 4 * g + q, r1 = r0 + 16;
  const char* a0 = tile + r0 * 256 + ((seg ^ (r0 & 7)) << 5) + inb;
  const char* a1 = tile + r1 * 256 + ((seg ^ (r1 & 7)) << 5) + inb;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a1);
  union { struct { s16x4 l, h; } s; bf16x8 v; } u;
  u.s.l = lo;
  u.s.h = hi;
  return u.v;
}

__global__ __launch_bounds__(kThreads, 2) void conv_wgrad_kernel(WgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int N = p.g.N, K = p.g.K;
  const int ntk = (K + BN - 1) / BN;
  const int tiles = ((N + BM - 1) / BM) * ntk;
  // consecutive workgroups share a slice of the pixels; the slice index is the slow one
  const int tile = blockIdx.x % tiles, sp = blockIdx.x / tiles;
  const int n0 = (tile / ntk) * BM, k0 = (tile % ntk) * BN;
  const int M = (int)p.g.M;
  const int rbeg = sp * p.rows_per_split;           // the plan leaves no slice empty: rbeg < M for every workgroup
  int rend = rbeg + p.rows_per_split;
  rend = rend < M ? rend : M;
  const int nst = (rend - rbeg + BR - 1) / BR;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage_rows(p, rbeg, rend, n0, k0, smem, wave, lane);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < nst; ++t) {
    if (t + 1 < nst) stage_rows(p, rbeg + (t + 1) * BR, rend, n0, k0, smem + (cur ^ 1) * kStageBytes, wave, lane);
    const char* At = smem + cur * kStageBytes;
    const char* Bt = At + kTileBytes;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = read_frag_tr(At, ks, wr * 64 + i * 16, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = read_frag_tr(Bt, ks, wc * 64 + j * 16, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
    cur ^= 1;
  }
  float* out = p.out + (p.splits > 1 ? (long long)sp * N * K : 0);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + wr * 64 + i * 16 + (lane >> 4) * 4 + r;
      if (n >= N) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + wc * 64 + j * 16 + (lane & 15);
        if (k >= K) continue;
        float* o = out + (long long)n * K + k;
        *o = p.accumulate ? *o + acc[i][j][r] : acc[i][j][r];      // one writer per element: plain
      }
    }
}

__global__ __launch_bounds__(256) void wgrad_fold_kernel(const float* __restrict__ ws, int splits, long long NK,
                                                         float* __restrict__ grad, int accumulate) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= NK) return;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += ws[k * NK + i];
  grad[i] = accumulate ? grad[i] + s : s;
}

// ---- ReLU backward in place + bias gradient.  A workgroup covers tpr 16-byte column chunks x (256 / tpr) rows at a time over
// its block of pixels; the row groups are folded through LDS in a fixed order into ONE partial row of the workspace per
// workgroup (plain stores); relu_colsum_fold_kernel adds the partial rows in ascending order.
struct ReluBwdArgs {
  __bf16* g;
  const __bf16* y;
  float* ws;                // [gridDim.y][C] or null
  int padded, H, W, C, R, rows_per_block, tpr;
};

__global__ __launch_bounds__(256) void relu_bwd_colsum_kernel(ReluBwdArgs p) {
  __shared__ float red[256 * 8];
  const int tpr = p.tpr, rp = 256 / tpr;
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr;
  const bool active = ty < rp;
  const int r0 = blockIdx.y * p.rows_per_block;
  const int r1 = min(p.R, r0 + p.rows_per_block);
  const int hw = p.H * p.W;
  for (int cb = blockIdx.x * tpr; cb * 8 < p.C; cb += gridDim.x * tpr) {
    const int c = (cb + tx) * 8;
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (active && c < p.C) {
      for (int r = r0 + ty; r < r1; r += rp) {
        long long row = r;
        if (p.padded) {
          const int b = r / hw, q = r - b * hw;
          const int yy = q / p.W, xx = q - yy * p.W;
          row = ((long long)b * (p.H + 2) + yy + 1) * (p.W + 2) + xx + 1;
        }
        bf16x8 v = *reinterpret_cast<const bf16x8*>(p.g + row * p.C + c);
        if (p.y) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(p.y + row * p.C + c);
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = (float)a[k] > 0.f ? v[k] : (__bf16)0.f;
          *reinterpret_cast<bf16x8*>(p.g + row * p.C + c) = v;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] += (float)v[k];
      }
    }
    if (!p.ws) continue;                                   // uniform
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) red[threadIdx.x * 8 + k] = s[k];
    __syncthreads();
    if (ty == 0 && c < p.C) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float t = 0.f;
        for (int g = 0; g < rp; ++g) t += red[(g * tpr + tx) * 8 + k];
        p.ws[(long long)blockIdx.y * p.C + c + k] = t;
      }
    }
  }
}

__global__ __launch_bounds__(256) void relu_colsum_fold_kernel(const float* __restrict__ ws, int copies, int C,
                                                               float* __restrict__ out, int accumulate) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
#pragma unroll 8
  for (int k = 0; k < copies; ++k) s += ws[(long long)k * C + c];      // ascending order; the loads do not depend on the sum
  out[c] = accumulate ? out[c] + s : s;
}

constexpr int kReluMaxRowBlocks = 1024;   // row blocks of >= 64 pixels: enough workgroups to stream a ViT-B level from HBM

struct ReluGrid { int tpr, gx, gy, rows_per_block; };
ReluGrid relu_grid(long long R, int C) {
  const int chunks = C / 8;
  ReluGrid q;
  q.tpr = chunks >= 256 ? 256 : chunks;
  q.gx = cdiv(chunks, q.tpr);
  long long rows = cdiv(R, kReluMaxRowBlocks);
  if (rows < 64) rows = 64;
  q.rows_per_block = (int)rows;
  q.gy = cdiv(R, rows);
  return q;
}

}  // namespace

extern "C" int memhip_conv_wgrad_plan(const memhip_conv_wgrad_args_t* args, int device_cus, memhip_conv_wgrad_plan_t* out) {
  WgradGeom g;
  if (int rc = wgrad_validate(args, true, &g)) return rc;
  MEMHIP_REQUIRE(out, "conv_wgrad_plan: null pointer");
  *out = wgrad_plan(g, device_cus >= 0 ? device_cus : max_cus());
  return MEMHIP_OK;
}

extern "C" size_t memhip_conv_wgrad_workspace(const memhip_conv_wgrad_args_t* args, int device_cus) {
  WgradGeom g;
  if (wgrad_validate(args, true, &g)) return 0;
  return (size_t)wgrad_plan(g, device_cus >= 0 ? device_cus : max_cus()).ws_bytes;
}

extern "C" int memhip_conv_wgrad_nhwc(const memhip_conv_wgrad_args_t* args, memhip_stream_t stream) {
  WgradGeom g;
  if (int rc = wgrad_validate(args, false, &g)) return rc;
  if (g.M == 0) return MEMHIP_OK;
  const WgradPlan plan = wgrad_plan(g, max_cus());
  if (plan.splits > 1) {
    MEMHIP_REQUIRE(args->workspace && ((uintptr_t)args->workspace & 15) == 0, "conv_wgrad: %d slices need a 16-byte aligned workspace",
                   plan.splits);
    if ((int64_t)args->workspace_bytes < plan.ws_bytes)
      return fail(MEMHIP_EWORKSPACE, "conv_wgrad: workspace %zu < %lld", args->workspace_bytes, (long long)plan.ws_bytes);
  }
  static bool attr_done = false;
  if (!attr_done) {
    MEMHIP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kWgLdsBytes));
    attr_done = true;
  }
  hipStream_t s = as_stream(stream);
  WgradArgs p{(const __bf16*)args->small, (const __bf16*)args->big, plan.splits > 1 ? (float*)args->workspace : args->grad, g,
              plan.splits, plan.rows_per_split, plan.splits > 1 ? 0 : args->accumulate};
  hipLaunchKernelGGL(conv_wgrad_kernel, dim3(plan.grid), dim3(plan.block), plan.lds_bytes, s, p);
  if (int rc = check_launch("conv_wgrad_nhwc")) return rc;
  if (plan.splits > 1) {
    hipLaunchKernelGGL(wgrad_fold_kernel, dim3(plan.fold_grid), dim3(256), 0, s, (const float*)args->workspace, plan.splits,
                       (long long)g.N * g.K, args->grad, args->accumulate);
    return check_launch("conv_wgrad_nhwc (fold)");
  }
  return MEMHIP_OK;
}

extern "C" size_t memhip_relu_bwd_colsum_workspace(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return 0;
  return (size_t)relu_grid((long long)B * H * W, C).gy * C * sizeof(float);
}

extern "C" int memhip_relu_bwd_colsum(void* g, const void* y, int padded, int B, int H, int W, int C, float* colsum, int accumulate,
                                      void* workspace, size_t workspace_bytes, memhip_stream_t stream) {
  MEMHIP_REQUIRE(B >= 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && (long long)B * (H + 2) * (W + 2) <= 1ll << 31,
                 "relu_bwd_colsum: bad shape B=%d H=%d W=%d C=%d (C %% 8 == 0)", B, H, W, C);
  if (B == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(g, "relu_bwd_colsum: null pointer");
  MEMHIP_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)y & 15) == 0, "relu_bwd_colsum: g and y must be 16-byte aligned");
  if (!y && !colsum) return MEMHIP_OK;
  const long long R = (long long)B * H * W;
  const ReluGrid q = relu_grid(R, C);
  const size_t need = (size_t)q.gy * C * sizeof(float);
  if (colsum) {
    MEMHIP_REQUIRE(workspace, "relu_bwd_colsum: the column sums need a workspace");
    if (workspace_bytes < need) return fail(MEMHIP_EWORKSPACE, "relu_bwd_colsum: workspace %zu < %zu", workspace_bytes, need);
  }
  hipStream_t s = as_stream(stream);
  ReluBwdArgs p{(__bf16*)g, (const __bf16*)y, colsum ? (float*)workspace : nullptr, padded ? 1 : 0, H, W, C, (int)R, q.rows_per_block,
                q.tpr};
  hipLaunchKernelGGL(relu_bwd_colsum_kernel, dim3(q.gx, q.gy), dim3(256), 0, s, p);
  if (int rc = check_launch("relu_bwd_colsum")) return rc;
  if (colsum) {
    hipLaunchKernelGGL(relu_colsum_fold_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, (const float*)workspace, q.gy, C, colsum, accumulate);
    return check_launch("relu_bwd_colsum (fold)");
  }
  return MEMHIP_OK;
}
