// bf16 MFMA GEMM for the ViT contractions:  C[M,N] = A[M,K] * B[N,K]^T  (both operands
// K-contiguous, fp32 accumulate), with the reference's elementwise neighbours fused into the
// epilogue (bias, exact-erf GELU, layer-scale + stochastic-depth + residual, GELU', mask-token
// blend, fp32 gradient accumulation).  Reference ops: F.linear / nn.Linear / nn.Conv2d(k=s=16)
// in mem/modeling_finetune.py:61-70,132-155,203-209 and mem/modeling_pretrain.py:59,101-108.
//
// CDNA4 mapping: 128x128x64 macro-tile, 256 threads = 4 waves (2x2), each wave a 64x64
// sub-tile of 4x4 v_mfma_f32_16x16x32_bf16 fragments.  Operand tiles go HBM -> LDS with
// global_load_lds_dwordx4 (no VGPR round trip), double-buffered; the LDS image is XOR-swizzled
// through the *source* address (LDS-DMA writes lane-linear) so that every ds_read_b128 fragment
// read is bank-conflict free.  Workgroup ids are remapped so that the 8 XCDs each walk a
// contiguous range of tiles (A row-panel reuse in the XCD-private L2).
#include <cstddef>
#include "common.h"
#include "gemm_epilogue.hpp"

namespace {

using namespace memhip;

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kThreads = 256;
constexpr int kTileBytes = BM * BK * 2;       // 16 KiB per operand tile
constexpr int kStageBytes = 2 * kTileBytes;   // A + B

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// 16-byte slot index of (row, 16B-chunk) inside a [128][64] bf16 tile (128-B rows).
__device__ __forceinline__ int swz_slot(int row, int chunk) { return row * 8 + (chunk ^ ((row >> 1) & 7)); }

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// Stage one [128][64] bf16 operand tile: 16 wave-instructions of 1 KiB (8 rows) each, 4 per wave.
// `src` points at (row0, k0) of a row-major [rows, ld] matrix; rows are clamped to `rows_valid-1`
// (out-of-range rows only feed outputs that the epilogue masks).
__device__ __forceinline__ void stage_tile(const __bf16* __restrict__ src, long long ld, int row0,
                                           int rows_valid, int k0, char* lds_tile, int wave, int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int inst = wave * 4 + j;
    const int row = inst * 8 + (lane >> 3);
    const int cpos = lane & 7;                       // chunk position in LDS
    const int chunk = cpos ^ ((row >> 1) & 7);       // global chunk that must land there
    int grow = row0 + row;
    grow = grow < rows_valid ? grow : rows_valid - 1;
    const __bf16* g = src + (long long)grow * ld + k0 + chunk * 8;
    glds16(g, lds_tile + inst * 1024);               // LDS dest = wave-uniform base + lane*16
  }
}

template <int EPI>
__global__ __launch_bounds__(kThreads, 2) void gemm_nt_kernel(typename EpiArgs<EPI>::type p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 1, wc = wave & 1;

  // XCD-aware, bijective remap of the linear block id (cdna guide T1)
  const int nwg = gridDim.x;
  int pid = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = pid & 7, idx = pid >> 3;
    pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int ntn = (p.N + BN - 1) / BN;
  const int tile_m = pid / ntn, tile_n = pid % ntn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / BK;
  stage_tile(p.A, p.lda, m0, p.M, 0, smem, wave, lane);
  stage_tile(p.B, p.ldb, n0, p.N, 0, smem + kTileBytes, wave, lane);
  __syncthreads();   // hipcc drains the LDS-DMA (vmcnt(0)) in front of the barrier

  int cur = 0;
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) {
      char* nxt = smem + (cur ^ 1) * kStageBytes;
      stage_tile(p.A, p.lda, m0, p.M, (t + 1) * BK, nxt, wave, lane);
      stage_tile(p.B, p.ldb, n0, p.N, (t + 1) * BK, nxt + kTileBytes, wave, lane);
    }
    const char* At = smem + cur * kStageBytes;
    const char* Bt = At + kTileBytes;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
      const int chunk = kk * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wr * 64 + i * 16 + (lane & 15);
        af[i] = *reinterpret_cast<const bf16x8*>(At + swz_slot(row, chunk) * 16);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = wc * 64 + j * 16 + (lane & 15);
        bfr[j] = *reinterpret_cast<const bf16x8*>(Bt + swz_slot(row, chunk) * 16);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue.  C/D layout of the 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg.
  // Fast path: each wave transposes its 64x64 fp32 sub-tile through its own 16 KiB slice of the
  // (now idle) staging LDS, 32 rows at a time, so that a lane owns 8 consecutive columns of one
  // row and every global access of the fused epilogue is a full 16-byte vector (a row of the
  // sub-tile = 256 contiguous bytes of fp32 / 128 of bf16).
  const int mw = m0 + wr * 64, nw = n0 + wc * 64;
  if (vec_ok(p) && nw + 64 <= p.N) {
    constexpr int LS = 72;                                  // padded row stride (floats)
    float* wreg = reinterpret_cast<float*>(smem + wave * 16384);
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    EpiCols cols;
    epi_cols_load<EPI>(p, nw + (lane & 7) * 8, cols);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            wreg[(ii * 16 + (lane >> 4) * 4 + r) * LS + j * 16 + (lane & 15)] = acc[half * 2 + ii][j][r];
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), c8 = (lane & 7) * 8;
        const int m = mw + half * 32 + row;
        float v[8];
        ld8(wreg + row * LS + c8, v);
        if (m < p.M) epilogue8<EPI>(p, m, nw + c8, v, cs, cols);
      }
    }
    colsum_flush(p, nw + (lane & 7) * 8, cs, lane);
    return;
  }
  float bias_n[4], vec_n[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wc * 64 + j * 16 + (lane & 15);
    const int nc = n < p.N ? n : p.N - 1;
    bias_n[j] = p.bias ? p.bias[nc] : 0.f;
    vec_n[j] = p.vec1 ? p.vec1[nc] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wr * 64 + i * 16 + (lane >> 4) * 4 + r;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + wc * 64 + j * 16 + (lane & 15);
        if (n < p.N) epilogue<EPI>(p, m, n, acc[i][j][r], bias_n[j], vec_n[j]);
      }
    }
  }
}

template <int EPI>
int launch(const GemmArgs& p, hipStream_t s, int grid) {
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_nt_kernel<EPI>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kStageBytes);
    if (e != hipSuccess) return fail(MEMHIP_ELAUNCH, "gemm: set smem attr: %s", hipGetErrorString(e));
    attr_done = true;
  }
  // (the dropout epilogue's kernel takes a GemmArgsD: the dispatcher's arguments are one)
  hipLaunchKernelGGL(gemm_nt_kernel<EPI>, dim3(grid), dim3(kThreads), 2 * kStageBytes, s,
                     static_cast<const typename EpiArgs<EPI>::type&>(p));
  return check_launch("gemm_bf16_nt");
}

// The argument checks of memhip_gemm_bf16_nt; `p` = the arguments as the launchers carry them (a GemmArgsD all the way
// down: the RESIDUAL_DROP launchers read its dropout parameters).
int validate(const memhip_gemm_args_t* a, GemmArgsD& p) {
  MEMHIP_REQUIRE(a, "gemm: null args");
  static_assert(offsetof(GemmArgs, m_base) == offsetof(memhip_gemm_args_t, dropout),
                "GemmArgs = the ABI struct up to `dropout` + internal tail");
  __builtin_memset(&p, 0, sizeof(p));
  __builtin_memcpy(&p, a, offsetof(memhip_gemm_args_t, dropout));
  MEMHIP_REQUIRE(p.M >= 0 && p.N > 0 && p.K > 0, "gemm: bad shape M=%d N=%d K=%d", p.M, p.N, p.K);
  if (p.M == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(p.K % BK == 0, "gemm: K=%d must be a multiple of %d", p.K, BK);
  MEMHIP_REQUIRE(p.A && p.B, "gemm: null operand");
  MEMHIP_REQUIRE(p.lda % 8 == 0 && p.ldb % 8 == 0 && ((uintptr_t)p.A & 15) == 0 && ((uintptr_t)p.B & 15) == 0,
                 "gemm: operands must be 16-byte aligned with ld %% 8 == 0");
  switch (p.epilogue) {
    case MEMHIP_EPI_BIAS_BF16: MEMHIP_REQUIRE(p.out0, "gemm: out0"); break;
    case MEMHIP_EPI_BIAS_GELU: MEMHIP_REQUIRE(p.out0 && p.out1, "gemm: out0/out1"); break;
    case MEMHIP_EPI_RESIDUAL:
      MEMHIP_REQUIRE(p.resid, "gemm: residual args");
      MEMHIP_REQUIRE(!p.sample_map || (!p.rowmask && p.rows_per_sample > 0), "gemm: sample_map excludes rowmask");
      break;
    case MEMHIP_EPI_DGELU: MEMHIP_REQUIRE(p.out0 && p.aux, "gemm: dgelu args"); break;
    case MEMHIP_EPI_BIAS_GELU_DG: MEMHIP_REQUIRE(p.out0 && p.out1, "gemm: out0/out1"); break;
    case MEMHIP_EPI_MUL_AUX: MEMHIP_REQUIRE(p.out0 && p.aux, "gemm: mul_aux args"); break;
    case MEMHIP_EPI_F32: MEMHIP_REQUIRE(p.out0, "gemm: out0"); break;
    case MEMHIP_EPI_PATCH_EMBED: MEMHIP_REQUIRE(p.resid && p.vec1 && p.aux, "gemm: patch args"); break;
    case MEMHIP_EPI_RESIDUAL_DROP:
      MEMHIP_REQUIRE(p.resid && a->dropout, "gemm: residual-dropout args (resid, dropout)");
      MEMHIP_REQUIRE(!p.out0, "gemm: the residual-dropout epilogue writes no bf16 branch copy (out0 must be NULL)");
      MEMHIP_REQUIRE(p.N % 8 == 0, "gemm: residual-dropout epilogue needs N %% 8 == 0 (N=%d)", p.N);
      MEMHIP_REQUIRE(!p.sample_map || (!p.rowmask && p.rows_per_sample > 0), "gemm: sample_map excludes rowmask");
      p.drop = drop_params(*a->dropout);
      break;
    default: return fail(MEMHIP_EINVAL, "gemm: unknown epilogue %d", p.epilogue);
  }
  MEMHIP_REQUIRE(!a->dropout || p.epilogue == MEMHIP_EPI_RESIDUAL_DROP, "gemm: dropout is taken by epilogue %d only",
                 MEMHIP_EPI_RESIDUAL_DROP);
  return MEMHIP_OK;
}

NtPlan plan_now(const GemmArgs& p, int stream_cus, int device_cus) {
  if (p.M == 0) return NtPlan{};
  const NtOptions o = {opt(OPT_GEMM_P8), opt(OPT_GEMM256), opt(OPT_GEMM_SPLIT), opt(OPT_GEMM_P8_HALF), opt(OPT_GEMM_P8_PAIR),
                       opt(OPT_GEMM_P8_MIN_N), opt(OPT_GEMM256_MIN_N)};
  return gemm_nt_plan(p, stream_cus, device_cus, o);
}

// Rows [row0, row0 + rows) of the product as a problem of its own.  Rows are independent, so a plan of two launches is the
// same contract on two row ranges.
GemmArgsD slice_rows(GemmArgsD p, int row0, int rows) {
  const long long r = row0;
  p.A += r * p.lda;
  if (p.out0) p.out0 = (char*)p.out0 + r * p.ldo0 * (p.epilogue == MEMHIP_EPI_F32 ? 4 : 2);
  if (p.out1) p.out1 = (char*)p.out1 + r * p.ldo1 * 2;
  // (with a sample map the residual rows are addressed through the map: resid / aux stay where they are)
  if (p.resid && !p.sample_map) p.resid += r * p.ldr;
  if (p.aux && !(p.sample_map && epi_resid(p.epilogue)))
    p.aux = (const char*)p.aux + r * p.ldaux * (epi_resid(p.epilogue) ? 4 : 2);
  p.M = rows;
  p.m_base = row0;
  return p;
}

}  // namespace

namespace memhip {
int gemm256_launch(const GemmArgs& p, const NtLaunch& l, hipStream_t s);
int gemm_p8_launch(const GemmArgs& p, const NtLaunch& l, hipStream_t s);
int gemm_p8_pair_launch(const GemmArgs& head, const GemmArgs& tail, const NtLaunch& l, hipStream_t s);
}

// validate -> plan -> launch
extern "C" int memhip_gemm_bf16_nt(const memhip_gemm_args_t* a, memhip_stream_t stream) {
  GemmArgsD p;
  if (const int rc = validate(a, p)) return rc;
  hipStream_t s = as_stream(stream);
  const NtPlan plan = plan_now(p, usable_cus(s), max_cus());
  for (int i = 0; i < plan.count; ++i) {
    const NtLaunch& l = plan.l[i];
    const GemmArgsD part = slice_rows(p, l.row0, l.rows);
    int rc;
    switch (l.kind) {
      case MEMHIP_NT_P8_PAIR: rc = gemm_p8_pair_launch(part, slice_rows(p, l.row0 + l.rows, l.tail_rows), l, s); break;
      case MEMHIP_NT_P8_256:
      case MEMHIP_NT_P8_128: rc = gemm_p8_launch(part, l, s); break;
      case MEMHIP_NT_G256: rc = gemm256_launch(part, l, s); break;
      default:             // MEMHIP_NT_128: all nine epilogues
        rc = dispatch_epilogue(part.epilogue, [&](auto E) { return launch<decltype(E)::value>(part, s, l.grid); });
    }
    if (rc != MEMHIP_OK) return rc;
  }
  return MEMHIP_OK;
}

extern "C" int memhip_gemm_bf16_nt_plan(const memhip_gemm_args_t* a, int stream_cus, int device_cus, memhip_nt_plan_t* out) {
  MEMHIP_REQUIRE(out && stream_cus >= 0 && device_cus >= 0, "gemm plan: bad arguments");
  GemmArgsD p;
  if (const int rc = validate(a, p)) return rc;
  *out = plan_now(p, stream_cus, device_cus);
  return MEMHIP_OK;
}
