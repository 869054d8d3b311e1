// Element-wise dropout outside the GEMM epilogue: the exported keep mask (tests, inspection) and the in-place row
// kernel of pos_drop (mem/modeling_finetune.py:271,343), which also masks the residual-stream gradient in front of the
// embedding backward.  The mask contract: include/memhip.h (memhip_dropout_t), computed by dropout_keep8.
#include "common.h"
#include "dropout.hpp"

namespace {

using namespace memhip;

// one thread per 8-column group of a row: 8 bytes of mask
__global__ __launch_bounds__(256) void dropout_mask_kernel(DropParams d, int row0, int rows, int groups,
                                                           unsigned char* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)rows * groups) return;
  const int r = (int)(t / groups), g = (int)(t - (long long)r * groups);
  const unsigned bits = dropout_keep8(d, (unsigned)(d.row0 + row0 + r), (unsigned)g);
  unsigned lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo |= ((bits >> j) & 1u) << (8 * j);
    hi |= ((bits >> (4 + j)) & 1u) << (8 * j);
  }
  *reinterpret_cast<uint2*>(out + (long long)r * groups * 8 + (long long)g * 8) = uint2{lo, hi};
}

// x[r, 8g .. 8g+7] *= keep * scale, one thread per 8-column group (HBM-bound: 32 bytes in, 32 out per Philox call)
__global__ __launch_bounds__(256) void dropout_rows_kernel(DropParams d, float* __restrict__ x, long long ldx, int rows,
                                                           int groups) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)rows * groups) return;
  const int r = (int)(t / groups), g = (int)(t - (long long)r * groups);
  float4* p = reinterpret_cast<float4*>(x + (long long)r * ldx + (long long)g * 8);
  float4 a = p[0], b = p[1];
  const unsigned bits = dropout_keep8(d, (unsigned)(d.row0 + r), (unsigned)g);
  a.x = __fmul_rn(a.x, dropout_mul(d, bits, 0)); a.y = __fmul_rn(a.y, dropout_mul(d, bits, 1));
  a.z = __fmul_rn(a.z, dropout_mul(d, bits, 2)); a.w = __fmul_rn(a.w, dropout_mul(d, bits, 3));
  b.x = __fmul_rn(b.x, dropout_mul(d, bits, 4)); b.y = __fmul_rn(b.y, dropout_mul(d, bits, 5));
  b.z = __fmul_rn(b.z, dropout_mul(d, bits, 6)); b.w = __fmul_rn(b.w, dropout_mul(d, bits, 7));
  p[0] = a;
  p[1] = b;
}

}  // namespace

extern "C" int memhip_dropout_mask(const memhip_dropout_t* d, int row0, int rows, int cols, uint8_t* out,
                                   memhip_stream_t stream) {
  MEMHIP_REQUIRE(d, "dropout_mask: null dropout");
  MEMHIP_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0 && row0 >= 0, "dropout_mask: bad shape rows=%d cols=%d", rows, cols);
  if (rows == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(out && ((uintptr_t)out & 7) == 0, "dropout_mask: out must be 8-byte aligned");
  const long long n = (long long)rows * (cols / 8);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), drop_params(*d),
                     row0, rows, cols / 8, (unsigned char*)out);
  return check_launch("dropout_mask");
}

extern "C" int memhip_dropout_rows_f32(const memhip_dropout_t* d, float* x, int64_t ldx, int rows, int D,
                                       memhip_stream_t stream) {
  MEMHIP_REQUIRE(d, "dropout_rows_f32: null dropout");
  MEMHIP_REQUIRE(rows >= 0 && D > 0 && D % 8 == 0 && ldx % 4 == 0 && ldx >= D, "dropout_rows_f32: bad shape rows=%d D=%d", rows, D);
  if (rows == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(x && ((uintptr_t)x & 15) == 0, "dropout_rows_f32: x must be 16-byte aligned");
  const long long n = (long long)rows * (D / 8);
  hipLaunchKernelGGL(dropout_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), drop_params(*d), x,
                     (long long)ldx, rows, D / 8);
  return check_launch("dropout_rows_f32");
}
