// The dVAE tokenizer's decoder side: ConvTranspose2d(k = 4, stride 2, pad 1) as four 2x2 implicit GEMMs, and the KL of a row of
// token logits to the uniform distribution (reference: eventvae/vae/vae_model.py:92 the transposed layer, :160-171 decode,
// :203-206 the KL term; evaluate :216-266 calls both on a validation set).
//
// Layout as in conv.hip: bf16 NHWC with a one-pixel ZERO border, in [B, H+2, W+2, Cin] -> out [B, 2H+2, 2W+2, Cout].  With that
// border the transposed convolution splits into four output phases (py, px) in {0,1}^2, each a plain stride-1 convolution with
// a 2x2 tap window and no bounds test:
//     out[b, 2y+py, 2x+px, co] = bias[co] + sum_{dy,dx in {0,1}} sum_ci in_pad[b, y+py+dy, x+px+dx, ci] * W[ci, co, ky, kx],
//     ky = 3 - py - 2 dy,  kx = 3 - px - 2 dx        (W = torch's ConvTranspose2d weight [Cin, Cout, 4, 4])
// (in_pad in padded coordinates; the output pixel is padded position (1+2y+py, 1+2x+px)).  Per phase: M = B*H*W rows, K = 4*Cin,
// N = Cout -- the 128x128x64 MFMA tile of conv_gemm_kernel, A rows gathered by the LDS-DMA source addresses, a K-tile inside one
// tap (Cin % 64 == 0), the 16-byte epilogue after the LDS transposition.  One launch covers the four phases: the workgroup id is
// (row tile, phase, column tile), columns fastest, so the four phases of a row panel -- they read the same 3x3 neighbourhoods --
// run next to each other.  Weights are packed on the host as [4 phases][Cout][(dy, dx, ci)], K-contiguous (pack_convt_weight).
// Epilogue: + bias, optional ReLU, bf16 into the interior; the output's border ring is never written.
#include "conv_common.hpp"

namespace {

using namespace memhip;

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kThreads = 256;
constexpr int kTileBytes = BM * BK * 2;
constexpr int kStageBytes = 2 * kTileBytes;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;

struct ConvTArgs {
  const __bf16* in;     // [B, H+2, W+2, Cin] padded
  const __bf16* w;      // [4, Cout, 4*Cin]
  const float* bias;    // [Cout] or null
  __bf16* out;          // [B, 2H+2, 2W+2, Cout] padded
  int B, H, W, Cin, Cout, relu;
};

__device__ __forceinline__ unsigned pack2(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}

__global__ __launch_bounds__(kThreads, 2) void convt_gemm_kernel(ConvTArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int M = p.B * p.H * p.W;
  const int Wp = p.W + 2, K = 4 * p.Cin;
  // XCD-aware bijective remap of the block id (a row panel's phases and column tiles stay in one XCD's L2)
  const int nwg = gridDim.x;
  int pid = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = pid & 7, idx = pid >> 3;
    pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int ntn = (p.Cout + BN - 1) / BN;
  const int n0 = (pid % ntn) * BN;
  const int phase = (pid / ntn) & 3;
  const int m0 = (pid / (4 * ntn)) * BM;
  const int py = phase >> 1, px = phase & 1;

  // ---- per-lane constants of the LDS-DMA issue: instruction j of this wave covers 8 rows
  long long abase[4];      // element offset of this lane's A row (tap dy = dx = 0, channel 0)
  long long bbase[4];      // element offset of this lane's weight row
  int chunkg[4];           // global 16-byte chunk that lands at this lane's LDS position
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int inst = wave * 4 + j;
    const int row = inst * 8 + (lane >> 3);
    chunkg[j] = (lane & 7) ^ ((row >> 1) & 7);
    int m = m0 + row;
    m = m < M ? m : M - 1;
    const int hw = p.H * p.W;
    const int b = m / hw, r = m - b * hw;
    const int y = r / p.W, x = r - y * p.W;
    abase[j] = (((long long)b * (p.H + 2) + y + py) * Wp + x + px) * p.Cin;
    int n = n0 + row;
    n = n < p.Cout ? n : p.Cout - 1;
    bbase[j] = ((long long)phase * p.Cout + n) * K;
  }
  auto stage = [&](int t, char* dst) {
    const int k0 = t * BK;
    const int tap = k0 / p.Cin, c0 = k0 - tap * p.Cin;
    const long long koff = ((long long)(tap >> 1) * Wp + (tap & 1)) * p.Cin + c0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int inst = wave * 4 + j;
      glds16(p.in + abase[j] + koff + chunkg[j] * 8, dst + inst * 1024);
      glds16(p.w + bbase[j] + k0 + chunkg[j] * 8, dst + kTileBytes + inst * 1024);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / BK;
  stage(0, smem);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) stage(t + 1, smem + (cur ^ 1) * kStageBytes);
    const char* At = smem + cur * kStageBytes;
    const char* Bt = At + kTileBytes;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
      const int chunk = kk * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(At + swz_slot(wr * 64 + i * 16 + (lane & 15), chunk) * 16);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bfr[j] = *reinterpret_cast<const bf16x8*>(Bt + swz_slot(wc * 64 + j * 16 + (lane & 15), chunk) * 16);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: transpose the wave's 64x64 sub-tile through LDS, 32 rows at a time
  const int mw = m0 + wr * 64, nw = n0 + wc * 64;
  constexpr int LS = 72;
  float* wreg = reinterpret_cast<float*>(smem + wave * 16384);
  const int c8 = (lane & 7) * 8;
  const int n = nw + c8;
  float bias[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) bias[k] = (p.bias && n + k < p.Cout) ? p.bias[n + k] : 0.f;
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
      const int row = it * 8 + (lane >> 3);
      const int m = mw + half * 32 + row;
      if (m >= M || n >= p.Cout) continue;
      const int hw = p.H * p.W;
      const int b = m / hw, r = m - b * hw;
      const int y = r / p.W, x = r - y * p.W;
      const long long mo = ((long long)b * (2 * p.H + 2) + 1 + 2 * y + py) * (2 * p.W + 2) + 1 + 2 * x + px;
      const float4 v0 = *reinterpret_cast<const float4*>(wreg + row * LS + c8);
      const float4 v1 = *reinterpret_cast<const float4*>(wreg + row * LS + c8 + 4);
      float v[8] = {v0.x + bias[0], v0.y + bias[1], v0.z + bias[2], v0.w + bias[3],
                    v1.x + bias[4], v1.y + bias[5], v1.z + bias[6], v1.w + bias[7]};
      if (p.relu) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
      }
      *reinterpret_cast<uint4*>(p.out + mo * p.Cout + n) =
          uint4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
    }
  }
}

// row_kl[m] = sum_n q log q + log N, q = softmax(logits[m]) -- F.kl_div(log_uniform, log_softmax(logits), log_target) summed
// over the row (vae_model.py:203-206), without the [M, N] log_softmax matrix.  One wave per row, one pass, 16-byte loads: each
// lane keeps a running maximum mx, s = sum e^(x - mx) and t = sum e^(x - mx) (x - mx); then
//     KL = t / s - log s + log N.
// e^(x - mx) is an fp32 expf; s and t are accumulated in fp64 (the three terms of the result are ~log N each and cancel to the
// KL: fp32 sums would leave an absolute error of a few ulp(log N)); the rescale at a new maximum is exact to fp64.
template <typename T, int V>
__global__ __launch_bounds__(256) void kl_uniform_rows_kernel(const T* __restrict__ logits, long long ld, int M, int N,
                                                             float* __restrict__ row_kl) {
  typedef __attribute__((ext_vector_type(V))) T vec;
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  double mx = -INFINITY, s = 0.0, t = 0.0;
  for (int n = lane * V; n < N; n += 64 * V) {
    const vec v = *reinterpret_cast<const vec*>(logits + (long long)m * ld + n);
    float f[V];
    float vm = -INFINITY;
#pragma unroll
    for (int k = 0; k < V; ++k) { f[k] = (float)v[k]; vm = fmaxf(vm, f[k]); }
    if ((double)vm > mx) {                                  // e^(x - new) = e^(x - old) e^(old - new); x - new = (x - old) + d
      if (s > 0.0) {
        const double d = mx - (double)vm, e = exp(d);
        t = e * (t + d * s);
        s *= e;
      }
      mx = (double)vm;
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float d = (float)((double)f[k] - mx);
      const float e = expf(d);
      s += (double)e;
      t += e > 0.f ? (double)e * (double)d : 0.0;       // a -inf logit has q = 0 and adds nothing (not 0 * inf)
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double om = __shfl_xor(mx, o), os = __shfl_xor(s, o), ot = __shfl_xor(t, o);
    const double nm = om > mx ? om : mx;
    double a = 0.0, at = 0.0;
    if (s > 0.0) { const double d = mx - nm, e = exp(d); a = s * e; at = e * (t + d * s); }
    if (os > 0.0) { const double d = om - nm, e = exp(d); a += os * e; at += e * (ot + d * os); }
    mx = nm; s = a; t = at;
  }
  if (lane == 0) row_kl[m] = (float)(t / s - log(s) + log((double)N));
}

}  // namespace

static_assert(BM == kConvTileM && BN == kConvTileN && BK == kConvBK16 && 2 * kStageBytes == kConvLdsBf16, "conv_plan.hpp: tile, LDS bytes");

namespace memhip {

int convt_bf16_launch(const void* in, const void* weight, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                      int relu, const ConvPlan& plan, memhip_stream_t stream) {
  ConvTArgs p{(const __bf16*)in, (const __bf16*)weight, bias, (__bf16*)out, B, H, W, Cin, Cout, relu};
  if (int rc = conv_launch<convt_gemm_kernel>(plan.l[0], as_stream(stream), p)) return rc;
  return check_launch("convt2d_nhwc");
}

int kl_uniform_rows_launch(const void* logits, int mode, int64_t ld, int M, int N, float* row_kl, memhip_stream_t stream) {
  const dim3 grid((M + 3) / 4), block(256);
  if (mode == MEMHIP_CONV_BF16)
    hipLaunchKernelGGL((kl_uniform_rows_kernel<__bf16, 8>), grid, block, 0, as_stream(stream), (const __bf16*)logits, (long long)ld,
                       M, N, row_kl);
  else
    hipLaunchKernelGGL((kl_uniform_rows_kernel<float, 4>), grid, block, 0, as_stream(stream), (const float*)logits, (long long)ld,
                       M, N, row_kl);
  return check_launch("kl_uniform_rows");
}

}  // namespace memhip
