// Row-wise / column-reducing kernels of the ViT block that sit between the MFMA GEMMs.
// All of them are HBM-bound: one wave per token row with 16-byte lane accesses (LayerNorm,
// cross-entropy), or column-owning threads sweeping a band of rows (the reductions that produce
// layer-scale / bias / LayerNorm-affine gradients), finished with one fp32 atomic per column per
// workgroup.  Reference ops: nn.LayerNorm(eps=1e-6) (mem/modeling_pretrain.py:132), the layer-scale
// + DropPath residual (mem/modeling_finetune.py:187-188), nn.CrossEntropyLoss + argmax accuracy
// (mem/engine_for_pretraining.py:152,233).
#include "common.h"
#include "dropout.hpp"

#include <type_traits>

namespace {

using namespace memhip;

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

__device__ __forceinline__ float wsum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wmax(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// a / b from r = rcp(b): q0 = a*r, one residual correction (correctly rounded away from denormals)
__device__ __forceinline__ float div_newton(float a, float b, float r) {
  const float q0 = a * r;
  return fmaf(fmaf(-q0, b, a), r, q0);
}

constexpr int kMaxChunks = 8;   // float4 chunks per lane: D <= 64*4*8 = 2048

// ---------------------------------------------------------------- what the four row kernels share
// NCH = float4 chunks per lane (D <= 256 * NCH): the per-lane arrays are sized for THIS D -- sized for the maximum they
// cost 198 VGPRs (2 waves per SIMD) and the kernel could not hide HBM latency.  FULL: D == 256 * NCH, every lane owns
// every chunk and the chunk guards do not exist (768, 1024, ...); ragged widths keep the guarded form.
template <bool FULL>
__device__ __forceinline__ bool chunk_ok(int i, int nch) {
  if constexpr (FULL) return true;
  else return i < nch;
}

// threadIdx.x >> 6 is the same in all 64 lanes but hipcc cannot prove it: through readfirstlane the row index, the map
// lookups and the row statistics below are SGPR arithmetic and scalar loads, off the vector-memory queue
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// rows r, r + stride, ... of one wave with their sample r / rps and offset r % rps: one division when the walk starts,
// then smp += q, off += rem with one carry (stride = q * rps + rem)
struct RowWalk {
  int r, smp, off, stride, q, rem, rps;
  __device__ __forceinline__ RowWalk(int r0, int stride_, int rps_) : r(r0), stride(stride_), rps(rps_) {
    smp = r0 / rps; off = r0 - smp * rps;
    q = stride / rps; rem = stride - q * rps;
  }
  __device__ __forceinline__ void next() {
    r += stride; smp += q; off += rem;
    if (off >= rps) { off -= rps; ++smp; }
  }
};

// The per-column vectors (LayerNorm gamma / beta, layer scale) are read by every row: a workgroup copies them ONCE to the
// front of its dynamic LDS (the column-sum area `red`, which is only needed after the row loop) and the rows read them with
// ds_read_b128 -- they count on lgkmcnt and never sit between a row's loads and its stores.  b == NULL: ones.
__device__ __forceinline__ void stage_columns(float4* dst, const float* a, const float* b, int nch) {
  for (int i = threadIdx.x; i < nch; i += 256) {
    dst[i] = reinterpret_cast<const float4*>(a)[i];
    dst[nch + i] = b ? reinterpret_cast<const float4*>(b)[i] : float4{1.f, 1.f, 1.f, 1.f};
  }
  __syncthreads();
}

// The lane's index into the staged vectors, made opaque once per row: hipcc otherwise hoists the (loop-invariant) LDS
// reads out of the row loop and keeps the vectors in registers -- the 12 VGPRs per vector that LDS is there to save.
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Rounding points.  The file is built with hipcc's default contraction (a * b + c may or may not become one fma, and
// which of two products is the fused one follows the shape of the surrounding code; __fmul_rn is a plain product there).
// Where a row output depends on it the choice is therefore written out, as the form these kernels have always computed:
// mul_rn is a product that is rounded (never fused into a following add), __fmaf_rn a fused one -- a later change of the
// code around them does not move a rounding.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float ln_dx(float gg, float xh, float m1, float m2) { return __fmaf_rn(-xh, m2, sub_rn(gg, m1)); }   // (gg - m1) - xh * m2, one rounding
__device__ __forceinline__ float sq2(float a, float b) { return __fmaf_rn(a, a, mul_rn(b, b)); }   // a * a + round(b * b)

// ---------------------------------------------------------------- LayerNorm forward
// one wave per output row; x fp32 (row via row_idx), y bf16, mean/rstd saved for backward.  One memory phase: the
// workgroup's share of gamma / beta is requested right behind the row itself and parked in LDS while the two reductions run.
template <int NCH, bool FULL>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, long long ldx,
                                                     const int* __restrict__ row_idx, int R, int D,
                                                     const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float eps,
                                                     __bf16* __restrict__ y, long long ldy,
                                                     float* __restrict__ mean, float* __restrict__ rstd) {
  extern __shared__ float red[];   // gamma [D], beta [D]
  const int lane = threadIdx.x & 63;
  const int r0 = blockIdx.x * 4 + wave_id();
  const bool act = r0 < R;                       // wave-uniform; an idle wave of the last workgroup redoes row R - 1 and stores nothing
  const int r = act ? r0 : R - 1;
  const long long src = row_idx ? row_idx[r] : r;
  const float4* xr = reinterpret_cast<const float4*>(x + src * ldx);
  const int nch = D >> 2;
  float4 v[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int i = lane + c * 64;
    if (chunk_ok<FULL>(i, nch)) v[c] = xr[i];
  }
  constexpr int NST = (64 * NCH + 255) / 256;      // float4 pieces of gamma, and of beta, per thread
  float4 sg[NST], sb[NST];
#pragma unroll
  for (int k = 0; k < NST; ++k) {           // unconditional (index clamped): under a lane mask hipcc waits for a load at once
    const int i = min((int)threadIdx.x + k * 256, nch - 1);
    sg[k] = reinterpret_cast<const float4*>(gamma)[i];
    sb[k] = reinterpret_cast<const float4*>(beta)[i];
  }
  __builtin_amdgcn_sched_barrier(0);          // (hipcc otherwise sinks these loads behind the first reduction)
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    if (chunk_ok<FULL>(lane + c * 64, nch)) s += (v[c].x + v[c].y) + (v[c].z + v[c].w);
  const float mu = wsum(s) / (float)D;
  float4* lgb = reinterpret_cast<float4*>(red);
#pragma unroll
  for (int k = 0; k < NST; ++k) {           // (threads past the end write the last piece once more: the same value)
    const int i = min((int)threadIdx.x + k * 256, nch - 1);
    lgb[i] = sg[k];
    lgb[nch + i] = sb[k];
  }
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (chunk_ok<FULL>(lane + c * 64, nch)) {
      const float a = v[c].x - mu, b = v[c].y - mu, cc = v[c].z - mu, d = v[c].w - mu;
      q += sq2(a, b) + sq2(cc, d);
    }
  }
  const float var = wsum(q) / (float)D;          // biased, as nn.LayerNorm
  const float rs = 1.0f / sqrtf(var + eps);
  __syncthreads();
  if (!act) return;
  if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
  bf16x4* yr = reinterpret_cast<bf16x4*>(y + (long long)r * ldy);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int i = lane + c * 64;
    if (chunk_ok<FULL>(i, nch)) {
      const float4 g = lgb[i], b = lgb[nch + i];
      bf16x4 o;
      o[0] = (__bf16)__fmaf_rn(mul_rn(v[c].x - mu, rs), g.x, b.x);
      o[1] = (__bf16)__fmaf_rn(mul_rn(v[c].y - mu, rs), g.y, b.y);
      o[2] = (__bf16)__fmaf_rn(mul_rn(v[c].z - mu, rs), g.z, b.z);
      o[3] = (__bf16)__fmaf_rn(mul_rn(v[c].w - mu, rs), g.w, b.w);
      yr[i] = o;
    }
  }
}

// ---------------------------------------------------------------- LayerNorm backward
// workgroup = 4 waves; dx per row (wave reductions), dgamma/dbeta per lane column accumulated in registers over the
// workgroup's rows, then LDS -> one atomic per column.
//
// The row loop of the three backward kernels is a three-deep software pipeline, all of it wave-uniform control flow:
//   row k + 2: its bookkeeping (row_idx / sample maps) is fetched with scalar loads,
//   row k + 1: its row loads are issued (addresses known since the iteration before) together with the scalar loads of
//              its statistics,
//   row k    : is reduced and stored; behind its stores the row of dres that row k + 1 adds to is requested (it is only
//              needed behind k + 1's reductions, and asked for this late it needs no second set of registers).
// vmcnt counts loads and stores in issue order, so a wait can leave the younger operations in flight only if their number
// is the same on every path that reaches it.  In the row loop every load and store is therefore UNCONDITIONAL:
//  - the loop only walks rows that take full part (the bookkeeping skips the others: scalar work, no vector memory),
//  - the wave's last row, which has no successor to request, requests itself again (one row per wave from the caches).
// The waits are then counted (vmcnt(n) with the next row's loads and this row's stores behind them), the next row's
// loads stay in flight across the reductions and the stores, and a store is never waited for.  The loop is entered with
// an empty queue (vm_drain), so that the counts that hold on its back-edge hold at its head.
__device__ __forceinline__ void vm_drain() { __builtin_amdgcn_s_waitcnt(0x0F70); }   // s_waitcnt vmcnt(0) alone

template <int NCH, bool FULL, bool ACC>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const __bf16* __restrict__ dy, long long lddy,
                                                     const float* __restrict__ x, long long ldx,
                                                     const int* __restrict__ row_idx, int R, int D,
                                                     const float* __restrict__ gamma,
                                                     const float* __restrict__ mean,
                                                     const float* __restrict__ rstd,
                                                     float* __restrict__ dres, long long lddres,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
  extern __shared__ float red[];   // [4][2][D]; during the row loop its front holds gamma [D]
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int nch = D >> 2;
  float4 ag[NCH], ab[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    ag[c] = float4{0, 0, 0, 0};
    ab[c] = float4{0, 0, 0, 0};
  }
  // rows are dealt to (workgroup, wave) round-robin: the column accumulators persist over ALL of a
  // workgroup's rows, so the number of same-address atomics is gridDim.x per column, not R/32
  const int rstride = gridDim.x * 4;
  float4 xn[NCH], prev[NCH];
  bf16x4 dn[NCH];
  auto issue = [&](int r, long long src, int lane) {
    const float4* xr = reinterpret_cast<const float4*>(x + src * ldx);
    const bf16x4* dyr = reinterpret_cast<const bf16x4*>(dy + (long long)r * lddy);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = lane + c * 64;
      if (chunk_ok<FULL>(i, nch)) {
        xn[c] = xr[i];
        dn[c] = dyr[i];
      }
    }
  };
  auto issue_prev = [&](long long src, int lane) {
    const float4* o = reinterpret_cast<const float4*>(dres + src * lddres);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = lane + c * 64;
      if (chunk_ok<FULL>(i, nch)) prev[c] = o[i];
    }
  };
  int r = blockIdx.x * 4 + wave;
  long long src = 0;
  float mu = 0.f, rs = 0.f;
  if (r < R) {                     // the first row is on its way while gamma is staged
    src = row_idx ? row_idx[r] : r;
    issue(r, src, lane);
    if constexpr (ACC) issue_prev(src, lane);
    mu = mean[r]; rs = rstd[r];
  }
  float4* lg = reinterpret_cast<float4*>(red);
  for (int i = threadIdx.x; i < nch; i += 256) lg[i] = reinterpret_cast<const float4*>(gamma)[i];
  __syncthreads();
  int r1 = r + rstride;
  long long src1 = 0;
  if (r1 < R) src1 = row_idx ? row_idx[r1] : r1;
  int r2 = r1 + rstride;
  vm_drain();
  while (r < R) {
    float4 xh[NCH], gg[NCH];
    float s1 = 0.f, s2 = 0.f;
    const int ol = opaque(lane);                     // (also keeps hipcc from hoisting a 64-bit lane pointer per stream)
    const float4* lgl = lg + ol;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = lane + c * 64;
      if (chunk_ok<FULL>(i, nch)) {
        const float4 xv = xn[c];
        const bf16x4 d4 = dn[c];
        const float4 g = lgl[c * 64];
        const float d0 = (float)d4[0], d1 = (float)d4[1], d2 = (float)d4[2], d3 = (float)d4[3];
        xh[c] = float4{mul_rn(xv.x - mu, rs), mul_rn(xv.y - mu, rs), mul_rn(xv.z - mu, rs), mul_rn(xv.w - mu, rs)};
        gg[c] = float4{mul_rn(d0, g.x), mul_rn(d1, g.y), mul_rn(d2, g.z), mul_rn(d3, g.w)};
        s1 += (gg[c].x + gg[c].y) + (gg[c].z + gg[c].w);
        s2 += (mul_rn(gg[c].x, xh[c].x) + mul_rn(gg[c].y, xh[c].y)) + (mul_rn(gg[c].z, xh[c].z) + mul_rn(gg[c].w, xh[c].w));
        ag[c].x += d0 * xh[c].x; ag[c].y += d1 * xh[c].y; ag[c].z += d2 * xh[c].z; ag[c].w += d3 * xh[c].w;
        ab[c].x += d0; ab[c].y += d1; ab[c].z += d2; ab[c].w += d3;
      }
    }
    float mu1 = 0.f, rs1 = 0.f;
    long long src2 = 0;
    const bool next = r1 < R;
    const int rl = next ? r1 : r;                    // the last row requests itself again
    const long long srcl = next ? src1 : src;
    issue(rl, srcl, ol);
    if (next) {
      mu1 = mean[r1]; rs1 = rstd[r1];
      if (r2 < R) src2 = row_idx ? row_idx[r2] : r2;
    }
    const float m1 = wsum(s1) / (float)D, m2 = wsum(s2) / (float)D;
    float4* o = reinterpret_cast<float4*>(dres + src * lddres);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = ol + c * 64;
      if (chunk_ok<FULL>(i, nch)) {
        const float4 t{ln_dx(gg[c].x, xh[c].x, m1, m2), ln_dx(gg[c].y, xh[c].y, m1, m2),
                       ln_dx(gg[c].z, xh[c].z, m1, m2), ln_dx(gg[c].w, xh[c].w, m1, m2)};
        float4 d;
        if constexpr (ACC) {
          const float4 p = prev[c];
          d = float4{__fmaf_rn(rs, t.x, p.x), __fmaf_rn(rs, t.y, p.y), __fmaf_rn(rs, t.z, p.z), __fmaf_rn(rs, t.w, p.w)};
        } else {
          d = float4{mul_rn(rs, t.x), mul_rn(rs, t.y), mul_rn(rs, t.z), mul_rn(rs, t.w)};
        }
        o[i] = d;
      }
    }
    if constexpr (ACC) {
      __builtin_amdgcn_sched_barrier(0);             // no load between the row's stores
      issue_prev(srcl, ol);
    }
    r = r1; src = src1; mu = mu1; rs = rs1;
    r1 = r2; src1 = src2;
    r2 += rstride;
  }
  __syncthreads();                 // every wave is done with gamma: `red` becomes the column-sum area
  float4* rg = reinterpret_cast<float4*>(red + (size_t)wave * 2 * D);
  float4* rb = reinterpret_cast<float4*>(red + (size_t)wave * 2 * D + D);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int i = lane + c * 64;
    if (chunk_ok<FULL>(i, nch)) { rg[i] = ag[c]; rb[i] = ab[c]; }
  }
  __syncthreads();
  for (int n = threadIdx.x; n < D; n += 256) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) { a += red[(size_t)w * 2 * D + n]; b += red[(size_t)w * 2 * D + D + n]; }
    atomicAdd(dgamma + n, a);
    atomicAdd(dbeta + n, b);
  }
}

// ---------------------------------------------------------------- residual-branch backward
// forward (modeling_finetune.py:187-188):  x += (gamma * y / keep) * mask[b]
// backward: dt = (dx * mask[b]) / keep ; dgamma += sum_m dt * y ; dy = bf16(dt * gamma) ;
//           dbias += sum_m dy   (the Linear that produced y)
// one wave per token row (16-byte lane accesses), rows dealt round-robin to a fixed grid so that the
// column sums cost gridDim.x atomics per column (same-address atomics are the slow part)
constexpr int kBrMaxChunks = 8;   // float4 chunks per lane: D <= 2048

// Drop = {DropParams} (memhip_branch_t.dropout): the branch had element-wise dropout, dt -> dt * keep * scale; empty: no
// dropout (the kernel arguments and code of that form are those without the parameter)
template <int NCH, bool FULL, bool HAS_Y, class... Drop>
__global__ __launch_bounds__(256) void branch_bwd_kernel(const float* __restrict__ dx, long long lddx,
                                                         const __bf16* __restrict__ y, long long ldy,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ rowmask, float keep,
                                                         int rps, int M, int D, __bf16* __restrict__ dyo,
                                                         long long lddy, float* __restrict__ dgamma,
                                                         float* __restrict__ dbias, const int* __restrict__ out_map,
                                                         Drop... drop) {
  // out_map (work-skipping stochastic depth): sample -> index of the sample among the KEPT ones, or -1.  The rows of a
  // dropped sample are neither read nor written; kept rows land at their compact position and are scaled by 1 / keep.
  extern __shared__ float red[];   // [4][2][D]; during the row loop its front holds gamma [D] (ones without one)
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int nch = D >> 2;
  float4 ag[NCH], ab[NCH];
  const float rk = __frcp_rn(keep);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    ag[c] = float4{0, 0, 0, 0};
    ab[c] = float4{0, 0, 0, 0};
  }
  // the pipeline of ln_bwd_kernel: maps two rows ahead, row loads one row ahead
  float4 dn[NCH];
  bf16x4 yn[HAS_Y ? NCH : 1];
  auto issue = [&](int m, int lane) {
    const float4* dr = reinterpret_cast<const float4*>(dx + (long long)m * lddx);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = lane + c * 64;
      if (chunk_ok<FULL>(i, nch)) {
        dn[c] = dr[i];
        if constexpr (HAS_Y) yn[c] = reinterpret_cast<const bf16x4*>(y + (long long)m * ldy)[i];
      }
    }
  };
  RowWalk w(blockIdx.x * 4 + wave, gridDim.x * 4, rps);
  // the wave's next row that has an output row (rows of dropped samples have nothing to do); leaves w behind it
  auto find = [&](int& m, int& mo, int& smp) {
    for (;;) {
      m = w.r; smp = w.smp; mo = -1;
      if (m >= M) return;
      mo = w.r;
      if (out_map) { const int co = out_map[w.smp]; mo = co < 0 ? -1 : co * w.rps + w.off; }
      w.next();
      if (mo >= 0) return;
    }
  };
  int m, mo, smp;
  float k = 1.f;
  find(m, mo, smp);
  if (m < M) {                     // the first row is on its way while gamma is staged
    issue(m, lane);
    if (rowmask) k = rowmask[smp];
  }
  float4* lg = reinterpret_cast<float4*>(red);
  for (int i = threadIdx.x; i < nch; i += 256)
    lg[i] = gamma ? reinterpret_cast<const float4*>(gamma)[i] : float4{1.f, 1.f, 1.f, 1.f};
  __syncthreads();
  int m1, mo1, smp1;
  find(m1, mo1, smp1);
  vm_drain();
  while (m < M) {
    const int ol = opaque(lane);                     // (also keeps hipcc from hoisting a 64-bit lane pointer per stream)
    float4 dv[NCH];
    bf16x4 yv[HAS_Y ? NCH : 1];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (chunk_ok<FULL>(lane + c * 64, nch)) {
        dv[c] = dn[c];
        if constexpr (HAS_Y) yv[c] = yn[c];
      }
    }
    float k1 = 1.f;
    const bool next = m1 < M;
    issue(next ? m1 : m, ol);                  // the last row requests itself again
    if (next && rowmask) k1 = rowmask[smp1];
    int m2, mo2, smp2;
    find(m2, mo2, smp2);
    bf16x4* orow = reinterpret_cast<bf16x4*>(dyo + (long long)mo * lddy);
    const float4* lgl = lg + ol;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = ol + c * 64;
      if (chunk_ok<FULL>(i, nch)) {
        float4 d = dv[c];
        if (rowmask || out_map) {            // (dx * mask) / keep: reciprocal + one Newton step = the IEEE quotient
          d.x = div_newton(d.x * k, keep, rk); d.y = div_newton(d.y * k, keep, rk);
          d.z = div_newton(d.z * k, keep, rk); d.w = div_newton(d.w * k, keep, rk);
        }
        if constexpr (sizeof...(Drop) > 0) {   // the lane's 4 columns 4i.. are one half of the 8-column group i / 2
          const DropParams dp = (drop, ...);
          const unsigned kb = dropout_keep8(dp, (unsigned)(dp.row0 + m), (unsigned)(i >> 1)) >> ((i & 1) * 4);
          d.x = __fmul_rn(d.x, dropout_mul(dp, kb, 0)); d.y = __fmul_rn(d.y, dropout_mul(dp, kb, 1));
          d.z = __fmul_rn(d.z, dropout_mul(dp, kb, 2)); d.w = __fmul_rn(d.w, dropout_mul(dp, kb, 3));
        }
        if constexpr (HAS_Y) {
          const bf16x4 yy = yv[c];
          ag[c].x += d.x * (float)yy[0]; ag[c].y += d.y * (float)yy[1];
          ag[c].z += d.z * (float)yy[2]; ag[c].w += d.w * (float)yy[3];
        }
        const float4 g = lgl[c * 64];
        bf16x4 o;
        o[0] = (__bf16)(d.x * g.x); o[1] = (__bf16)(d.y * g.y);
        o[2] = (__bf16)(d.z * g.z); o[3] = (__bf16)(d.w * g.w);
        orow[i] = o;
        ab[c].x += (float)o[0]; ab[c].y += (float)o[1]; ab[c].z += (float)o[2]; ab[c].w += (float)o[3];
      }
    }
    m = m1; mo = mo1; k = k1;
    m1 = m2; mo1 = mo2; smp1 = smp2;
  }
  __syncthreads();                 // every wave is done with gamma: `red` becomes the column-sum area
  float4* rg = reinterpret_cast<float4*>(red + (size_t)wave * 2 * D);
  float4* rb = reinterpret_cast<float4*>(red + (size_t)wave * 2 * D + D);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int i = lane + c * 64;
    if (chunk_ok<FULL>(i, nch)) { rg[i] = ag[c]; rb[i] = ab[c]; }
  }
  __syncthreads();
  for (int n = threadIdx.x; n < D; n += 256) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) { a += red[(size_t)w2 * 2 * D + n]; b += red[(size_t)w2 * 2 * D + D + n]; }
    if (dgamma) atomicAdd(dgamma + n, a);
    if (dbias) atomicAdd(dbias + n, b);
  }
}

// ---------------------------------------------------------------- fused LayerNorm backward + next branch backward
// In the backward of a block the LayerNorm gradient is added to the residual-stream gradient dx and the
// very next kernel (the backward of the previous residual branch) reads that dx back: fused, the row of
// dx is produced, stored and consumed in registers -- one pass over the fp32 gradient stream less.
//   dx[r] += LN'(dy[r]) ;  dt = dx[r] * mask[r / rps] / keep ;  dyb[r] = bf16(dt * gb) ;
//   dgamma_ln += sum dy*xhat ; dbeta_ln += sum dy ; dgb += sum dt*y ; dbias_b += sum dyb
// Drop = {DropParams} (memhip_branch_t.dropout): the produced branch gradient carries the branch's dropout mask
template <int NCH, bool FULL, bool HAS_Y, class... Drop>
__global__ __launch_bounds__(256) void ln_bwd_branch_kernel(const __bf16* __restrict__ dy, long long lddy,
                                                            const float* __restrict__ x, long long ldx, int R, int D,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            float* __restrict__ dres, long long lddres,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            const __bf16* __restrict__ yb, long long ldyb,
                                                            const float* __restrict__ gb, const float* __restrict__ rowmask,
                                                            float keep, int rps, __bf16* __restrict__ dyo, long long lddyo,
                                                            float* __restrict__ dgb, float* __restrict__ dbiasb,
                                                            const int* __restrict__ in_map, const int* __restrict__ out_map,
                                                            Drop... drop) {
  // Work-skipping stochastic depth: r runs over the rows of the residual stream (x, dres).  in_map: sample -> its index
  // among the samples the LayerNorm'ed branch KEPT (dy, mean, rstd hold those samples only), -1: that branch skipped the
  // sample, its rows get no LayerNorm gradient.  out_map: the same for the branch whose output gradient is produced
  // (dyo holds the kept samples only, scaled by 1 / keep), -1: no output row.  NULL = identity.
  extern __shared__ float red[];   // [4][4][D]; during the row loop its front holds gamma [D] and gb [D] (ones without one)
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int nch = D >> 2;
  float4 ag[NCH], ab[NCH], bg[HAS_Y ? NCH : 1], bb[NCH];      // the gamma vectors are re-read per row (LDS): 24 VGPRs
  const float rk = __frcp_rn(keep);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    ag[c] = ab[c] = bb[c] = float4{0, 0, 0, 0};
    if (HAS_Y) bg[c] = float4{0, 0, 0, 0};
  }
  // software prefetch: the raw loads of the wave's NEXT row are issued before the current row is reduced
  float4 xn[NCH], prev[NCH];
  bf16x4 dn[NCH], yn[HAS_Y ? NCH : 1];
  auto issue_x = [&](int r, int rin, int lane) {           // rin: the row's compact row in dy
    const float4* xr = reinterpret_cast<const float4*>(x + (long long)r * ldx);
    const bf16x4* dyr = reinterpret_cast<const bf16x4*>(dy + (long long)rin * lddy);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = lane + c * 64;
      if (chunk_ok<FULL>(i, nch)) {
        xn[c] = xr[i];
        dn[c] = dyr[i];
      }
    }
  };
  auto issue_y = [&](int r, int lane) {
    if constexpr (HAS_Y) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int i = lane + c * 64;
        if (chunk_ok<FULL>(i, nch)) yn[c] = reinterpret_cast<const bf16x4*>(yb + (long long)r * ldyb)[i];
      }
    }
  };
  auto issue_prev = [&](int r, int lane) {
    const float4* o = reinterpret_cast<const float4*>(dres + (long long)r * lddres);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = lane + c * 64;
      if (chunk_ok<FULL>(i, nch)) prev[c] = o[i];
    }
  };
  const int row0 = blockIdx.x * 4 + wave, rstride = gridDim.x * 4;
  auto resolve = [&](const RowWalk& t, int& rin, int& rout) {      // compact rows (-1: not taking part)
    rin = rout = t.r;
    if (in_map) { const int ci = in_map[t.smp]; rin = ci < 0 ? -1 : ci * t.rps + t.off; }
    if (out_map) { const int co = out_map[t.smp]; rout = co < 0 ? -1 : co * t.rps + t.off; }
  };
  int r, rin, rout;
  float mu = 0.f, rs = 0.f, km = 1.f;
  float4 xh[NCH], gg[NCH];
  bf16x4 yv[HAS_Y ? NCH : 1];
  float s1, s2;
  float4 *lg = reinterpret_cast<float4*>(red), *lgb = lg + nch;
  // the two halves of a row's step, on the state above
  // ol: the lane, opaque once per row (also keeps hipcc from hoisting a 64-bit lane pointer per stream)
  auto reduce_row = [&](bool has_in, int ol) {
    s1 = s2 = 0.f;
    const float4* lgl = lg + ol;
    if (has_in) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (chunk_ok<FULL>(lane + c * 64, nch)) {
          if constexpr (HAS_Y) yv[c] = yn[c];
          const float4 xv = xn[c];
          const bf16x4 d4 = dn[c];
          const float d0 = (float)d4[0], d1 = (float)d4[1], d2 = (float)d4[2], d3 = (float)d4[3];
          xh[c] = float4{mul_rn(xv.x - mu, rs), mul_rn(xv.y - mu, rs), mul_rn(xv.z - mu, rs), mul_rn(xv.w - mu, rs)};
          const float4 gmc = lgl[c * 64];
          gg[c] = float4{mul_rn(d0, gmc.x), mul_rn(d1, gmc.y), mul_rn(d2, gmc.z), mul_rn(d3, gmc.w)};
          s1 += (gg[c].x + gg[c].y) + (gg[c].z + gg[c].w);
          s2 += (mul_rn(gg[c].x, xh[c].x) + mul_rn(gg[c].y, xh[c].y)) + (mul_rn(gg[c].z, xh[c].z) + mul_rn(gg[c].w, xh[c].w));
          ag[c].x += d0 * xh[c].x; ag[c].y += d1 * xh[c].y; ag[c].z += d2 * xh[c].z; ag[c].w += d3 * xh[c].w;
          ab[c].x += d0; ab[c].y += d1; ab[c].z += d2; ab[c].w += d3;
        }
      }
    } else {                                         // no LayerNorm gradient for this row (rs = 0 below: d = prev)
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (chunk_ok<FULL>(lane + c * 64, nch)) {
          if constexpr (HAS_Y) yv[c] = yn[c];
          xh[c] = gg[c] = float4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
  };
  auto store_row = [&](bool has_in, bool has_out, int ol) {
    const float m1 = wsum(s1) / (float)D, m2 = wsum(s2) / (float)D;
    float4* o = reinterpret_cast<float4*>(dres + (long long)r * lddres);
    bf16x4* orow = reinterpret_cast<bf16x4*>(dyo + (long long)(has_out ? rout : 0) * lddyo);
    const float4* lgbl = lgb + ol;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = ol + c * 64;
      if (chunk_ok<FULL>(i, nch)) {
        float4 d{__fmaf_rn(rs, ln_dx(gg[c].x, xh[c].x, m1, m2), prev[c].x), __fmaf_rn(rs, ln_dx(gg[c].y, xh[c].y, m1, m2), prev[c].y),
                 __fmaf_rn(rs, ln_dx(gg[c].z, xh[c].z, m1, m2), prev[c].z), __fmaf_rn(rs, ln_dx(gg[c].w, xh[c].w, m1, m2), prev[c].w)};
        if (has_in) o[i] = d;
        if (!has_out) continue;
        if (rowmask || out_map) {
          d.x = div_newton(d.x * km, keep, rk); d.y = div_newton(d.y * km, keep, rk);
          d.z = div_newton(d.z * km, keep, rk); d.w = div_newton(d.w * km, keep, rk);
        }
        if constexpr (sizeof...(Drop) > 0) {     // the lane's 4 columns 4i.. are one half of the 8-column group i / 2
          const DropParams dp = (drop, ...);
          const unsigned kb = dropout_keep8(dp, (unsigned)(dp.row0 + r), (unsigned)(i >> 1)) >> ((i & 1) * 4);
          d.x = __fmul_rn(d.x, dropout_mul(dp, kb, 0)); d.y = __fmul_rn(d.y, dropout_mul(dp, kb, 1));
          d.z = __fmul_rn(d.z, dropout_mul(dp, kb, 2)); d.w = __fmul_rn(d.w, dropout_mul(dp, kb, 3));
        }
        if constexpr (HAS_Y) {
          bg[c].x += d.x * (float)yv[c][0]; bg[c].y += d.y * (float)yv[c][1];
          bg[c].z += d.z * (float)yv[c][2]; bg[c].w += d.w * (float)yv[c][3];
        }
        const float4 gbc = lgbl[c * 64];
        bf16x4 q;
        q[0] = (__bf16)(d.x * gbc.x); q[1] = (__bf16)(d.y * gbc.y);
        q[2] = (__bf16)(d.z * gbc.z); q[3] = (__bf16)(d.w * gbc.w);
        orow[i] = q;
        bb[c].x += (float)q[0]; bb[c].y += (float)q[1]; bb[c].z += (float)q[2]; bb[c].w += (float)q[3];
      }
    }
  };
  // ---- pass 1: the rows that take part in both branches, pipelined
  RowWalk w(row0, rstride, rps);
  auto find = [&](int& fr, int& frin, int& frout, int& fsmp) {     // the wave's next such row; leaves w behind it
    for (;;) {
      fr = w.r; fsmp = w.smp; frin = frout = -1;
      if (fr >= R) return;
      resolve(w, frin, frout);
      w.next();
      if ((frin | frout) >= 0) return;
    }
  };
  int smp;
  find(r, rin, rout, smp);
  if (r < R) {                     // the first row is on its way while gamma and gb are staged
    issue_x(r, rin, lane); issue_y(r, lane); issue_prev(r, lane);
    mu = mean[rin]; rs = rstd[rin];
    if (rowmask) km = rowmask[smp];
  }
  stage_columns(lg, gamma, gb, nch);
  int r1, rin1, rout1, smp1;
  find(r1, rin1, rout1, smp1);
  vm_drain();
  while (r < R) {
    const int ol = opaque(lane);
    reduce_row(true, ol);
    float mu1 = 0.f, rs1 = 0.f, km1 = 1.f;
    const bool next = r1 < R;
    const int rl = next ? r1 : r, rinl = next ? rin1 : rin;       // the last row requests itself again
    issue_x(rl, rinl, ol); issue_y(rl, ol);
    if (next) {
      mu1 = mean[rin1]; rs1 = rstd[rin1];
      if (rowmask) km1 = rowmask[smp1];
    }
    int r2, rin2, rout2, smp2;
    find(r2, rin2, rout2, smp2);
    store_row(true, true, ol);
    __builtin_amdgcn_sched_barrier(0);               // no load between the row's stores
    issue_prev(rl, ol);
    r = r1; rin = rin1; rout = rout1; mu = mu1; rs = rs1; km = km1;
    r1 = r2; rin1 = rin2; rout1 = rout2; smp1 = smp2;
  }
  // ---- pass 2: the rows of samples that ONE of the two branches dropped (dropped by both: the row of dres stays as it
  // is), one at a time behind run-time conditions, with the waits hipcc derives for them
  if (in_map || out_map) {
    for (RowWalk v(row0, rstride, rps); v.r < R; v.next()) {
      resolve(v, rin, rout);
      if ((rin >= 0) == (rout >= 0)) continue;
      r = v.r;
      const int ol = opaque(lane);
      issue_prev(r, ol); issue_y(r, ol);
      mu = rs = 0.f;
      if (rin >= 0) {
        issue_x(r, rin, ol);
        mu = mean[rin]; rs = rstd[rin];
      }
      km = rowmask ? rowmask[v.smp] : 1.f;
      reduce_row(rin >= 0, ol);
      store_row(rin >= 0, rout >= 0, ol);
    }
  }
  __syncthreads();                 // every wave is done with gamma / gb: `red` becomes the column-sum area
  float4* r0 = reinterpret_cast<float4*>(red + (size_t)wave * 4 * D);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int i = lane + c * 64;
    if (chunk_ok<FULL>(i, nch)) { r0[i] = ag[c]; r0[nch + i] = ab[c]; r0[2 * nch + i] = HAS_Y ? bg[HAS_Y ? c : 0] : float4{0, 0, 0, 0}; r0[3 * nch + i] = bb[c]; }
  }
  __syncthreads();
  for (int n = threadIdx.x; n < D; n += 256) {
    float a = 0.f, b = 0.f, c2 = 0.f, d2 = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {
      const float* rw = red + (size_t)w2 * 4 * D;
      a += rw[n]; b += rw[D + n]; c2 += rw[2 * D + n]; d2 += rw[3 * D + n];
    }
    atomicAdd(dgamma + n, a);
    atomicAdd(dbeta + n, b);
    if (dgb) atomicAdd(dgb + n, c2);
    if (dbiasb) atomicAdd(dbiasb + n, d2);
  }
}


// Layer-scale gradient without the branch output:  x += gamma * y,  y = A W^T + b  gives
//   dgamma_c = sum_m dt[m,c] y[m,c] = (sum_k W[c,k] dW[c,k] + b_c db_c) / gamma_c
// because dW[c,k] = sum_m dY[m,c] A[m,k], db_c = sum_m dY[m,c] and dY = gamma * dt: the forward does not
// have to store y (77 MB per branch at B=256) and the backward does not read it.  One wave per channel.
__global__ __launch_bounds__(256) void layerscale_grad_kernel(const __bf16* __restrict__ W, long long ldw,
                                                              const float* __restrict__ dW, long long lddw,
                                                              const float* __restrict__ b, const float* __restrict__ db,
                                                              const float* __restrict__ gamma, int N, int K,
                                                              float* __restrict__ dgamma) {
  // A workgroup takes four channels and ALL of its 256 threads walk each row (a wave per channel was latency-bound:
  // 1024 waves on the chip for the 1024 x 4096 fc2 weights of ViT-L, 24 MB in 44-54 us); the loads of the four rows are
  // independent, so up to 16 pieces per thread are in flight.
  __shared__ float red[4][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 4;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 4096) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int n = n0 + c < N ? n0 + c : N - 1;
      const __bf16* wr = W + (long long)n * ldw;
      const float* gr = dW + (long long)n * lddw;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * 1024 + (int)threadIdx.x * 4;
        if (k < K) {
          const bf16x4 w = *reinterpret_cast<const bf16x4*>(wr + k);
          const float4 g = *reinterpret_cast<const float4*>(gr + k);
          s[c] += (float)w[0] * g.x + (float)w[1] * g.y + (float)w[2] * g.z + (float)w[3] * g.w;
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float t = wsum(s[c]);
    if (lane == 0) red[wave][c] = t;
  }
  __syncthreads();
  if (threadIdx.x < 4 && n0 + (int)threadIdx.x < N) {
    const int n = n0 + threadIdx.x;
    float t = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    if (b && db) t += b[n] * db[n];
    const float g = gamma[n];
    dgamma[n] = g != 0.f ? t / g : 0.f;
  }
}

// ---------------------------------------------------------------- patch-embed / token backward
// forward (modeling_pretrain.py:101-108): row b*(L+1) = cls ; row b*(L+1)+1+p = y*(1-w) + mask_token*w
// backward: dcls += dx[cls rows]; dmask_token += sum dx*w; dy = bf16(dx*(1-w))
// A workgroup takes samples b, b + gridDim.x, ... and keeps its column sums in registers: one atomic per column and
// WORKGROUP (atomics on one address serialise at ~0.17 us each: with a workgroup per sample the 2 x 256 of them per column
// were most of the kernel's 142 us); seven rows of loads in flight per thread.
__global__ __launch_bounds__(256) void embed_bwd_kernel(const float* __restrict__ dx, long long lddx,
                                                        const unsigned char* __restrict__ mask, int B,
                                                        int L, int D, __bf16* __restrict__ dy,
                                                        long long lddy, float* __restrict__ dcls,
                                                        float* __restrict__ dmask) {
  constexpr int U = 7;
  for (int c = threadIdx.x * 4; c < D; c += 256 * 4) {
    float4 cls{0, 0, 0, 0}, am{0, 0, 0, 0};
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
      const float* row0 = dx + (long long)b * (L + 1) * lddx + c;
      const float4 dc = *reinterpret_cast<const float4*>(row0);
      cls.x += dc.x; cls.y += dc.y; cls.z += dc.z; cls.w += dc.w;
      const unsigned char* mk = mask + (long long)b * L;
      __bf16* out = dy + (long long)b * L * lddy + c;
      int p = 0;
      for (; p + U <= L; p += U) {
        float4 d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = *reinterpret_cast<const float4*>(row0 + (long long)(1 + p + u) * lddx);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float w = (float)mk[p + u], q = 1.0f - w;
          am.x += d[u].x * w; am.y += d[u].y * w; am.z += d[u].z * w; am.w += d[u].w * w;
          bf16x4 o;
          o[0] = (__bf16)(d[u].x * q); o[1] = (__bf16)(d[u].y * q); o[2] = (__bf16)(d[u].z * q); o[3] = (__bf16)(d[u].w * q);
          *reinterpret_cast<bf16x4*>(out + (long long)(p + u) * lddy) = o;
        }
      }
      for (; p < L; ++p) {
        const float4 d = *reinterpret_cast<const float4*>(row0 + (long long)(1 + p) * lddx);
        const float w = (float)mk[p], q = 1.0f - w;
        am.x += d.x * w; am.y += d.y * w; am.z += d.z * w; am.w += d.w * w;
        bf16x4 o;
        o[0] = (__bf16)(d.x * q); o[1] = (__bf16)(d.y * q); o[2] = (__bf16)(d.z * q); o[3] = (__bf16)(d.w * q);
        *reinterpret_cast<bf16x4*>(out + (long long)p * lddy) = o;
      }
    }
    atomicAdd(dcls + c, cls.x); atomicAdd(dcls + c + 1, cls.y);
    atomicAdd(dcls + c + 2, cls.z); atomicAdd(dcls + c + 3, cls.w);
    atomicAdd(dmask + c, am.x); atomicAdd(dmask + c + 1, am.y);
    atomicAdd(dmask + c + 2, am.z); atomicAdd(dmask + c + 3, am.w);
  }
}

// ---------------------------------------------------------------- softmax cross-entropy
// one 256-thread workgroup per masked-token row; logits bf16 (the lm_head output under autocast),
// statistics in fp32.  Writes the row loss, "argmax == label" and (in place) dlogits = (softmax -
// onehot) * grad_scale as bf16.
template <int VPT>   // bf16x8 chunks per thread
__global__ __launch_bounds__(256) void ce_kernel(__bf16* __restrict__ logits, long long ld,
                                                 const long long* __restrict__ labels, int V,
                                                 float grad_scale, float* __restrict__ row_loss,
                                                 int* __restrict__ row_correct, int write_grad) {
  __shared__ float sm[4];
  __shared__ int si[4];
  __shared__ float bc[2];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bf16x8* row = reinterpret_cast<bf16x8*>(logits + (long long)r * ld);
  const int nch = V >> 3;
  float v[VPT][8];
  float mx = -INFINITY;
  int amax = 0x7fffffff;
#pragma unroll
  for (int c = 0; c < VPT; ++c) {
    const int i = tid + c * 256;
    if (i < nch) {
      const bf16x8 t = row[i];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[c][k] = (float)t[k];
        if (v[c][k] > mx) { mx = v[c][k]; amax = i * 8 + k; }   // first index of the max in this thread
      }
    }
  }
  // (max, smallest index) reduction == torch.max(-1) on CPU (first occurrence)
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o);
    const int oi = __shfl_xor(amax, o);
    if (om > mx || (om == mx && oi < amax)) { mx = om; amax = oi; }
  }
  if (lane == 0) { sm[wave] = mx; si[wave] = amax; }
  __syncthreads();
  if (tid == 0) {
    float m = sm[0]; int a = si[0];
    for (int w = 1; w < 4; ++w) if (sm[w] > m || (sm[w] == m && si[w] < a)) { m = sm[w]; a = si[w]; }
    bc[0] = m; si[0] = a;
  }
  __syncthreads();
  mx = bc[0];
  amax = si[0];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < VPT; ++c) {
    const int i = tid + c * 256;
    if (i < nch) {
#pragma unroll
      for (int k = 0; k < 8; ++k) { v[c][k] = __expf(v[c][k] - mx); s += v[c][k]; }
    }
  }
  s = wsum(s);
  __syncthreads();
  if (lane == 0) sm[wave] = s;
  __syncthreads();
  if (tid == 0) bc[1] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  __syncthreads();
  const float sum = bc[1];
  const long long lab = labels[r];
  if (tid == 0) {
    // a label outside [0, V) (torch: "Target out of bounds") must not become an out-of-bounds read: the row's loss is
    // NaN, which the training loop's non-finite-loss abort reports (engine_for_pretraining.py:154-156)
    const bool lab_ok = lab >= 0 && lab < V;
    const float zl = lab_ok ? (float)logits[(long long)r * ld + lab] : __builtin_nanf("");
    row_loss[r] = (mx + __logf(sum)) - zl;        // -log_softmax[label]
    row_correct[r] = (amax == (int)lab) ? 1 : 0;
  }
  if (write_grad) {
    const float inv = 1.0f / sum;
    __syncthreads();                              // tid 0 has read logits[label] before it is overwritten
#pragma unroll
    for (int c = 0; c < VPT; ++c) {
      const int i = tid + c * 256;
      if (i < nch) {
        bf16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float p = v[c][k] * inv;
          if ((long long)(i * 8 + k) == lab) p -= 1.0f;
          o[k] = (__bf16)(p * grad_scale);
        }
        row[i] = o;
      }
    }
  }
}

__global__ __launch_bounds__(256) void ce_reduce_kernel(const float* __restrict__ row_loss,
                                                        const int* __restrict__ row_correct, int M,
                                                        float* __restrict__ out) {
  __shared__ double sd[4];
  __shared__ int sc[4];
  double s = 0.0;
  int c = 0;
  for (int i = threadIdx.x; i < M; i += 256) { s += (double)row_loss[i]; c += row_correct[i]; }
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); c += __shfl_xor(c, o); }
  if ((threadIdx.x & 63) == 0) { sd[threadIdx.x >> 6] = s; sc[threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double t = (sd[0] + sd[1]) + (sd[2] + sd[3]);
    const int k = sc[0] + sc[1] + sc[2] + sc[3];
    out[0] = (float)(t / (double)M);          // nn.CrossEntropyLoss(reduction="mean")
    out[1] = (float)k / (float)M;             // mlm_acc
  }
}

}  // namespace

// NCH and FULL of a width as template arguments: f(std::integral_constant<int, NCH>{}, std::bool_constant<FULL>{}), the guard-free
// instantiation wherever every lane owns every chunk (D a multiple of 256).  MAXN = 4: a kernel whose widths end at 1024;
// 8: beyond 1024 only 1280 and 2048 have a form of their own, every other width takes the guarded <8>
template <int MAXN, class F>
void dispatch_width(int D, F&& f) {
  const int nch = cdiv(D / 4, 64);
  const bool full = D % 256 == 0;
  const auto either = [&](auto N) { if (full) f(N, std::true_type{}); else f(N, std::false_type{}); };
  if (nch <= 1) either(std::integral_constant<int, 1>{});
  else if (nch <= 2) either(std::integral_constant<int, 2>{});
  else if (nch <= 3) either(std::integral_constant<int, 3>{});
  else if (MAXN == 4 || nch <= 4) either(std::integral_constant<int, 4>{});
  else if constexpr (MAXN == 8) {
    if (nch == 5 && full) f(std::integral_constant<int, 5>{}, std::true_type{});
    else if (nch == 8 && full) f(std::integral_constant<int, 8>{}, std::true_type{});
    else f(std::integral_constant<int, 8>{}, std::false_type{});
  }
}

extern "C" int memhip_layernorm_fwd(const float* x, int64_t ldx, const int32_t* row_idx, int R, int D,
                                    const float* gamma, const float* beta, float eps, void* y,
                                    int64_t ldy, float* mean, float* rstd, memhip_stream_t stream) {
  MEMHIP_REQUIRE(R >= 0 && D > 0 && D % 4 == 0 && D <= 64 * 4 * kMaxChunks, "layernorm_fwd: bad R=%d D=%d", R, D);
  if (R == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(x && gamma && beta && y && mean && rstd, "layernorm_fwd: null pointer");
  MEMHIP_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0, "layernorm_fwd: ld must be a multiple of 4");
  dispatch_width<kMaxChunks>(D, [&](auto N, auto F) {
    hipLaunchKernelGGL((ln_fwd_kernel<decltype(N)::value, decltype(F)::value>), dim3(cdiv(R, 4)), dim3(256), (size_t)2 * D * sizeof(float), as_stream(stream),
                       x, (long long)ldx, row_idx, R, D, gamma, beta, eps, (__bf16*)y, (long long)ldy, mean, rstd);
  });
  return check_launch("layernorm_fwd");
}

extern "C" int memhip_layernorm_bwd(const void* dy, int64_t lddy, const float* x, int64_t ldx,
                                    const int32_t* row_idx, int R, int D, const float* gamma,
                                    const float* mean, const float* rstd, float* dres, int64_t lddres,
                                    int accumulate, float* dgamma, float* dbeta, memhip_stream_t stream) {
  MEMHIP_REQUIRE(R >= 0 && D > 0 && D % 4 == 0 && D <= 64 * 4 * kMaxChunks, "layernorm_bwd: bad R=%d D=%d", R, D);
  if (R == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(dy && x && gamma && mean && rstd && dres && dgamma && dbeta, "layernorm_bwd: null pointer");
  MEMHIP_REQUIRE(ldx % 4 == 0 && lddy % 4 == 0 && lddres % 4 == 0, "layernorm_bwd: ld must be a multiple of 4");
  int grid = cdiv(R, 4);
  const int cap = opt(OPT_LN_BWD_GRID) * 4 / 3;      // (4/3 of the fused kernel's grid: this one needs half the LDS per workgroup)
  if (grid > cap) grid = cap;
  dispatch_width<kMaxChunks>(D, [&](auto N, auto F) {
    dispatch_bool(accumulate, [&](auto A) {
      hipLaunchKernelGGL((ln_bwd_kernel<decltype(N)::value, decltype(F)::value, decltype(A)::value>), dim3(grid), dim3(256), (size_t)8 * D * sizeof(float), as_stream(stream),
                         (const __bf16*)dy, (long long)lddy, x, (long long)ldx, row_idx, R, D, gamma, mean, rstd, dres,
                         (long long)lddres, dgamma, dbeta);
      return 0;
    });
  });
  return check_launch("layernorm_bwd");
}

// the one launch text of branch_bwd_kernel; drop = drop_params(*dropout) or nothing
template <int NCH, bool FULL, bool HAS_Y, class... Drop>
static void branch_bwd_launch(const memhip_branch_bwd_args_t& a, int grid, memhip_stream_t stream, Drop... drop) {
  const memhip_branch_t& b = a.branch;
  hipLaunchKernelGGL((branch_bwd_kernel<NCH, FULL, HAS_Y, Drop...>), dim3(grid), dim3(256), (size_t)8 * a.D * sizeof(float),
                     as_stream(stream), a.dx, (long long)a.lddx, (const __bf16*)b.y, (long long)b.ldy, b.gamma, b.rowmask,
                     b.keep_prob, b.rows_per_sample > 0 ? b.rows_per_sample : 1, a.M, a.D, (__bf16*)b.dy, (long long)b.lddy,
                     b.dgamma, b.dbias, (const int*)b.out_map, drop...);
}

extern "C" int memhip_branch_bwd(const memhip_branch_bwd_args_t* args, memhip_stream_t stream) {
  MEMHIP_REQUIRE(args, "branch_bwd: null args");
  const memhip_branch_t& b = args->branch;
  const int M = args->M, D = args->D;
  MEMHIP_REQUIRE(M >= 0 && D > 0 && D % 4 == 0, "branch_bwd: bad M=%d D=%d", M, D);
  MEMHIP_REQUIRE(!b.dropout || D % 8 == 0, "branch_bwd_drop: D=%d must be a multiple of 8", D);
  MEMHIP_REQUIRE(!b.out_map || (!b.rowmask && !b.y && b.rows_per_sample > 0), "branch_bwd: out_map excludes rowmask / y");
  if (M == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(args->dx && b.dy, "branch_bwd: null pointer");
  MEMHIP_REQUIRE(b.y || !b.dgamma, "branch_bwd: dgamma needs y (or use memhip_layerscale_grad)");
  MEMHIP_REQUIRE(args->lddx % 4 == 0 && b.ldy % 4 == 0 && b.lddy % 4 == 0, "branch_bwd: ld must be a multiple of 4");
  MEMHIP_REQUIRE(D <= 64 * 4 * kBrMaxChunks, "branch_bwd: D=%d too large", D);
  int grid = cdiv(M, 4);
  if (grid > 1024) grid = 1024;
  dispatch_width<kBrMaxChunks>(D, [&](auto N, auto F) {
    dispatch_bool(b.y, [&](auto Y) {
      if (b.dropout) branch_bwd_launch<decltype(N)::value, decltype(F)::value, decltype(Y)::value>(*args, grid, stream, drop_params(*b.dropout));
      else branch_bwd_launch<decltype(N)::value, decltype(F)::value, decltype(Y)::value>(*args, grid, stream);
      return 0;
    });
  });
  return check_launch("branch_bwd");
}

extern "C" int memhip_embed_bwd(const float* dx, int64_t lddx, const uint8_t* mask, int B, int L, int D,
                                void* dy, int64_t lddy, float* dcls, float* dmask_token,
                                memhip_stream_t stream) {
  MEMHIP_REQUIRE(B >= 0 && L > 0 && D > 0 && D % 4 == 0, "embed_bwd: bad shape");
  if (B == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(dx && mask && dy && dcls && dmask_token, "embed_bwd: null pointer");
  hipLaunchKernelGGL(embed_bwd_kernel, dim3(B < 128 ? B : 128), dim3(256), 0, as_stream(stream), dx, (long long)lddx, mask, B,
                     L, D, (__bf16*)dy, (long long)lddy, dcls, dmask_token);
  return check_launch("embed_bwd");
}

extern "C" int memhip_cross_entropy(void* logits, int64_t ld, const int64_t* labels, int M, int V,
                                    float grad_scale, float* row_loss, int32_t* row_correct,
                                    int write_grad, float* out2, memhip_stream_t stream) {
  MEMHIP_REQUIRE(M >= 0 && V > 0 && V % 8 == 0 && V <= 256 * 8 * 8, "cross_entropy: V=%d unsupported", V);
  if (M == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(logits && labels && row_loss && row_correct && out2, "cross_entropy: null pointer");
  MEMHIP_REQUIRE(ld % 8 == 0, "cross_entropy: ld must be a multiple of 8");
  hipStream_t s = as_stream(stream);
  const int nch = V / 8, vpt = cdiv(nch, 256);
  __bf16* lg = (__bf16*)logits;
  const long long* lab = (const long long*)labels;
#define CE_LAUNCH(N) hipLaunchKernelGGL(ce_kernel<N>, dim3(M), dim3(256), 0, s, lg, (long long)ld, lab, V, \
                                        grad_scale, row_loss, row_correct, write_grad)
  if (vpt <= 1) CE_LAUNCH(1);
  else if (vpt <= 2) CE_LAUNCH(2);
  else if (vpt <= 4) CE_LAUNCH(4);
  else CE_LAUNCH(8);
#undef CE_LAUNCH
  hipLaunchKernelGGL(ce_reduce_kernel, dim3(1), dim3(256), 0, s, row_loss, row_correct, M, out2);
  return check_launch("cross_entropy");
}

// the one launch text of ln_bwd_branch_kernel; drop = drop_params(*dropout) or nothing
template <int NCH, bool FULL, bool HAS_Y, class... Drop>
static void ln_bwd_branch_launch(const memhip_ln_bwd_branch_args_t& a, int grid, memhip_stream_t stream, Drop... drop) {
  const memhip_branch_t& b = a.branch;
  hipLaunchKernelGGL((ln_bwd_branch_kernel<NCH, FULL, HAS_Y, Drop...>), dim3(grid), dim3(256), (size_t)16 * a.D * sizeof(float),
                     as_stream(stream), (const __bf16*)a.dy, (long long)a.lddy, a.x, (long long)a.ldx, a.R, a.D, a.gamma, a.mean,
                     a.rstd, a.dres, (long long)a.lddres, a.dgamma, a.dbeta, (const __bf16*)b.y, (long long)b.ldy, b.gamma,
                     b.rowmask, b.keep_prob, b.rows_per_sample > 0 ? b.rows_per_sample : 1, (__bf16*)b.dy, (long long)b.lddy,
                     b.dgamma, b.dbias, (const int*)a.in_map, (const int*)b.out_map, drop...);
}

extern "C" int memhip_layernorm_bwd_branch(const memhip_ln_bwd_branch_args_t* args, memhip_stream_t stream) {
  MEMHIP_REQUIRE(args, "layernorm_bwd_branch: null args");
  const memhip_ln_bwd_branch_args_t& a = *args;
  const memhip_branch_t& b = a.branch;
  const int R = a.R, D = a.D;
  MEMHIP_REQUIRE(R >= 0 && D > 0 && D % 4 == 0 && D <= 64 * 4 * 4, "layernorm_bwd_branch: D=%d unsupported (<= 1024)", D);
  MEMHIP_REQUIRE(!b.dropout || D % 8 == 0, "layernorm_bwd_branch_drop: D=%d must be a multiple of 8", D);
  MEMHIP_REQUIRE(!(a.in_map || b.out_map) || (!b.rowmask && !b.y && b.rows_per_sample > 0),
                 "layernorm_bwd_branch: sample maps exclude rowmask / y_branch");
  if (R == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(a.dy && a.x && a.gamma && a.mean && a.rstd && a.dres && a.dgamma && a.dbeta && b.dy,
                 "layernorm_bwd_branch: null pointer");
  MEMHIP_REQUIRE(b.y || !b.dgamma, "layernorm_bwd_branch: dgamma_branch needs y_branch");
  MEMHIP_REQUIRE(a.ldx % 4 == 0 && a.lddy % 4 == 0 && a.lddres % 4 == 0 && b.ldy % 4 == 0 && b.lddy % 4 == 0,
                 "layernorm_bwd_branch: ld must be a multiple of 4");
  int grid = cdiv(R, 4);
  int cap = opt(OPT_LN_BWD_GRID);                      // 2048 (round 5).  768 = 3 resident workgroups per CU = one full round was the optimum of the
                                                       // kernel ALONE; inside the step it runs beside the weight-gradient workgroups of the other stream (128 KB of
                                                       // LDS each: a CU that holds one has no room for this kernel's 48 KB) and more, shorter workgroups find the
                                                       // free CUs sooner: 512 / 768 / 1024 / 1536 / 2048 / 3072 / 4096 = 35.0 / 34.64 / 34.6 / 34.45 / 34.35-34.43 /
                                                       // 34.5 / 34.65 ms per step (tools/exp/r05_run27.sh); ViT-L step 219 -> 216 ms
  if (D > 768 && cap > 512) cap = 512;                 // D = 1024: 64 KiB of LDS and 212 VGPRs per workgroup, two per CU (tools/ln_bwd_probe.py:
                                                       // 76 864 rows 301 -> 262 us, 19 216 rows 69 -> 64 us)
  if (grid > cap) grid = cap;
  dispatch_width<4>(D, [&](auto N, auto F) {     // (dropout outside HAS_Y: the order in which the instantiations have always been emitted)
    if (b.dropout)
      dispatch_bool(b.y, [&](auto Y) {
        ln_bwd_branch_launch<decltype(N)::value, decltype(F)::value, decltype(Y)::value>(a, grid, stream, drop_params(*b.dropout));
        return 0;
      });
    else
      dispatch_bool(b.y, [&](auto Y) {
        ln_bwd_branch_launch<decltype(N)::value, decltype(F)::value, decltype(Y)::value>(a, grid, stream);
        return 0;
      });
  });
  return check_launch("layernorm_bwd_branch");
}

extern "C" int memhip_layerscale_grad(const void* W_bf16, int64_t ldw, const float* dW, int64_t lddw, const float* bias,
                                      const float* dbias, const float* gamma, int N, int K, float* dgamma,
                                      memhip_stream_t stream) {
  MEMHIP_REQUIRE(N >= 0 && K > 0 && K % 4 == 0 && ldw % 4 == 0 && lddw % 4 == 0, "layerscale_grad: bad shape");
  if (N == 0) return MEMHIP_OK;
  MEMHIP_REQUIRE(W_bf16 && dW && gamma && dgamma && (!bias == !dbias), "layerscale_grad: null pointer");
  hipLaunchKernelGGL(layerscale_grad_kernel, dim3((N + 3) / 4), dim3(256), 0, as_stream(stream), (const __bf16*)W_bf16,
                     (long long)ldw, dW, (long long)lddw, bias, dbias, gamma, N, K, dgamma);
  return check_launch("layerscale_grad");
}
