// The finetuning recipe around the ViT step (mem/run_class_finetuning.py:504-527,609-616,654): mixup / cutmix of the image
// batch with its soft targets (timm.data.Mixup), the soft-target / label-smoothing cross-entropy
// (timm.loss.SoftTargetCrossEntropy, LabelSmoothingCrossEntropy) and the weight EMA (timm.utils.ModelEma.update).
// Mixup and the EMA are single streaming passes with 16-byte lane accesses (byte floors 2 x batch bytes and 12 B per
// parameter); the loss is a row kernel of ce_kernel's shape (rowops.hip) without its multiple-of-8 class count.
#include "common.h"

namespace {

using namespace memhip;

constexpr int kT = 256;

// ---------------------------------------------------------------- mixup / cutmix, in place
// Sample i mixes with sample j = B - 1 - i of the batch BEFORE the call (timm: x.flip(0)).  One work-item owns the same
// VEC elements of BOTH samples of a pair: it reads both, then writes both, so the in-place form needs no copy of the
// batch and has no race (the middle sample of an odd batch pairs with itself and is written once).
// Per sample: box = (yl, yh, xl, xh); a box without area means "blend with lam"; lam == 1 without a box leaves the sample
// untouched bit for bit (timm skips such samples), and a pair of two untouched samples is not even read.
struct MixParam { float lam; int yl, yh, xl, xh; bool box, keep; };

__device__ __forceinline__ MixParam mix_param(const float* lam, const int* box, int i) {
  MixParam m;
  m.lam = lam[i];
  m.yl = box[4 * i]; m.yh = box[4 * i + 1]; m.xl = box[4 * i + 2]; m.xh = box[4 * i + 3];
  m.box = m.yh > m.yl && m.xh > m.xl;
  m.keep = !m.box && m.lam == 1.0f;
  return m;
}

__device__ __forceinline__ float mix_one(const MixParam& m, float own, float other, int h, int w) {
  if (m.box) return (h >= m.yl && h < m.yh && w >= m.xl && w < m.xh) ? other : own;
  return m.lam * own + (1.0f - m.lam) * other;
}

template <int VEC>   // 4: 16-byte accesses (C*H*W a multiple of 4, x 16-byte aligned); 1: any shape
__global__ __launch_bounds__(kT) void mixup_kernel(float* __restrict__ x, int B, long long n, int H, int W,
                                                   const float* __restrict__ lam, const int* __restrict__ box) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  const int i = blockIdx.y, j = B - 1 - i;
  const MixParam mi = mix_param(lam, box, i), mj = mix_param(lam, box, j);
  if (mi.keep && mj.keep) return;
  vec_t* xi = reinterpret_cast<vec_t*>(x + (long long)i * n);
  vec_t* xj = reinterpret_cast<vec_t*>(x + (long long)j * n);
  const long long nq = n / VEC;
  for (long long q = (long long)blockIdx.x * kT + threadIdx.x; q < nq; q += (long long)gridDim.x * kT) {
    const vec_t a = __builtin_nontemporal_load(xi + q);
    const vec_t b = (i == j) ? a : __builtin_nontemporal_load(xj + q);
    const long long e = q * VEC;
    int w = (int)(e % W), h = (int)((e / W) % H);
    vec_t oa, ob;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      oa[k] = mix_one(mi, a[k], b[k], h, w);
      ob[k] = mix_one(mj, b[k], a[k], h, w);
      if (++w == W) { w = 0; if (++h == H) h = 0; }
    }
    if (!mi.keep) xi[q] = oa;
    if (i != j && !mj.keep) xj[q] = ob;
  }
}

// ---------------------------------------------------------------- soft targets of a mixed batch
// timm.data.mixup.mixup_target: t[i] = lam[i] * onehot(labels[i]) + (1 - lam[i]) * onehot(labels[B-1-i]) with the
// smoothed one-hot (off = smoothing / V elsewhere, on = 1 - smoothing + off at the label).  One workgroup per row.
__global__ __launch_bounds__(kT) void mix_targets_kernel(const long long* __restrict__ labels,
                                                         const float* __restrict__ lam, int B, int V, double on,
                                                         double off, float* __restrict__ t, long long ldt) {
  const int i = blockIdx.x;
  const long long a = labels[i], b = labels[B - 1 - i];
  const double l = (double)lam[i];
  // a label outside [0, V) never indexes anything here; the row becomes NaN (memhip_cross_entropy's convention), which
  // the training loop's non-finite-loss abort reports
  const bool ok = a >= 0 && a < V && b >= 0 && b < V;
  for (int c = threadIdx.x; c < V; c += kT) {
    const double v = l * (c == a ? on : off) + (1.0 - l) * (c == b ? on : off);
    t[(long long)i * ldt + c] = ok ? (float)v : __builtin_nanf("");
  }
}

// ---------------------------------------------------------------- soft-target / label-smoothing cross-entropy
__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__bf16 v) { return (float)v; }

// (max, smallest index of it) over the workgroup == torch.max(-1) on CPU (first occurrence); every thread gets the result
__device__ __forceinline__ void block_argmax(float& mx, int& amax, float* sm, int* si) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o);
    const int oi = __shfl_xor(amax, o);
    if (om > mx || (om == mx && oi < amax)) { mx = om; amax = oi; }
  }
  __syncthreads();
  if (lane == 0) { sm[wave] = mx; si[wave] = amax; }
  __syncthreads();
  mx = sm[0]; amax = si[0];
  for (int w = 1; w < kT / 64; ++w)
    if (sm[w] > mx || (sm[w] == mx && si[w] < amax)) { mx = sm[w]; amax = si[w]; }
}

__device__ __forceinline__ float block_sum(float v, float* sm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// One 256-thread workgroup per row, column c = tid + k * 256 (scalar, coalesced accesses: a row of an arbitrary class
// count starts at no particular alignment), logits kept in registers, statistics in fp32.
//   target != NULL: loss = -sum_c t_c * log_softmax(x)_c                      (SoftTargetCrossEntropy)
//   else:           loss = (1 - s) * nll + s * mean_c(-log_softmax(x)_c)      (LabelSmoothingCrossEntropy)
// dlogits = grad_scale * (softmax * sum_c t_c - t); it may alias the logits (every read of the row precedes its writes).
template <typename T, int N>
__global__ __launch_bounds__(kT) void ce_soft_kernel(const T* logits, long long ld,
                                                     const float* __restrict__ target, long long ldt,
                                                     const long long* __restrict__ labels, float smoothing, int V,
                                                     float grad_scale, T* dlogits, long long lddl,
                                                     float* __restrict__ row_loss, int* __restrict__ row_correct,
                                                     int write_grad) {
  __shared__ float sm[kT / 64];
  __shared__ int si[kT / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const T* row = logits + (long long)r * ld;
  const float* trow = target ? target + (long long)r * ldt : nullptr;
  float v[N];
  float mx = -INFINITY, tmx = -INFINITY;
  int amax = 0x7fffffff, tamax = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int c = tid + k * kT;
    if (c < V) {
      v[k] = to_f32(row[c]);
      if (v[k] > mx) { mx = v[k]; amax = c; }
      if (trow) {
        const float t = trow[c];
        if (t > tmx) { tmx = t; tamax = c; }
      }
    }
  }
  block_argmax(mx, amax, sm, si);
  long long lab;
  if (trow) {
    block_argmax(tmx, tamax, sm, si);
    lab = tamax;
  } else {
    lab = labels[r];
  }
  // sums over the row of exp(x - max), t and t * (x - max)   [labels: of x - max in place of the last two]
  float s_exp = 0.f, s_t = 0.f, s_tx = 0.f;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int c = tid + k * kT;
    if (c < V) {
      const float d = v[k] - mx;
      v[k] = expf(d);
      s_exp += v[k];
      if (trow) {
        const float t = trow[c];
        s_t += t;
        s_tx += t * d;
      } else {
        s_t += d;
        if (c == lab) s_tx = d;
      }
    }
  }
  s_exp = block_sum(s_exp, sm);
  s_t = block_sum(s_t, sm);
  s_tx = block_sum(s_tx, sm);
  const float lse = logf(s_exp);                   // log-sum-exp of the shifted row
  const bool lab_ok = trow || (lab >= 0 && lab < V);
  float tsum;
  if (trow) {
    tsum = s_t;
    if (tid == 0) row_loss[r] = lse * s_t - s_tx;
  } else {
    tsum = 1.0f;
    // a label outside [0, V) matches no column above, indexes nothing, and gives a NaN row (memhip_cross_entropy)
    const float nll = lab_ok ? lse - s_tx : __builtin_nanf("");
    if (tid == 0) row_loss[r] = (1.0f - smoothing) * nll + smoothing * (lse - s_t / (float)V);
  }
  if (tid == 0) row_correct[r] = (lab_ok && amax == (int)lab) ? 1 : 0;
  if (write_grad) {
    const float inv = tsum / s_exp;
    const float off = smoothing / (float)V, on = 1.0f - smoothing + off;
    T* drow = dlogits + (long long)r * lddl;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int c = tid + k * kT;
      if (c < V) {
        const float t = trow ? trow[c] : (c == lab ? on : off);
        drow[c] = (T)((v[k] * inv - t) * grad_scale);
      }
    }
  }
}

__global__ __launch_bounds__(kT) void ce_soft_reduce_kernel(const float* __restrict__ row_loss,
                                                            const int* __restrict__ row_correct, int M,
                                                            float* __restrict__ out) {
  __shared__ double sd[kT / 64];
  __shared__ int sc[kT / 64];
  double s = 0.0;
  int c = 0;
  for (int i = threadIdx.x; i < M; i += kT) { s += (double)row_loss[i]; c += row_correct[i]; }
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); c += __shfl_xor(c, o); }
  if ((threadIdx.x & 63) == 0) { sd[threadIdx.x >> 6] = s; sc[threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = (float)(((sd[0] + sd[1]) + (sd[2] + sd[3])) / (double)M);   // reduction "mean" over the batch
    out[1] = (float)(sc[0] + sc[1] + sc[2] + sc[3]) / (float)M;
  }
}

template <typename T>
int ce_soft_launch(const void* logits, int64_t ld, const float* target, int64_t ldt, const int64_t* labels,
                   float smoothing, int M, int V, float grad_scale, void* dlogits, int64_t lddl, float* row_loss,
                   int32_t* row_correct, int write_grad, hipStream_t s) {
  const int n = cdiv(V, kT);
#define CE_SOFT(N) hipLaunchKernelGGL((ce_soft_kernel<T, N>), dim3(M), dim3(kT), 0, s, (const T*)logits, (long long)ld, \
                                      target, (long long)ldt, (const long long*)labels, smoothing, V, grad_scale,       \
                                      (T*)dlogits, (long long)lddl, row_loss, row_correct, write_grad)
  if (n <= 1) CE_SOFT(1);
  else if (n <= 2) CE_SOFT(2);
  else if (n <= 4) CE_SOFT(4);
  else if (n <= 8) CE_SOFT(8);
  else if (n <= 16) CE_SOFT(16);
  else CE_SOFT(32);
#undef CE_SOFT
  return MEMHIP_OK;
}

// ---------------------------------------------------------------- weight EMA
// ema = decay * ema + (1 - decay) * p: 8 B read + 4 B written per value, nothing re-read.
__global__ __launch_bounds__(kT) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long long n,
                                                 float decay, float one_minus) {
  const long long n4 = n >> 2;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4* e4 = reinterpret_cast<f32x4*>(ema);
  const f32x4* p4 = reinterpret_cast<const f32x4*>(p);
  const long long t0 = (long long)blockIdx.x * kT + threadIdx.x, stride = (long long)gridDim.x * kT;
  for (long long i = t0; i < n4; i += stride) {
    f32x4 e = __builtin_nontemporal_load(e4 + i);
    const f32x4 q = __builtin_nontemporal_load(p4 + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = decay * e[k] + one_minus * q[k];
    e4[i] = e;
  }
  for (long long i = (n4 << 2) + t0; i < n; i += stride) ema[i] = decay * ema[i] + one_minus * p[i];
}

int grid_for(long long items) {       // memory-bound grid: enough workgroups to fill the chip, the rest by stride
  const long long b = (items + kT - 1) / kT;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" int memhip_mixup(float* x, int B, int C, int H, int W, const float* lam, const int32_t* box,
                            const float* lam_host, const int32_t* box_host, memhip_stream_t stream) {
  MEMHIP_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "mixup: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
  for (int i = 0; (lam_host || box_host) && i < B; ++i) {
    if (lam_host) MEMHIP_REQUIRE(lam_host[i] >= 0.f && lam_host[i] <= 1.f, "mixup: lam[%d] = %g outside [0, 1]", i, lam_host[i]);
    if (box_host) {
      const int32_t* b = box_host + 4 * i;
      MEMHIP_REQUIRE(0 <= b[0] && b[0] <= b[1] && b[1] <= H && 0 <= b[2] && b[2] <= b[3] && b[3] <= W,
                     "mixup: bad box[%d] = (yl %d, yh %d, xl %d, xh %d) for H=%d W=%d", i, b[0], b[1], b[2], b[3], H, W);
    }
  }
  MEMHIP_REQUIRE(x && lam && box, "mixup: null pointer");
  const long long n = (long long)C * H * W;
  const int pairs = (B + 1) / 2;
  const bool vec = n % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const long long items = vec ? n / 4 : n;
  int bx = grid_for(items);
  const int cap = 4096 / pairs > 8 ? 4096 / pairs : 8;      // ~4096 workgroups over all pairs
  if (bx > cap) bx = cap;
  if (vec)
    hipLaunchKernelGGL(mixup_kernel<4>, dim3(bx, pairs), dim3(kT), 0, as_stream(stream), x, B, n, H, W, lam, box);
  else
    hipLaunchKernelGGL(mixup_kernel<1>, dim3(bx, pairs), dim3(kT), 0, as_stream(stream), x, B, n, H, W, lam, box);
  return check_launch("mixup");
}

extern "C" int memhip_mix_targets(const int64_t* labels, const float* lam, int B, int V, double smoothing, float* t,
                                  int64_t ldt, memhip_stream_t stream) {
  MEMHIP_REQUIRE(B > 0 && V >= 2 && ldt >= V, "mix_targets: bad shape B=%d V=%d ldt=%lld", B, V, (long long)ldt);
  MEMHIP_REQUIRE(smoothing >= 0.0 && smoothing <= 1.0, "mix_targets: smoothing %g outside [0, 1]", smoothing);
  MEMHIP_REQUIRE(labels && lam && t, "mix_targets: null pointer");
  const double off = smoothing / V, on = 1.0 - smoothing + off;      // timm: Python floats, then fp32 tensors
  hipLaunchKernelGGL(mix_targets_kernel, dim3(B), dim3(kT), 0, as_stream(stream), (const long long*)labels, lam, B, V, on,
                     off, t, (long long)ldt);
  return check_launch("mix_targets");
}

extern "C" int memhip_ce_soft(const void* logits, int logits_f32, int64_t ld, const float* target, int64_t ldt,
                              const int64_t* labels, float smoothing, int M, int V, float grad_scale, void* dlogits,
                              int64_t lddl, float* row_loss, int32_t* row_correct, int write_grad, float* out2,
                              memhip_stream_t stream) {
  MEMHIP_REQUIRE(M > 0 && V >= 2 && V <= kT * 32, "ce_soft: bad shape M=%d V=%d (2 <= V <= %d)", M, V, kT * 32);
  MEMHIP_REQUIRE(ld >= V, "ce_soft: ld=%lld < V=%d", (long long)ld, V);
  MEMHIP_REQUIRE(logits && row_loss && row_correct && out2, "ce_soft: null pointer");
  MEMHIP_REQUIRE((target != nullptr) != (labels != nullptr), "ce_soft: give dense targets or hard labels, not both or neither");
  MEMHIP_REQUIRE(!target || ldt >= V, "ce_soft: ldt=%lld < V=%d", (long long)ldt, V);
  MEMHIP_REQUIRE(target || (smoothing >= 0.f && smoothing < 1.f), "ce_soft: smoothing %g outside [0, 1)", smoothing);
  MEMHIP_REQUIRE(!write_grad || (dlogits && lddl >= V), "ce_soft: write_grad needs dlogits with lddl >= V");
  hipStream_t s = as_stream(stream);
  if (target) smoothing = 0.f;
  if (logits_f32)
    ce_soft_launch<float>(logits, ld, target, ldt, labels, smoothing, M, V, grad_scale, dlogits, lddl, row_loss,
                          row_correct, write_grad, s);
  else
    ce_soft_launch<__bf16>(logits, ld, target, ldt, labels, smoothing, M, V, grad_scale, dlogits, lddl, row_loss,
                           row_correct, write_grad, s);
  hipLaunchKernelGGL(ce_soft_reduce_kernel, dim3(1), dim3(kT), 0, s, row_loss, row_correct, M, out2);
  return check_launch("ce_soft");
}

extern "C" int memhip_ema_update(float* ema, const float* p, int64_t n, double decay, memhip_stream_t stream) {
  MEMHIP_REQUIRE(n > 0, "ema_update: n=%lld", (long long)n);
  MEMHIP_REQUIRE(ema && p, "ema_update: null pointer");
  MEMHIP_REQUIRE(decay >= 0.0 && decay <= 1.0, "ema_update: decay %g outside [0, 1]", decay);
  MEMHIP_REQUIRE(((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(p)) & 15) == 0,
                 "ema_update: buffers must be 16-byte aligned");
  // timm: ema * decay + (1. - decay) * p on fp32 tensors -- both Python scalars are rounded to fp32 on their own (1 - decay
  // formed in fp32 would be off by 1.7e-4 of itself at decay 0.9999)
  hipLaunchKernelGGL(ema_kernel, dim3(grid_for((n + 3) / 4)), dim3(kT), 0, as_stream(stream), ema, p, (long long)n,
                     (float)decay, (float)(1.0 - decay));
  return check_launch("ema_update");
}
