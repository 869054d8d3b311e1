// Which kernel takes which rows of a memhip_gemm_bf16_nt product: gemm_nt_plan (gemm_nt_plan.cpp) is the one place that
// decides, once per call, from shapes, leading dimensions, CU counts and a snapshot of the options.  Host arithmetic only:
// memhip_gemm_bf16_nt_plan returns the same plan without a device (tests/test_gemm_plan_cpu.py checks the table).
#pragma once
#include "../../include/memhip.h"

namespace memhip {

struct GemmArgs {   // memhip_gemm_args_t, followed by launcher-internal fields
  const __bf16* A; const __bf16* B;
  long long lda, ldb;
  int M, N, K, epilogue;
  void* out0; long long ldo0;
  void* out1; long long ldo1;
  const float* bias;
  const float* vec1;
  float* resid; long long ldr;
  const void* aux; long long ldaux;
  const float* rowmask;
  float keep_prob;
  float colscale; int colscale_n;
  int rows_per_sample;
  int accumulate;
  float* colsum;   // optional: += column sums of the (rounded) primary output
  const int* sample_map;   // RESIDUAL: compact sample -> sample whose residual rows this output row updates (NULL: identity)
  int colsum_copies;       // > 1: colsum holds that many accumulator copies of N floats; a workgroup uses copy blockIdx % copies
  int reserved0;
  // ---- internal (not part of the C ABI; zero when the struct is copied from memhip_gemm_args_t)
  int m_base;      // row offset of this launch inside the caller's problem (a GEMM may be launched in two
                   // row ranges): only the per-sample row mask index needs the absolute row
};

// The plan is the ABI's memhip_nt_plan_t: kinds MEMHIP_NT_*, rows [row0, row0 + rows) per launch.  `grid`, `guard` and
// `copy` are the grid and the template choices of the launch (a MEMHIP_NT_P8_PAIR launch runs grid + tail_grid workgroups).
typedef memhip_nt_launch_t NtLaunch;
typedef memhip_nt_plan_t NtPlan;

// the options the plan reads, taken once per call (gemm_stagger / gemm_prefetch are launch arguments, read by the launchers)
struct NtOptions { int gemm_p8, gemm256, gemm_split, gemm_p8_half, gemm_p8_pair, gemm_p8_min_n, gemm256_min_n; };

// ---- the kernel instantiations each form has.  The plan names a form only where its predicate holds, and the launchers
// instantiate exactly these (asked for anything else they fail with MEMHIP_EINVAL).
// COPY of the p8 kernels: the epilogue stores out0.  Only the residual epilogues can do without.
inline bool nt_p8_copy(const GemmArgs& p) {
  return !(p.epilogue == MEMHIP_EPI_RESIDUAL_DROP || (p.epilogue == MEMHIP_EPI_RESIDUAL && !p.out0));
}
// gemm_p8.hip, tile height bmt = 256 / 128.  The 256-row form has no row guard, no residual-dropout epilogue (no room for
// the Philox state beside its hand-counted row loads) and no bf16 branch copy beside the residual epilogue (it spills).
constexpr bool nt_p8_has(int epi, int bmt, bool guard, bool copy) {
  if (epi == MEMHIP_EPI_PATCH_EMBED || (bmt == 256 && guard)) return false;
  if (epi == MEMHIP_EPI_RESIDUAL_DROP) return bmt == 128 && !copy;
  if (epi == MEMHIP_EPI_RESIDUAL) return bmt == 128 || !copy;
  return copy;
}
// gemm_p8_pair_kernel: the four epilogues of the step's N = 768 products (the residual one without the branch copy)
constexpr bool nt_pair_has(int epi, bool copy) {
  return (epi == MEMHIP_EPI_BIAS_BF16 || epi == MEMHIP_EPI_RESIDUAL || epi == MEMHIP_EPI_BIAS_GELU_DG ||
          epi == MEMHIP_EPI_MUL_AUX) && copy == (epi != MEMHIP_EPI_RESIDUAL);
}
// gemm256.hip
constexpr bool nt_g256_has(int epi) {
  return epi == MEMHIP_EPI_BIAS_BF16 || epi == MEMHIP_EPI_BIAS_GELU || epi == MEMHIP_EPI_RESIDUAL ||
         epi == MEMHIP_EPI_RESIDUAL_DROP || epi == MEMHIP_EPI_DGELU || epi == MEMHIP_EPI_F32;
}

// stream_cus: usable_cus(stream), the CUs the p8 forms size their grids for (0: no p8 form).
// device_cus: max_cus(): gemm256 sizes its grid for the whole device and ignores reservations (0: no gemm256).
NtPlan gemm_nt_plan(const GemmArgs& p, int stream_cus, int device_cus, const NtOptions& o);

}  // namespace memhip
