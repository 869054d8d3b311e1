// Which kernel form, how many row slices and which part of the workspace every product of a weight-gradient call gets:
// tn_plan (gemm_tn_plan.cpp) is the one place that decides, once per call, for memhip_gemm_bf16_tn / _tn_group
// and for the two workspace queries.  Host arithmetic only: memhip_gemm_bf16_tn_plan returns the same plan without a
// device (tests/test_tn_plan_cpu.py pins it to the launchers it replaced).
#pragma once
#include <cstddef>
#include "../../include/memhip.h"

namespace memhip {

// ---- the tiles of the two kernels (gemm_tn.hip, gemm_tn_p8.hip use these)
constexpr int kTn128Tile = 128;      // gemm_tn_kernel: 128 x 128 outputs per workgroup
constexpr int kTnP8Tile = 256;       // gemm_tn_p8_kernel: 256 x 256
constexpr int kTnStageRows = 64;     // token rows per stage (K-tile) of both; the p8 kernel advances by pairs of them
constexpr int kTnMinRows = 2048;     // below this the p8 kernel does not pay
constexpr int kTnGroupMax = 4;       // products per grouped launch (memhip_tn_launch_t::p)

// the plan is the ABI's memhip_tn_plan_t: kinds MEMHIP_TN_*
typedef memhip_tn_part_t TnPart;
typedef memhip_tn_launch_t TnLaunch;
typedef memhip_tn_plan_t TnPlan;

struct TnOptions { int tn_p8, tn_group; };                    // taken once per call
struct TnWorkspace { bool present, aligned; size_t bytes; };  // what the plan may know of the caller's workspace
struct TnSlices { int rows_per_split, splits; };

// the 256 x 256 kernel has no column guard and wants a main loop worth its prologue
inline bool tn_p8_fits(int R, int N, int K) {
  return N > 0 && K > 0 && N % kTnP8Tile == 0 && K % kTnP8Tile == 0 && R >= kTnMinRows;
}
// `wanted` row slices of R rows (R > 0).  p8 kernel: whole pairs of K-tiles, at least 256 rows per slice; 128 x 128 kernel:
// whole K-tiles, at least 4 of them (256 rows) per slice.  The count that comes back leaves no slice empty.
TnSlices tn_p8_slices(int R, int wanted);
TnSlices tn_128_slices(int R, int wanted);

// stream_cus: usable_cus(stream), the CUs the p8 forms fill (0: no p8 form).  count 1..kTnGroupMax, shapes validated.
TnPlan tn_plan(const memhip_tn_problem_t* pr, int count, int accumulate, const TnWorkspace& ws, int stream_cus,
               const TnOptions& o);

// Workspace bytes with which no plan of these products takes an atomic form for want of space, on a device of
// device_cus CUs: the maximum over the CU counts a stream can be left with (device_cus ... 8, step 8).
size_t tn_workspace_bytes(int R, int N, int K, int device_cus);                                     // one product
size_t tn_group_workspace_bytes(const memhip_tn_problem_t* pr, int count, int device_cus);         // the group, and each alone

}  // namespace memhip
