// The host side of memhip_seg_predict: the one place that reads a memhip_segpredict_args_t, accepts or rejects it, checks that
// the views cover the canvas and sizes the launch; the launcher (seg_predict.hip) obeys.  Host integer arithmetic only:
// memhip_seg_predict_plan runs without a device (tests/test_seg_infer_cpu.py).
#pragma once
#include <cstdint>
#include "../../include/memhip.h"

namespace memhip {
namespace segp {

constexpr int kThreads = 256;
constexpr int kPx = 4;                         // consecutive x per thread: pred leaves as one dword
constexpr int kLanesX = 16;                    // threads along x
constexpr int kTileW = kLanesX * kPx;          // 64
constexpr int kTileH = kThreads / kLanesX;     // 16
constexpr int kMaxViews = 64;

}  // namespace segp

// query: the device pointers of logits and tables may be NULL.  passes: bit f is set when a view with flip = f is present.
int seg_predict_plan(const memhip_segpredict_args_t* a, bool query, memhip_segpredict_plan_t* p, int* passes);

}  // namespace memhip
