// Which kernels take a memhip_rasterize call, with which bands, grids, LDS bytes, workspace layout and clears: raster_plan
// (raster_plan.cpp) is the one place that reads a memhip_raster_args_t, accepts or rejects it and decides the dispatch -- once
// per call, from the struct, the device's CU count and a snapshot of the options.  Host arithmetic only: memhip_rasterize_plan
// takes the struct of the call and returns the same plan without a device (tests/test_raster_plan_cpu.py checks it against the
// launchers it replaced).  The constants below are read by the kernels (raster.hip) and by the plan alike.
#pragma once
#include <cstdint>
#include "../../include/memhip.h"

namespace memhip {
namespace raster {

// ---- global-atomic kernels (raster_count / raster_finalize) and the extent kernels
constexpr int kThreads = 256;
constexpr int kEvPerThread = 8;

// ---- privatised counters (raster_lds_kernel)
constexpr int kLdsThreads = 1024;
constexpr int kBandPixels = 14336;            // 2 polarities x 14336 x 4 B = 112 KiB of LDS
constexpr int kMaxBands = 6;

// ---- two-pass binned kernels (raster_bin_keys / raster_bin_accum)
constexpr int kBinThreads = 512;
constexpr int kBinEvPerThread = 8;
constexpr int kBinChunk = kBinThreads * kBinEvPerThread;   // 4096 events
constexpr int kBinParts = 2;                               // the next chunk is requested in this many parts (4: the same, 8: 5 % slower)
constexpr int kBinMaxBands = 64;
constexpr int kBinBandPixels = 40000;                      // pixels of a band: 16-bit key (0xFFFF is the pad key), 160 000 B of LDS counters in pass 2
constexpr int kBinSegs = 2 * kBinMaxBands;                 // a chunk's keys are sorted by (band, polarity): two segments per band
constexpr int kBinHdr = kBinSegs + 1;                      // segment boundaries of a chunk
constexpr int kBinSlots = kBinChunk + 8 * kBinSegs;        // key slots of a chunk: events + padding of every segment to 8
constexpr int kAccThreads = 1024;
constexpr int kBinKeyGrid = 4096;                           // pass-1 workgroups in all (rounded up to whole samples)
constexpr int kBinOverflow = 1 << 30;                      // status flag: n_events smaller than the offsets say

}  // namespace raster

// the options the plan reads, taken once per call
struct RasterOptions { int raster_lds, raster_bands; };

// Validates *a like the call (query: a pointer may be null, and workspace_bytes is compared only when there is a workspace)
// and fills *p.  device_cus: the CUs the band model of the binned form plans for; < 0: max_cus(), asked only when that model
// runs; a device that reports none counts as 256, as the model always assumed.
int raster_plan(const memhip_raster_args_t* a, bool query, const RasterOptions& o, int device_cus, memhip_raster_plan_t* p);

}  // namespace memhip
