// trace_smooth.h -- a symmetric FIR along float32 traces on the device, inside segments, with an optional mean over
// traces first (include/ghostcwt.h: gcwt_trace_smooth has the definition; profiles/smooth.md).  trace_smooth.cpp checks
// the arguments, copies the taps, the segments and the members and sizes the grid; trace_smooth.hip does the work.  The
// tiles are regular -- kSmCols columns counted from column 0, the tiles of detect_runs.h -- so a workgroup finds its
// (output trace, tile) from its index: unit = trace * n_tiles + tile.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "detect_runs.h"

namespace gcwt {

constexpr int kSmThreads = 256;                      // four waves
constexpr int kSmLaneCols = 4;                       // adjacent outputs of a lane: one 16-byte LDS read moves a window by as many
constexpr int kSmCols = kSmThreads * kSmLaneCols;    // columns per tile
constexpr int kSmMaxHalf = 4096;                     // GCWT_SMOOTH_MAX_HALF: (kSmCols + 2 * 4096) floats of LDS = 36 KB
static_assert(kSmCols == kRunCols, "TraceArgs::n_tiles counts these tiles");
static_assert(kSmMaxHalf % kSmLaneCols == 0, "the halo is staged in whole 16-byte groups");

struct SmoothArgs {
  TraceArgs t;                 // the input traces; t.n_tiles tiles per trace
  const float* taps;           // device copy: w_1 .. w_half, then zeros up to a multiple of 4 (never used)
  float w0;
  int32_t half;
  int32_t halo;                // half rounded up to a multiple of kSmLaneCols: the columns staged on either side of a tile
  const longlong2* segments;   // device copy: n_segments (start, stop), ascending and disjoint
  int64_t n_segments;          // >= 1
  const int32_t* members;      // device copy: n_members traces to average, or NULL
  int32_t n_members;
  float inv_members;           // (float)(1.0 / n_members)
  int64_t n_out;               // output traces: 1 with members, else t.n_traces
  float* out;
  int64_t out_pitch;
  int32_t out_aligned;         // every output row starts on 16 bytes
};

inline size_t smooth_lds_bytes(const SmoothArgs& a) { return (size_t)(kSmCols + 2 * a.halo) * sizeof(float); }

hipError_t launch_trace_smooth(const SmoothArgs& a, hipStream_t st);

}  // namespace gcwt
