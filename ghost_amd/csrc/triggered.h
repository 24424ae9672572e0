// triggered.h -- event-locked averages of the rows of a resident complex result (include/ghostcwt.h: gcwt_triggered).
// triggered.cpp checks the arguments, copies the event list and sizes the grid; triggered.hip does the work.  The tiles
// are regular -- kTrgRows rows counted from the first row asked for x kTrgLags lags counted from lag 0 -- so a
// workgroup finds its tile from its index and there is no task list.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resident_op.h"

namespace gcwt {

constexpr int kTrgRows = 4;                       // rows per tile: one per wave when the chains are combined
constexpr int kTrgLags = 64;                      // lags per tile: lane = lag
constexpr int kTrgChains = 4;                     // interleaved chains of a sum: chain j adds events j, j + 4, ...

struct TrgArgs {
  const float2* rows;          // [channel][scale] rows, pitch complex elements apart
  const int64_t* events;       // device copy of the event columns, in the order given
  int64_t pitch, n_events, before, n_lags, out_pitch, n_ltiles, n_units;   // n_units = n_channels * n_ltiles
  int32_t n_channels, n_scales, row_first, n_rows, n_rtiles;
  float* amplitude;            // [C][n_rows][out_pitch] or NULL
  float* power;                // [C][n_rows][out_pitch] or NULL
  float2* evoked;              // [C][n_rows][out_pitch] or NULL
  float2* vector;              // [C][n_rows][out_pitch] or NULL
  float* itpc;                 // [C][n_rows][out_pitch] or NULL
};
// workgroups of the grid: the row tiles of a unit share its columns (resident_op.h: the placement)
inline int64_t triggered_blocks(const TrgArgs& a) { return shared_blocks(a.n_units, a.n_rtiles); }
hipError_t launch_triggered(const TrgArgs& a, hipStream_t st);

}  // namespace gcwt
