// bandpass.h -- band-limited analytic signals from the rows of a resident complex result (include/ghostcwt.h:
// gcwt_bandpass).  bandpass.cpp checks the arguments, copies the band table and the weights and sizes the grid;
// bandpass.hip does the work.  The tiles are regular -- kBpCols columns counted from column 0 x kBpBands consecutive
// bands of the list -- so a workgroup finds its tile from its index and there is no task list.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resident_op.h"

namespace gcwt {

constexpr int kBpThreads = 256;                   // four waves, each on its own columns (they never meet)
constexpr int kBpLaneCols = 2;                    // adjacent columns of a lane: one 16-byte load per row
constexpr int kBpCols = kBpThreads * kBpLaneCols; // columns per tile
constexpr int kBpBands = 4;                       // bands per group: a row the group's bands share is read once

struct BpArgs {
  const float2* rows;          // [channel][scale] rows, pitch complex elements apart
  const int2* bands;           // device copy of the band list: (first row, rows)
  const float* g;              // device copy: n_scales weights of the analytic sum ...
  const float* h;              // ... and n_scales of the power sum, right behind (zeros where the host gave none)
  int64_t pitch, n_cols, out_pitch, n_ctiles, n_units;   // n_units = n_channels * n_ctiles
  int32_t n_channels, n_scales, n_bands, n_groups;
  int32_t aligned;             // every row and output row starts on 16 bytes: two columns move as one vector
  float2* analytic;            // [C][n_bands][out_pitch] or NULL
  float* envelope;             // [C][n_bands][out_pitch] or NULL
  float* power;                // [C][n_bands][out_pitch] or NULL
};
// workgroups of the grid: the band groups of a unit share its columns (resident_op.h: the placement)
inline int64_t bandpass_blocks(const BpArgs& a) { return shared_blocks(a.n_units, a.n_groups); }
hipError_t launch_bandpass(const BpArgs& a, hipStream_t st);

}  // namespace gcwt
