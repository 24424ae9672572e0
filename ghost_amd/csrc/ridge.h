// ridge.h -- the spectral ridge of a band of a resident complex result and the instantaneous frequency on it
// (include/ghostcwt.h: gcwt_ridge).  ridge.cpp checks the arguments, copies the band table, the weights and the segment
// table and sizes the grid; ridge.hip does the work.  The tiles are bandpass.h's: kRgCols columns counted from column 0 x
// kRgBands consecutive bands of the list, so a workgroup finds its tile from its index and there is no task list.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resident_op.h"

namespace gcwt {

constexpr int kRgThreads = 256;                   // four waves, each on its own columns (they never meet)
constexpr int kRgLaneCols = 2;                    // adjacent columns of a lane: one 16-byte load per row
constexpr int kRgCols = kRgThreads * kRgLaneCols; // columns per tile
constexpr int kRgBands = 4;                       // bands per group: a row the group's bands share is read once

struct RgArgs {
  const float2* rows;          // [channel][scale] rows, pitch complex elements apart
  const int2* bands;           // device copy of the band list: (first row, rows)
  const float* e;              // device copy: n_scales weights of the ranking ...
  const float* nu;             // ... and n_scales expected phase advances, right behind
  const longlong2* segments;   // device copy: (start, stop), ascending, each starting where the one before stops
  int64_t pitch, n_cols, out_pitch, n_ctiles, n_units, n_segments;   // n_units = n_channels * n_ctiles
  int32_t n_channels, n_scales, n_bands, n_groups;
  int32_t aligned;             // every row and output row starts on 16 bytes: two columns move as one vector
  float hz_per_cycle;
  int32_t* row;                // [C][n_bands][out_pitch] or NULL
  float* amplitude;            // [C][n_bands][out_pitch] or NULL
  float* offset;               // [C][n_bands][out_pitch] or NULL
  float* frequency;            // [C][n_bands][out_pitch] or NULL
};
// workgroups of the grid: the band groups of a unit share its columns (resident_op.h: the placement)
inline int64_t ridge_blocks(const RgArgs& a) { return shared_blocks(a.n_units, a.n_groups); }
hipError_t launch_ridge(const RgArgs& a, hipStream_t st);

}  // namespace gcwt
