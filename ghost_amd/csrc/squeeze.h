// squeeze.h -- the synchrosqueezed transform of a run of rows of a resident complex result (include/ghostcwt.h:
// gcwt_squeeze).  squeeze.cpp checks the arguments, copies the tables and sizes the grid; squeeze.hip does the work.  The
// tiles are regular: kSqCols columns counted from column 0 x kSqCells consecutive output rows counted from row 0, so a
// workgroup finds its tile from its index and there is no task list.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resident_op.h"

namespace gcwt {

constexpr int kSqThreads = 256;                   // four waves, each on its own columns (they never meet)
constexpr int kSqLaneCols = 2;                    // adjacent columns of a lane: one 16-byte load per row
constexpr int kSqCols = kSqThreads * kSqLaneCols; // columns per tile
constexpr int kSqCells = 16;                      // output rows per group: 16 x 512 float2 = 64 KiB of LDS, two workgroups per CU
constexpr int kSqMaxCells = 4096;

struct SqArgs {
  const float2* rows;          // [channel][scale] rows, pitch complex elements apart
  const float* g;              // device copy: n_scales weights of the sum ...
  const float* floor2;         // ... n_scales thresholds on |w|^2 ...
  const float* nu;             // ... and n_scales expected phase advances, one behind the other
  const float* edges;          // device copy: n_cells + 1 cell edges, ascending
  const longlong2* segments;   // device copy: (start, stop), ascending, each starting where the one before stops
  int64_t pitch, n_cols, out_pitch, n_ctiles, n_units, n_segments;   // n_units = n_channels * n_ctiles
  int32_t n_channels, n_scales, first, count, n_cells, n_groups;
  int32_t descending;          // output row of cell l: n_cells - 1 - l, else l
  int32_t aligned;             // every row and output row starts on 16 bytes: two columns move as one vector
  float hz_per_cycle;
  float2* coefficients;        // [C][n_cells][out_pitch] or NULL
  float* power;                // [C][n_cells][out_pitch] or NULL
  float* frequency;            // [C][count][out_pitch] or NULL
  int32_t* index;              // [C][count][out_pitch] or NULL
};
// workgroups of the grid: the cell groups of a unit share its columns (resident_op.h: the placement)
inline int64_t squeeze_blocks(const SqArgs& a) { return shared_blocks(a.n_units, a.n_groups); }
hipError_t launch_squeeze(const SqArgs& a, hipStream_t st);

}  // namespace gcwt
