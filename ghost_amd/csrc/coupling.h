// coupling.h -- binned phase-amplitude coupling inside the channels of a resident complex result (include/ghostcwt.h:
// gcwt_coupling).  coupling.cpp checks the arguments and sizes the grid; coupling.hip does the work.  The tiles are
// regular -- kCplPhase phase rows x kCplAmp amplitude rows, counted from the first row of each range -- so a workgroup
// finds its tile from its index and there is no task list.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resident_op.h"

namespace gcwt {

constexpr int kCplPhase = 4;                      // phase rows per tile
constexpr int kCplAmp = 8;                        // amplitude rows per tile
constexpr int kCplCells = kCplPhase * kCplAmp;    // cell (i, j) = i * kCplAmp + j: 64 accumulators (re, im) and 8 for S

struct CplArgs {
  const float2* rows;          // [channel][scale] rows, pitch complex elements apart
  int64_t pitch, n_cols, window, n_bins, out_pitch, run_bins, n_runs, n_units;   // n_units = n_channels * n_runs
  int32_t n_channels, n_scales, phase_first, n_phase, amp_first, n_amp, n_ptiles, n_atiles;
  float2* vector;              // [C][P][A][out_pitch] or NULL
  float* mvl;                  // [C][P][A][out_pitch] or NULL
  float* amplitude;            // [C][A][out_pitch] or NULL
};
// workgroups of the grid: the tiles of a unit share its rows (resident_op.h: the placement)
inline int64_t coupling_blocks(const CplArgs& a) { return shared_blocks(a.n_units, (int64_t)a.n_ptiles * a.n_atiles); }
hipError_t launch_coupling(const CplArgs& a, hipStream_t st);

}  // namespace gcwt
