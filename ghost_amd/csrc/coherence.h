// coherence.h -- binned cross-spectra of channel pairs from a resident complex result (include/ghostcwt.h:
// gcwt_coherence).  coherence.cpp cuts a pair list into tile-pair tasks on the host; coherence.hip runs them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace gcwt {

constexpr int kCohTile = 8;                       // channels per tile: a task works on kCohTile x kCohTile cells
constexpr int kCohCells = kCohTile * kCohTile;

// One (tile A, tile B) of the pair list, tile_a <= tile_b.  Cell (i, j) = i * kCohTile + j accumulates
// sum W[A i] conj(W[B j]); in a diagonal task (tile_a == tile_b) only cells i < j are used.
struct CohTask {
  int32_t tile_a, tile_b;
  int32_t flags;               // bit 0: this task writes the power rows of tile A's channels; bit 1: of tile B's
  int32_t entry_first, n_entries;
  uint32_t rows_a, rows_b;     // rows of the tiles the task reads (wanted cells, and every channel whose power it writes)
  uint64_t cells;              // wanted cells
};
// An output row of a task: pair `out_row` of the caller's list is cell `cell`, conjugated when the pair was asked
// for as (channel of tile B, channel of tile A) -- or as (j, i), i < j, of a diagonal task.
struct CohEntry {
  int32_t cell, conjugate, out_row;
};

// Host only.  Tasks in order of (tile_a, tile_b): those with entries first -- none of them empty, each tile pair
// once --, then one entry-less task (t, t) for every tile that no pair touches, so that each tile's power is written
// by exactly one task.
void coherence_tasks(int32_t n_channels, const int32_t* pairs, int32_t n_pairs, std::vector<CohTask>* tasks,
                     std::vector<CohEntry>* entries);

struct CohArgs {
  const float2* rows;          // [channel][scale] rows, pitch complex elements apart
  int64_t pitch, n_cols, window, n_bins, out_pitch, run_bins, n_runs;
  int32_t n_channels, n_scales, n_tasks;
  const CohTask* tasks;        // device copies
  const CohEntry* entries;
  float* power;                // [C][S][out_pitch] or NULL
  float2* cross;               // [P][S][out_pitch] or NULL
  float* coherence;            // [P][S][out_pitch] or NULL
};
hipError_t launch_coherence(const CohArgs& a, hipStream_t st);

}  // namespace gcwt
