// coupling_surrogates.h -- shift-surrogate statistics of gcwt_coupling's mean vector length (include/ghostcwt.h:
// gcwt_coupling_surrogates).  coupling_surrogates.cpp checks the arguments and sizes the grid; coupling_surrogates.hip
// does the work.  The tiles are coupling.h's -- kSurPhase phase rows x kSurAmp amplitude rows, counted from the first row
// of each range --, a workgroup takes one (channel, bin, tile) and holds the bin in LDS, so the bin has a largest length.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resident_op.h"

namespace gcwt {

constexpr int kSurPhase = 4;                      // phase rows per tile
constexpr int kSurAmp = 8;                        // amplitude rows per tile
constexpr int kSurCells = kSurPhase * kSurAmp;    // cell (i, j) = i * kSurAmp + j: one lane each when a shift is judged
constexpr int kSurWaves = 8;                      // per workgroup: two per SIMD, up to 256 registers each
constexpr int kSurMaxWindow = 2048;               // GCWT_COUPLING_SURROGATES_MAX_WINDOW
constexpr int kSurMaxShifts = 4096;
// LDS of a bin of `window` columns: u (8 B) of each phase row and |w| (4 B) of each amplitude row per column, the planes
// padded to whole 16 bytes; then per wave its reduced sums (re, im per cell) and its partial T, Q and count per cell;
// then S per amplitude row and mvl_0 per cell.
constexpr int kSurColBytes = 8 * kSurPhase + 4 * kSurAmp;
constexpr int kSurWaveBytes = 2 * kSurCells * 4 + kSurCells * (8 + 8 + 4);
constexpr int kSurTailBytes = kSurWaves * kSurWaveBytes + (kSurAmp + kSurCells) * 4;
constexpr int64_t surrogates_plane_cols(int64_t window) { return (window + 3) & ~int64_t(3); }
constexpr int64_t surrogates_lds_bytes(int64_t window) { return surrogates_plane_cols(window) * kSurColBytes + kSurTailBytes; }
static_assert(kSurTailBytes % 16 == 0 && kSurMaxWindow * kSurColBytes + kSurTailBytes <= 160 * 1024,
              "the largest bin and the waves' sums fit in a CU's LDS");

struct SurArgs {
  const float2* rows;          // [channel][scale] rows, pitch complex elements apart
  const int32_t* shifts;       // [n_shifts], device memory, each in [0, window)
  int64_t pitch, n_cols, window, n_bins, out_pitch, n_units;   // n_units = n_channels * n_bins
  int32_t n_channels, n_scales, phase_first, n_phase, amp_first, n_amp, n_ptiles, n_atiles, n_shifts;
  float* mean;                 // [C][P][A][out_pitch] or NULL
  float* sd;                   // [C][P][A][out_pitch] or NULL
  int32_t* count_ge;           // [C][P][A][out_pitch] or NULL
  float* surrogates;           // [K][C][P][A][out_pitch] or NULL
};
// workgroups of the grid: the tiles of a unit share its rows (resident_op.h: the placement)
inline int64_t surrogates_blocks(const SurArgs& a) { return shared_blocks(a.n_units, (int64_t)a.n_ptiles * a.n_atiles); }
// asks for the kernel's LDS (above the 64 KiB a kernel gets by default) and launches
hipError_t launch_coupling_surrogates(const SurArgs& a, hipStream_t st);

}  // namespace gcwt
