// coupling.cpp -- the host side of gcwt_coupling (include/ghostcwt.h): argument checks, the grid (coupling.h: regular
// tiles, no task list), the launch (coupling.hip).  Plan-independent, like gcwt_coherence.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ghostcwt_debug.h"
#include "coupling.h"
#include "errors.h"
#include "resident_op.h"

static_assert(gcwt::kCplPhase == GCWT_COUPLING_TILE_PHASE && gcwt::kCplAmp == GCWT_COUPLING_TILE_AMP,
              "ghostcwt_debug.h names the tile the kernel is built for");

using namespace gcwt;

namespace {

constexpr const char* kOp = "gcwt_coupling";

// everything that needs no device; fills the grid's numbers
int check_and_cut(int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols, int32_t phase_first,
                  int32_t n_phase, int32_t amp_first, int32_t n_amp, int64_t window, gcwt::CplArgs* a) {
  int rc = check_channels(kOp, n_channels);
  if (!rc) rc = check_rows(kOp, n_scales, n_cols, pitch);
  if (!rc) rc = check_window(kOp, window);
  if (!rc) rc = check_row_range(kOp, "phase rows", phase_first, n_phase, n_scales);
  if (!rc) rc = check_row_range(kOp, "amplitude rows", amp_first, n_amp, n_scales);
  if (rc) return rc;
  a->pitch = pitch; a->n_cols = n_cols; a->window = window;
  a->n_bins = (n_cols + window - 1) / window;
  a->n_channels = n_channels; a->n_scales = n_scales;
  a->phase_first = phase_first; a->n_phase = n_phase; a->amp_first = amp_first; a->n_amp = n_amp;
  a->n_ptiles = (n_phase + gcwt::kCplPhase - 1) / gcwt::kCplPhase;
  a->n_atiles = (n_amp + gcwt::kCplAmp - 1) / gcwt::kCplAmp;
  // a workgroup's run of bins: about 2048 columns for each of its four waves -- short, so that the tiles of one
  // (channel, run) stay close together on the rows they share --, fewer runs where the grid would not fit
  a->run_bins = 4 * std::max<int64_t>(1, (2048 + window - 1) / window);
  for (;; a->run_bins *= 2) {
    a->n_runs = (a->n_bins + a->run_bins - 1) / a->run_bins;
    a->n_units = a->n_runs * n_channels;
    if (gcwt::coupling_blocks(*a) <= 0x7fffffff) break;
  }
  return GCWT_OK;
}

}  // namespace

extern "C" {

int gcwt_debug_coupling_grid(int32_t n_channels, int64_t n_cols, int32_t n_phase, int32_t n_amp, int64_t window,
                             int32_t* n_phase_tiles, int32_t* n_amp_tiles, int64_t* run_bins, int64_t* n_runs,
                             int64_t* n_blocks) {
  return guarded([&] {
    gcwt::CplArgs a{};
    const int32_t n_scales = std::max(n_phase, n_amp);
    const int rc = check_and_cut(n_cols, n_channels, n_scales, n_cols, 0, n_phase, 0, n_amp, window, &a);
    if (rc) return rc;
    if (n_phase_tiles) *n_phase_tiles = a.n_ptiles;
    if (n_amp_tiles) *n_amp_tiles = a.n_atiles;
    if (run_bins) *run_bins = a.run_bins;
    if (n_runs) *n_runs = a.n_runs;
    if (n_blocks) *n_blocks = gcwt::coupling_blocks(a);
    return (int)GCWT_OK;
  });
}

int gcwt_coupling(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                  int32_t phase_first, int32_t n_phase, int32_t amp_first, int32_t n_amp, int64_t window,
                  float* d_vector, float* d_mvl, float* d_amplitude, int64_t out_pitch) {
  return guarded([&] {
    if (!d_rows) return fail(GCWT_ERR_INVALID, "gcwt_coupling: d_rows is NULL");
    gcwt::CplArgs a{};
    int rc = check_and_cut(pitch, n_channels, n_scales, n_cols, phase_first, n_phase, amp_first, n_amp, window, &a);
    if (rc) return rc;
    if (!d_vector && !d_mvl && !d_amplitude) return fail(GCWT_ERR_INVALID, "gcwt_coupling: nothing to compute (no output)");
    if (out_pitch < a.n_bins) return fail(GCWT_ERR_INVALID, "gcwt_coupling: out_pitch is below the number of bins, ceil(n_cols / window)");

    rc = resolve_device(kOp, d_rows, {d_vector, d_mvl, d_amplitude});
    if (rc) return rc;

    a.rows = reinterpret_cast<const float2*>(d_rows);
    a.out_pitch = out_pitch;
    a.vector = reinterpret_cast<float2*>(d_vector); a.mvl = d_mvl; a.amplitude = d_amplitude;
    return finish(kOp, gcwt::launch_coupling(a, nullptr));
  });
}

}  // extern "C"
