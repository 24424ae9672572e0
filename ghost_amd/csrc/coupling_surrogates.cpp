// coupling_surrogates.cpp -- the host side of gcwt_coupling_surrogates (include/ghostcwt.h): argument checks, the grid
// (coupling_surrogates.h: regular tiles, one bin per workgroup), the device copy of the shift list, the launch
// (coupling_surrogates.hip).  Plan-independent, like gcwt_coupling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ghostcwt_debug.h"
#include "coupling_surrogates.h"
#include "errors.h"
#include "resident_op.h"

static_assert(gcwt::kSurPhase == GCWT_COUPLING_SURROGATES_TILE_PHASE && gcwt::kSurAmp == GCWT_COUPLING_SURROGATES_TILE_AMP &&
                  gcwt::kSurWaves == GCWT_COUPLING_SURROGATES_WAVES,
              "ghostcwt_debug.h names the tile the kernel is built for");
static_assert(gcwt::kSurMaxWindow == GCWT_COUPLING_SURROGATES_MAX_WINDOW && gcwt::kSurMaxWindow >= 2048,
              "ghostcwt.h names the limit the kernel is built for");

using namespace gcwt;

namespace {

constexpr const char* kOp = "gcwt_coupling_surrogates";

// everything that needs no device and no shift list; fills the grid's numbers
int check_and_cut(int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols, int32_t phase_first,
                  int32_t n_phase, int32_t amp_first, int32_t n_amp, int64_t window, gcwt::SurArgs* a) {
  int rc = check_channels(kOp, n_channels);
  if (!rc) rc = check_rows(kOp, n_scales, n_cols, pitch);
  if (!rc) rc = check_window(kOp, window);
  if (!rc) rc = check_row_range(kOp, "phase rows", phase_first, n_phase, n_scales);
  if (!rc) rc = check_row_range(kOp, "amplitude rows", amp_first, n_amp, n_scales);
  if (rc) return rc;
  if (window > gcwt::kSurMaxWindow)
    return fail(GCWT_ERR_INVALID, std::string(kOp) + ": window = " + std::to_string(window) +
                                      " is above GCWT_COUPLING_SURROGATES_MAX_WINDOW = " + std::to_string(gcwt::kSurMaxWindow) +
                                      " columns (a bin is held in LDS; an output stride shortens the window)");
  a->pitch = pitch; a->n_cols = n_cols; a->window = window;
  a->n_bins = (n_cols + window - 1) / window;
  a->n_channels = n_channels; a->n_scales = n_scales;
  a->phase_first = phase_first; a->n_phase = n_phase; a->amp_first = amp_first; a->n_amp = n_amp;
  a->n_ptiles = (n_phase + gcwt::kSurPhase - 1) / gcwt::kSurPhase;
  a->n_atiles = (n_amp + gcwt::kSurAmp - 1) / gcwt::kSurAmp;
  // (n_bins <= n_cols / 2 + 1 and n_channels < 2^31: the product fits in 64 bits)
  a->n_units = a->n_bins * n_channels;
  if (a->n_units > 0x7fffffff || gcwt::surrogates_blocks(*a) > 0x7fffffff)
    return fail(GCWT_ERR_INVALID, std::string(kOp) + ": channels x bins x tiles need more than 2^31 - 1 workgroups: fewer rows "
                                                     "or a wider window per call");
  return GCWT_OK;
}

}  // namespace

extern "C" {

int gcwt_debug_coupling_surrogates_grid(int32_t n_channels, int64_t n_cols, int32_t n_phase, int32_t n_amp, int64_t window,
                                        int32_t* n_phase_tiles, int32_t* n_amp_tiles, int64_t* n_blocks, int64_t* lds_bytes) {
  return guarded([&] {
    gcwt::SurArgs a{};
    const int32_t n_scales = std::max(n_phase, n_amp);
    const int rc = check_and_cut(n_cols, n_channels, n_scales, n_cols, 0, n_phase, 0, n_amp, window, &a);
    if (rc) return rc;
    if (n_phase_tiles) *n_phase_tiles = a.n_ptiles;
    if (n_amp_tiles) *n_amp_tiles = a.n_atiles;
    if (n_blocks) *n_blocks = gcwt::surrogates_blocks(a);
    if (lds_bytes) *lds_bytes = gcwt::surrogates_lds_bytes(window);
    return (int)GCWT_OK;
  });
}

int gcwt_coupling_surrogates(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                             int32_t phase_first, int32_t n_phase, int32_t amp_first, int32_t n_amp, int64_t window,
                             const int64_t* shifts, int32_t n_shifts, float* d_mean, float* d_sd, int32_t* d_count_ge,
                             float* d_surrogates, int64_t out_pitch) {
  return guarded([&] {
    if (!d_rows) return fail(GCWT_ERR_INVALID, "gcwt_coupling_surrogates: d_rows is NULL");
    if (!shifts) return fail(GCWT_ERR_INVALID, "gcwt_coupling_surrogates: shifts is NULL");
    gcwt::SurArgs a{};
    int rc = check_and_cut(pitch, n_channels, n_scales, n_cols, phase_first, n_phase, amp_first, n_amp, window, &a);
    if (rc) return rc;
    if (n_shifts < 2 || n_shifts > gcwt::kSurMaxShifts)
      return fail(GCWT_ERR_INVALID, "gcwt_coupling_surrogates: n_shifts must be in 2 .. 4096 (the sd divides by n_shifts - 1)");
    std::vector<int32_t> table((size_t)n_shifts);
    for (int32_t k = 0; k < n_shifts; ++k) {
      if (shifts[k] < 0 || shifts[k] >= window)
        return fail(GCWT_ERR_INVALID, "gcwt_coupling_surrogates: shift " + std::to_string(k) + " (" + std::to_string(shifts[k]) +
                                          " columns) is outside [0, window)");
      table[(size_t)k] = (int32_t)shifts[k];
    }
    if (!d_mean && !d_sd && !d_count_ge && !d_surrogates)
      return fail(GCWT_ERR_INVALID, "gcwt_coupling_surrogates: nothing to compute (no output)");
    if (out_pitch < a.n_bins)
      return fail(GCWT_ERR_INVALID, "gcwt_coupling_surrogates: out_pitch is below the number of bins, ceil(n_cols / window)");

    rc = resolve_device(kOp, d_rows, {d_mean, d_sd, d_count_ge, d_surrogates});
    if (rc) return rc;

    DeviceTable tab;
    const size_t at_shifts = tab.add(table.data(), table.size() * sizeof(int32_t));
    rc = tab.upload(kOp, "the shift list");
    if (rc) return rc;

    a.rows = reinterpret_cast<const float2*>(d_rows);
    a.shifts = tab.at<int32_t>(at_shifts);
    a.n_shifts = n_shifts;
    a.out_pitch = out_pitch;
    a.mean = d_mean; a.sd = d_sd; a.count_ge = d_count_ge; a.surrogates = d_surrogates;
    return finish(kOp, gcwt::launch_coupling_surrogates(a, nullptr));
  });
}

}  // extern "C"
