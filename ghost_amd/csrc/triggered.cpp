// triggered.cpp -- the host side of gcwt_triggered (include/ghostcwt.h): argument checks, the grid (triggered.h:
// regular tiles, no task list), the device copy of the event list, the launch (triggered.hip).  Plan-independent, like
// gcwt_coupling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ghostcwt_debug.h"
#include "errors.h"
#include "resident_op.h"
#include "triggered.h"

static_assert(gcwt::kTrgRows == GCWT_TRIGGERED_TILE_ROWS && gcwt::kTrgLags == GCWT_TRIGGERED_TILE_LAGS,
              "ghostcwt_debug.h names the tile the kernel is built for");

using namespace gcwt;

namespace {

constexpr const char* kOp = "gcwt_triggered";
constexpr int64_t kMaxEvents = int64_t(1) << 24;            // (float)E is exact

// the grid of (n_channels, n_rows, before, after), each already checked
int cut(int32_t n_channels, int32_t n_rows, int64_t before, int64_t after, gcwt::TrgArgs* a) {
  a->n_channels = n_channels; a->n_rows = n_rows; a->before = before;
  a->n_lags = before + after + 1;
  a->n_rtiles = (n_rows + gcwt::kTrgRows - 1) / gcwt::kTrgRows;
  a->n_ltiles = (a->n_lags + gcwt::kTrgLags - 1) / gcwt::kTrgLags;
  // (each factor is below 2^31 before it is multiplied)
  if (a->n_ltiles > 0x7fffffff || (a->n_units = a->n_ltiles * n_channels) > 0x7fffffff ||
      gcwt::triggered_blocks(*a) > 0x7fffffff)
    return fail(GCWT_ERR_INVALID, "gcwt_triggered: channels x rows x lags need more than 2^31 - 1 workgroups: fewer rows or "
                                  "a shorter window per call");
  return GCWT_OK;
}

// everything that needs no device; fills the grid's numbers
int check_and_cut(const int64_t* events, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                  int32_t row_first, int32_t n_rows, int64_t n_events, int64_t before, int64_t after, gcwt::TrgArgs* a) {
  int rc = check_channels(kOp, n_channels);
  if (!rc) rc = check_rows(kOp, n_scales, n_cols, pitch);
  if (!rc) rc = check_row_range(kOp, "rows", row_first, n_rows, n_scales);
  if (rc) return rc;
  if (n_events < 1 || n_events > kMaxEvents)
    return fail(GCWT_ERR_INVALID, "gcwt_triggered: n_events must be in 1 .. 2^24");
  if (before < 0 || after < 0)
    return fail(GCWT_ERR_INVALID, "gcwt_triggered: before and after must be at least 0 columns");
  if (before >= n_cols || after >= n_cols - before)          // L = before + after + 1 <= n_cols, without overflow
    return fail(GCWT_ERR_INVALID, "gcwt_triggered: the window of before + after + 1 columns is longer than n_cols");
  for (int64_t k = 0; k < n_events; ++k)
    if (events[k] < before || events[k] >= n_cols - after)
      return fail(GCWT_ERR_INVALID, "gcwt_triggered: the window of event " + std::to_string(k) + " (column " +
                                        std::to_string(events[k]) + ") leaves [0, n_cols): before <= e and e + after < n_cols");
  a->pitch = pitch; a->n_scales = n_scales; a->row_first = row_first; a->n_events = n_events;
  return cut(n_channels, n_rows, before, after, a);
}

}  // namespace

extern "C" {

int gcwt_debug_triggered_grid(int32_t n_channels, int32_t n_rows, int64_t before, int64_t after, int32_t* n_row_tiles,
                              int64_t* n_lag_tiles, int64_t* n_blocks) {
  return guarded([&] {
    if (n_channels < 1 || n_rows < 1 || before < 0 || after < 0 || after > INT64_MAX - 1 - before)
      return fail(GCWT_ERR_INVALID, "gcwt_debug_triggered_grid: n_channels, n_rows >= 1; before, after >= 0");
    gcwt::TrgArgs a{};
    const int rc = cut(n_channels, n_rows, before, after, &a);
    if (rc) return rc;
    if (n_row_tiles) *n_row_tiles = a.n_rtiles;
    if (n_lag_tiles) *n_lag_tiles = a.n_ltiles;
    if (n_blocks) *n_blocks = gcwt::triggered_blocks(a);
    return (int)GCWT_OK;
  });
}

int gcwt_triggered(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                   int32_t row_first, int32_t n_rows, const int64_t* events, int64_t n_events, int64_t before,
                   int64_t after, float* d_amplitude, float* d_power, float* d_evoked, float* d_vector, float* d_itpc,
                   int64_t out_pitch) {
  return guarded([&] {
    if (!d_rows) return fail(GCWT_ERR_INVALID, "gcwt_triggered: d_rows is NULL");
    if (!events) return fail(GCWT_ERR_INVALID, "gcwt_triggered: events is NULL");
    gcwt::TrgArgs a{};
    int rc = check_and_cut(events, pitch, n_channels, n_scales, n_cols, row_first, n_rows, n_events, before, after, &a);
    if (rc) return rc;
    if (!d_amplitude && !d_power && !d_evoked && !d_vector && !d_itpc)
      return fail(GCWT_ERR_INVALID, "gcwt_triggered: nothing to compute (no output)");
    if (out_pitch < a.n_lags) return fail(GCWT_ERR_INVALID, "gcwt_triggered: out_pitch is below the number of lags, before + after + 1");

    rc = resolve_device(kOp, d_rows, {d_amplitude, d_power, d_evoked, d_vector, d_itpc});
    if (rc) return rc;

    DeviceTable tab;
    const size_t at_events = tab.add(events, (size_t)n_events * sizeof(int64_t));
    rc = tab.upload(kOp, "the event list");
    if (rc) return rc;

    a.rows = reinterpret_cast<const float2*>(d_rows);
    a.events = tab.at<int64_t>(at_events);
    a.out_pitch = out_pitch;
    a.amplitude = d_amplitude; a.power = d_power; a.itpc = d_itpc;
    a.evoked = reinterpret_cast<float2*>(d_evoked); a.vector = reinterpret_cast<float2*>(d_vector);
    return finish(kOp, gcwt::launch_triggered(a, nullptr));
  });
}

}  // extern "C"
