// squeeze.cpp -- the host side of gcwt_squeeze (include/ghostcwt.h): argument checks, the grid (squeeze.h: regular tiles,
// no task list), the device copy of the segment table, the three per-row tables and the cell edges, the launch
// (squeeze.hip).  Plan-independent, like gcwt_ridge.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "errors.h"
#include "resident_op.h"
#include "squeeze.h"

static_assert(gcwt::kSqCols == GCWT_SQUEEZE_TILE_COLS && gcwt::kSqCells == GCWT_SQUEEZE_GROUP_CELLS &&
                  gcwt::kSqMaxCells == GCWT_SQUEEZE_MAX_CELLS,
              "ghostcwt.h names the tile the kernel is built for");

using namespace gcwt;

namespace {

constexpr const char* kOp = "gcwt_squeeze";

// finite, above 0, strictly ascending
int check_edges(const float* edges, int32_t n_cells) {
  for (int32_t l = 0; l <= n_cells; ++l) {
    if (!std::isfinite(edges[l]) || !(edges[l] > 0.f))
      return fail(GCWT_ERR_INVALID, "gcwt_squeeze: edges[" + std::to_string(l) + "] must be finite and above 0");
    if (l > 0 && !(edges[l] > edges[l - 1]))
      return fail(GCWT_ERR_INVALID, "gcwt_squeeze: edges[" + std::to_string(l) + "] is not above edges[" + std::to_string(l - 1) +
                                        "]: the edges must be strictly ascending");
  }
  return GCWT_OK;
}

}  // namespace

extern "C" int gcwt_squeeze(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                            int32_t row_first, int32_t n_rows, const float* g, const float* floor2, const float* nu,
                            float hz_per_cycle, const int64_t* segments, int64_t n_segments, const float* edges, int32_t n_cells,
                            int32_t descending, float* d_coefficients, float* d_power, float* d_frequency, int32_t* d_index,
                            int64_t out_pitch) {
  return guarded([&] {
    if (!d_rows) return fail(GCWT_ERR_INVALID, "gcwt_squeeze: d_rows is NULL");
    if (!g) return fail(GCWT_ERR_INVALID, "gcwt_squeeze: g is NULL");
    if (!floor2) return fail(GCWT_ERR_INVALID, "gcwt_squeeze: floor2 is NULL");
    if (!nu) return fail(GCWT_ERR_INVALID, "gcwt_squeeze: nu is NULL");
    if (!segments || n_segments < 1) return fail(GCWT_ERR_INVALID, "gcwt_squeeze: segments is NULL or n_segments is below 1");
    if (!edges) return fail(GCWT_ERR_INVALID, "gcwt_squeeze: edges is NULL");
    if (!d_coefficients && !d_power && !d_frequency && !d_index)
      return fail(GCWT_ERR_INVALID, "gcwt_squeeze: nothing to compute (no output)");
    gcwt::SqArgs a{};
    int rc = check_channels(kOp, n_channels);
    if (!rc) rc = check_rows(kOp, n_scales, n_cols, pitch);
    if (!rc) rc = check_row_range(kOp, "rows", row_first, n_rows, n_scales);
    if (!rc) rc = check_table(kOp, "g", g, n_scales, Bound::kNone);
    if (!rc) rc = check_table(kOp, "floor2", floor2, n_scales, Bound::kAtLeast0);
    if (!rc) rc = check_table(kOp, "nu", nu, n_scales, Bound::kAtLeast0);
    if (!rc) rc = check_phase_advance(kOp, hz_per_cycle, segments, n_segments, n_cols);
    if (rc) return rc;
    if (n_cells < 1 || n_cells > gcwt::kSqMaxCells)
      return fail(GCWT_ERR_INVALID, "gcwt_squeeze: n_cells must be 1 .. " + std::to_string(gcwt::kSqMaxCells));
    rc = check_edges(edges, n_cells);
    if (rc) return rc;
    if (out_pitch < n_cols) return fail(GCWT_ERR_INVALID, "gcwt_squeeze: out_pitch is below n_cols");
    a.pitch = pitch; a.n_scales = n_scales; a.first = row_first; a.count = n_rows; a.n_cells = n_cells;
    // without coefficients and power nothing is summed: one group makes frequency and index
    rc = cut_column_tiles(kOp, "cells", gcwt::kSqCols, gcwt::squeeze_blocks, n_channels, n_cols,
                          d_coefficients || d_power ? (n_cells - 1) / gcwt::kSqCells + 1 : 1, &a);
    if (rc) return rc;

    rc = resolve_device(kOp, d_rows, {d_coefficients, d_power, d_frequency, d_index});
    if (rc) return rc;

    // one copy: the segment table (16-byte entries first), g, floor2, nu, the edges
    const size_t weights = (size_t)n_scales * sizeof(float);
    DeviceTable tab;
    const size_t at_segments = tab.add(segments, (size_t)n_segments * 2 * sizeof(int64_t));
    const size_t at_g = tab.add(g, weights), at_floor2 = tab.add(floor2, weights), at_nu = tab.add(nu, weights);
    const size_t at_edges = tab.add(edges, ((size_t)n_cells + 1) * sizeof(float), 16);
    rc = tab.upload(kOp, "the row, edge and segment tables");
    if (rc) return rc;

    a.rows = reinterpret_cast<const float2*>(d_rows);
    a.segments = tab.at<longlong2>(at_segments);
    a.n_segments = n_segments;
    a.g = tab.at<float>(at_g);
    a.floor2 = tab.at<float>(at_floor2);
    a.nu = tab.at<float>(at_nu);
    a.edges = tab.at<float>(at_edges);
    a.descending = descending != 0;
    a.hz_per_cycle = hz_per_cycle;
    a.out_pitch = out_pitch;
    a.coefficients = reinterpret_cast<float2*>(d_coefficients);
    a.power = d_power; a.frequency = d_frequency; a.index = d_index;
    a.aligned = rows_on16(d_rows, pitch, out_pitch, {d_coefficients, d_power, d_frequency, d_index});
    return finish(kOp, gcwt::launch_squeeze(a, nullptr));
  });
}
