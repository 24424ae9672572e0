// ridge.cpp -- the host side of gcwt_ridge (include/ghostcwt.h): argument checks, the grid (ridge.h: regular tiles, no
// task list), the device copy of the band table, the weights, the phase advances and the segment table, the launch
// (ridge.hip).  Plan-independent, like gcwt_bandpass.
#include <hip/hip_runtime.h>

#include "errors.h"
#include "resident_op.h"
#include "ridge.h"

static_assert(gcwt::kRgCols == GCWT_RIDGE_TILE_COLS && gcwt::kRgBands == GCWT_RIDGE_GROUP_BANDS,
              "ghostcwt.h names the tile the kernel is built for");

using namespace gcwt;

namespace {

constexpr const char* kOp = "gcwt_ridge";

}  // namespace

extern "C" int gcwt_ridge(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                          const int32_t* bands, int32_t n_bands, const float* e, const float* nu, float hz_per_cycle,
                          const int64_t* segments, int64_t n_segments, int32_t* d_row, float* d_amplitude, float* d_offset,
                          float* d_frequency, int64_t out_pitch) {
  return guarded([&] {
    if (!d_rows) return fail(GCWT_ERR_INVALID, "gcwt_ridge: d_rows is NULL");
    if (!bands) return fail(GCWT_ERR_INVALID, "gcwt_ridge: bands is NULL");
    if (!e) return fail(GCWT_ERR_INVALID, "gcwt_ridge: e is NULL");
    if (!nu) return fail(GCWT_ERR_INVALID, "gcwt_ridge: nu is NULL");
    if (!segments || n_segments < 1) return fail(GCWT_ERR_INVALID, "gcwt_ridge: segments is NULL or n_segments is below 1");
    if (!d_row && !d_amplitude && !d_offset && !d_frequency) return fail(GCWT_ERR_INVALID, "gcwt_ridge: nothing to compute (no output)");
    gcwt::RgArgs a{};
    int rc = check_channels(kOp, n_channels);
    if (!rc) rc = check_rows(kOp, n_scales, n_cols, pitch);
    if (!rc) rc = check_band_list(kOp, bands, n_bands, n_scales);
    if (!rc) rc = check_table(kOp, "e", e, n_scales, Bound::kAbove0);
    if (!rc) rc = check_table(kOp, "nu", nu, n_scales, Bound::kAtLeast0);
    if (!rc) rc = check_phase_advance(kOp, hz_per_cycle, segments, n_segments, n_cols);
    if (rc) return rc;
    if (out_pitch < n_cols) return fail(GCWT_ERR_INVALID, "gcwt_ridge: out_pitch is below n_cols");
    a.pitch = pitch; a.n_scales = n_scales; a.n_bands = n_bands;
    rc = cut_column_tiles(kOp, "bands", gcwt::kRgCols, gcwt::ridge_blocks, n_channels, n_cols, (n_bands - 1) / gcwt::kRgBands + 1, &a);
    if (rc) return rc;

    rc = resolve_device(kOp, d_rows, {d_row, d_amplitude, d_offset, d_frequency});
    if (rc) return rc;

    // one copy: the segment table (16-byte entries first), the band table, e, nu
    const size_t weights = (size_t)n_scales * sizeof(float);
    DeviceTable tab;
    const size_t at_segments = tab.add(segments, (size_t)n_segments * 2 * sizeof(int64_t));
    const size_t at_bands = tab.add(bands, (size_t)n_bands * 2 * sizeof(int32_t));
    const size_t at_e = tab.add(e, weights, 16), at_nu = tab.add(nu, weights);
    rc = tab.upload(kOp, "the band and segment tables");
    if (rc) return rc;

    a.rows = reinterpret_cast<const float2*>(d_rows);
    a.segments = tab.at<longlong2>(at_segments);
    a.n_segments = n_segments;
    a.bands = tab.at<int2>(at_bands);
    a.e = tab.at<float>(at_e);
    a.nu = tab.at<float>(at_nu);
    a.hz_per_cycle = hz_per_cycle;
    a.out_pitch = out_pitch;
    a.row = d_row; a.amplitude = d_amplitude; a.offset = d_offset; a.frequency = d_frequency;
    a.aligned = rows_on16(d_rows, pitch, out_pitch, {d_row, d_amplitude, d_offset, d_frequency});
    return finish(kOp, gcwt::launch_ridge(a, nullptr));
  });
}
