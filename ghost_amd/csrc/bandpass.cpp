// bandpass.cpp -- the host side of gcwt_bandpass (include/ghostcwt.h): argument checks, the grid (bandpass.h: regular
// tiles, no task list), the device copy of the band table and the weights, the launch (bandpass.hip).
// Plan-independent, like gcwt_triggered.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ghostcwt_debug.h"
#include "bandpass.h"
#include "errors.h"
#include "resident_op.h"

static_assert(gcwt::kBpCols == GCWT_BANDPASS_TILE_COLS && gcwt::kBpBands == GCWT_BANDPASS_GROUP_BANDS,
              "ghostcwt_debug.h names the tile the kernel is built for");

using namespace gcwt;

namespace {

constexpr const char* kOp = "gcwt_bandpass";

// the grid of (n_channels, n_cols, n_bands), each already checked
int cut(int32_t n_channels, int64_t n_cols, int32_t n_bands, gcwt::BpArgs* a) {
  a->n_bands = n_bands;
  return cut_column_tiles(kOp, "bands", gcwt::kBpCols, gcwt::bandpass_blocks, n_channels, n_cols,
                          (n_bands - 1) / gcwt::kBpBands + 1, a);
}

// everything that needs no device; fills the grid's numbers
int check_and_cut(int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols, const int32_t* bands, int32_t n_bands,
                  const float* g, const float* h, gcwt::BpArgs* a) {
  int rc = check_channels(kOp, n_channels);
  if (!rc) rc = check_rows(kOp, n_scales, n_cols, pitch);
  if (!rc) rc = check_band_list(kOp, bands, n_bands, n_scales);
  if (!rc && g) rc = check_table(kOp, "g", g, n_scales, Bound::kNone);
  if (!rc && h) rc = check_table(kOp, "h", h, n_scales, Bound::kAtLeast0);
  if (rc) return rc;
  a->pitch = pitch; a->n_scales = n_scales;
  return cut(n_channels, n_cols, n_bands, a);
}

}  // namespace

extern "C" {

int gcwt_debug_bandpass_grid(int32_t n_channels, int64_t n_cols, int32_t n_bands, int64_t* n_col_tiles,
                             int32_t* n_band_groups, int64_t* n_blocks) {
  return guarded([&] {
    if (n_channels < 1 || n_cols < 1 || n_bands < 1)
      return fail(GCWT_ERR_INVALID, "gcwt_debug_bandpass_grid: n_channels, n_cols, n_bands >= 1");
    gcwt::BpArgs a{};
    const int rc = cut(n_channels, n_cols, n_bands, &a);
    if (rc) return rc;
    if (n_col_tiles) *n_col_tiles = a.n_ctiles;
    if (n_band_groups) *n_band_groups = a.n_groups;
    if (n_blocks) *n_blocks = gcwt::bandpass_blocks(a);
    return (int)GCWT_OK;
  });
}

int gcwt_bandpass(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                  const int32_t* bands, int32_t n_bands, const float* g, const float* h, float* d_analytic,
                  float* d_envelope, float* d_power, int64_t out_pitch) {
  return guarded([&] {
    if (!d_rows) return fail(GCWT_ERR_INVALID, "gcwt_bandpass: d_rows is NULL");
    if (!bands) return fail(GCWT_ERR_INVALID, "gcwt_bandpass: bands is NULL");
    if (!d_analytic && !d_envelope && !d_power) return fail(GCWT_ERR_INVALID, "gcwt_bandpass: nothing to compute (no output)");
    if (!g && (d_analytic || d_envelope))
      return fail(GCWT_ERR_INVALID, "gcwt_bandpass: g is NULL and analytic or envelope is asked for");
    if (!h && d_power) return fail(GCWT_ERR_INVALID, "gcwt_bandpass: h is NULL and power is asked for");
    gcwt::BpArgs a{};
    int rc = check_and_cut(pitch, n_channels, n_scales, n_cols, bands, n_bands, g, h, &a);
    if (rc) return rc;
    if (out_pitch < n_cols) return fail(GCWT_ERR_INVALID, "gcwt_bandpass: out_pitch is below n_cols");

    rc = resolve_device(kOp, d_rows, {d_analytic, d_envelope, d_power});
    if (rc) return rc;

    // one copy: the band table, then g, then h (zeros for a weight array that no output asked for needs)
    const size_t weights = (size_t)n_scales * sizeof(float);
    DeviceTable tab;
    const size_t at_bands = tab.add(bands, (size_t)n_bands * 2 * sizeof(int32_t)), at_g = tab.add(g, weights);
    const size_t at_h = tab.add(h, weights);
    rc = tab.upload(kOp, "the band table");
    if (rc) return rc;

    a.rows = reinterpret_cast<const float2*>(d_rows);
    a.bands = tab.at<int2>(at_bands);
    a.g = tab.at<float>(at_g);
    a.h = tab.at<float>(at_h);
    a.out_pitch = out_pitch;
    a.analytic = reinterpret_cast<float2*>(d_analytic); a.envelope = d_envelope; a.power = d_power;
    a.aligned = rows_on16(d_rows, pitch, out_pitch, {d_analytic, d_envelope, d_power});
    return finish(kOp, gcwt::launch_bandpass(a, nullptr));
  });
}

}  // extern "C"
