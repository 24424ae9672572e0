// ridge.cpp -- the host side of gcwt_ridge (include/ghostcwt.h): argument checks, the grid (ridge.h: regular tiles, no
// task list), the device copy of the band table, the weights, the phase advances and the segment table, the launch
// (ridge.hip).  Plan-independent, like gcwt_bandpass.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "errors.h"
#include "resident_op.h"
#include "ridge.h"

static_assert(gcwt::kRgCols == GCWT_RIDGE_TILE_COLS && gcwt::kRgBands == GCWT_RIDGE_GROUP_BANDS,
              "ghostcwt.h names the tile the kernel is built for");

using namespace gcwt;

namespace {

constexpr const char* kOp = "gcwt_ridge";

// the grid of (n_channels, n_cols, n_bands), each already checked
int cut(int32_t n_channels, int64_t n_cols, int32_t n_bands, gcwt::RgArgs* a) {
  a->n_channels = n_channels; a->n_cols = n_cols; a->n_bands = n_bands;
  a->n_ctiles = (n_cols - 1) / gcwt::kRgCols + 1;
  a->n_groups = (n_bands - 1) / gcwt::kRgBands + 1;
  // (each factor is below 2^31 before it is multiplied)
  if (a->n_ctiles > 0x7fffffff || (a->n_units = a->n_ctiles * n_channels) > 0x7fffffff || gcwt::ridge_blocks(*a) > 0x7fffffff)
    return fail(GCWT_ERR_INVALID, "gcwt_ridge: channels x columns x bands need more than 2^31 - 1 workgroups: fewer bands or "
                                  "fewer channels per call");
  return GCWT_OK;
}

bool on16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
size_t up16(size_t v) { return (v + 15) / 16 * 16; }

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
    if (rc) return rc;
    if (n_bands < 1) return fail(GCWT_ERR_INVALID, "gcwt_ridge: n_bands must be at least 1");
    for (int32_t k = 0; k < n_bands; ++k) {
      rc = check_row_range(kOp, ("band " + std::to_string(k)).c_str(), bands[2 * k], bands[2 * k + 1], n_scales);
      if (rc) return rc;
    }
    rc = check_table(kOp, "e", e, n_scales, true);
    if (!rc) rc = check_table(kOp, "nu", nu, n_scales, false);
    if (rc) return rc;
    if (!std::isfinite(hz_per_cycle) || !(hz_per_cycle > 0.f)) return fail(GCWT_ERR_INVALID, "gcwt_ridge: hz_per_cycle must be finite and above 0");
    if (n_segments > n_cols) return fail(GCWT_ERR_INVALID, "gcwt_ridge: more segments than columns");
    rc = check_segments(kOp, segments, n_segments, n_cols);
    if (rc) return rc;
    if (out_pitch < n_cols) return fail(GCWT_ERR_INVALID, "gcwt_ridge: out_pitch is below n_cols");
    a.pitch = pitch; a.n_scales = n_scales;
    rc = cut(n_channels, n_cols, n_bands, &a);
    if (rc) return rc;

    rc = resolve_device(kOp, d_rows, {d_row, d_amplitude, d_offset, d_frequency});
    if (rc) return rc;

    // one copy: the segment table (16-byte entries first), the band table, e, nu
    const size_t seg_bytes = (size_t)n_segments * 2 * sizeof(int64_t), table = (size_t)n_bands * 2 * sizeof(int32_t);
    const size_t weights = (size_t)n_scales * sizeof(float), at_bands = seg_bytes, at_e = up16(at_bands + table);
    DeviceCopy copy;
    hipError_t err = copy.alloc(at_e + 2 * weights);
    if (err != hipSuccess)
      return fail(GCWT_ERR_NOMEM, std::string("gcwt_ridge: no device memory for the band and segment tables: ") + hipGetErrorString(err));
    err = copy.put(0, segments, seg_bytes);
    if (err == hipSuccess) err = copy.put(at_bands, bands, table);
    if (err == hipSuccess) err = copy.put(at_e, e, weights);
    if (err == hipSuccess) err = copy.put(at_e + weights, nu, weights);
    if (err != hipSuccess) return fail(GCWT_ERR_HIP, std::string("gcwt_ridge: ") + hipGetErrorString(err));

    const char* base = static_cast<const char*>(copy.p);
    a.rows = reinterpret_cast<const float2*>(d_rows);
    a.segments = reinterpret_cast<const longlong2*>(base);
    a.n_segments = n_segments;
    a.bands = reinterpret_cast<const int2*>(base + at_bands);
    a.e = reinterpret_cast<const float*>(base + at_e);
    a.nu = a.e + n_scales;
    a.hz_per_cycle = hz_per_cycle;
    a.out_pitch = out_pitch;
    a.row = d_row; a.amplitude = d_amplitude; a.offset = d_offset; a.frequency = d_frequency;
    a.aligned = pitch % 2 == 0 && out_pitch % 2 == 0 && on16(d_rows) && on16(d_row) && on16(d_amplitude) && on16(d_offset) &&
                on16(d_frequency);
    err = gcwt::launch_ridge(a, nullptr);
    if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
    if (err != hipSuccess) return fail(GCWT_ERR_HIP, std::string("gcwt_ridge: ") + hipGetErrorString(err));
    return (int)GCWT_OK;
  });
}
