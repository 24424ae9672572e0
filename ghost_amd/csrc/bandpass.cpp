// bandpass.cpp -- the host side of gcwt_bandpass (include/ghostcwt.h): argument checks, the grid (bandpass.h: regular
// tiles, no task list), the device copy of the band table and the weights, the launch (bandpass.hip).
// Plan-independent, like gcwt_triggered.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

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
  a->n_channels = n_channels; a->n_cols = n_cols; a->n_bands = n_bands;
  a->n_ctiles = (n_cols - 1) / gcwt::kBpCols + 1;
  a->n_groups = (n_bands - 1) / gcwt::kBpBands + 1;
  // (each factor is below 2^31 before it is multiplied)
  if (a->n_ctiles > 0x7fffffff || (a->n_units = a->n_ctiles * n_channels) > 0x7fffffff ||
      gcwt::bandpass_blocks(*a) > 0x7fffffff)
    return fail(GCWT_ERR_INVALID, "gcwt_bandpass: channels x columns x bands need more than 2^31 - 1 workgroups: fewer bands or "
                                  "fewer channels per call");
  return GCWT_OK;
}

int check_weights(const char* name, const float* w, int32_t n_scales, bool sign) {
  for (int32_t r = 0; r < n_scales; ++r)
    if (!std::isfinite(w[r]) || (sign && w[r] < 0.f))
      return fail(GCWT_ERR_INVALID, std::string("gcwt_bandpass: ") + name + "[" + std::to_string(r) + "] must be finite" +
                                        (sign ? " and at least 0" : ""));
  return GCWT_OK;
}

// everything that needs no device; fills the grid's numbers
int check_and_cut(int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols, const int32_t* bands, int32_t n_bands,
                  const float* g, const float* h, gcwt::BpArgs* a) {
  int rc = check_channels(kOp, n_channels);
  if (!rc) rc = check_rows(kOp, n_scales, n_cols, pitch);
  if (rc) return rc;
  if (n_bands < 1) return fail(GCWT_ERR_INVALID, "gcwt_bandpass: n_bands must be at least 1");
  for (int32_t k = 0; k < n_bands; ++k) {
    rc = check_row_range(kOp, ("band " + std::to_string(k)).c_str(), bands[2 * k], bands[2 * k + 1], n_scales);
    if (rc) return rc;
  }
  if (g) rc = check_weights("g", g, n_scales, false);
  if (!rc && h) rc = check_weights("h", h, n_scales, true);
  if (rc) return rc;
  a->pitch = pitch; a->n_scales = n_scales;
  return cut(n_channels, n_cols, n_bands, a);
}

bool on16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

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
    const size_t table = (size_t)n_bands * 2 * sizeof(int32_t), weights = (size_t)n_scales * sizeof(float);
    const std::vector<float> none((size_t)n_scales, 0.f);
    DeviceCopy copy;
    hipError_t e = copy.alloc(table + 2 * weights);
    if (e != hipSuccess)
      return fail(GCWT_ERR_NOMEM, std::string("gcwt_bandpass: no device memory for the band table: ") + hipGetErrorString(e));
    e = copy.put(0, bands, table);
    if (e == hipSuccess) e = copy.put(table, g ? g : none.data(), weights);
    if (e == hipSuccess) e = copy.put(table + weights, h ? h : none.data(), weights);
    if (e != hipSuccess) return fail(GCWT_ERR_HIP, std::string("gcwt_bandpass: ") + hipGetErrorString(e));

    a.rows = reinterpret_cast<const float2*>(d_rows);
    a.bands = static_cast<const int2*>(copy.p);
    a.g = reinterpret_cast<const float*>(static_cast<const char*>(copy.p) + table);
    a.h = a.g + n_scales;
    a.out_pitch = out_pitch;
    a.analytic = reinterpret_cast<float2*>(d_analytic); a.envelope = d_envelope; a.power = d_power;
    a.aligned = pitch % 2 == 0 && out_pitch % 2 == 0 && on16(d_rows) && on16(d_analytic) && on16(d_envelope) && on16(d_power);
    e = gcwt::launch_bandpass(a, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(GCWT_ERR_HIP, std::string("gcwt_bandpass: ") + hipGetErrorString(e));
    return (int)GCWT_OK;
  });
}

}  // extern "C"
