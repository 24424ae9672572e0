// coupling.cpp -- the host side of gcwt_coupling (include/ghostcwt.h): argument checks, the grid (coupling.h: regular
// tiles, no task list), the launch (coupling.hip).  Plan-independent, like gcwt_coherence.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "../../include/ghostcwt.h"
#include "../../include/ghostcwt_debug.h"
#include "coupling.h"

int gcwt_internal_set_error(int code, const char* msg);   // api.cpp (C++ linkage)

static_assert(gcwt::kCplPhase == GCWT_COUPLING_TILE_PHASE && gcwt::kCplAmp == GCWT_COUPLING_TILE_AMP,
              "ghostcwt_debug.h names the tile the kernel is built for");

namespace {

int fail(int code, const std::string& m) { return gcwt_internal_set_error(code, m.c_str()); }

// nothing may unwind across the C ABI
template <typename F>
int guarded(F&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail(GCWT_ERR_NOMEM, "out of host memory");
  } catch (...) {
    return fail(GCWT_ERR_INVALID, "internal error");
  }
}

// everything that needs no device; fills the grid's numbers
int check_and_cut(int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols, int32_t phase_first,
                  int32_t n_phase, int32_t amp_first, int32_t n_amp, int64_t window, gcwt::CplArgs* a) {
  if (n_channels < 1) return fail(GCWT_ERR_INVALID, "gcwt_coupling: n_channels must be at least 1");
  if (n_scales < 1 || n_cols < 1 || pitch < n_cols)
    return fail(GCWT_ERR_INVALID, "gcwt_coupling: bad rows (n_scales, n_cols >= 1, pitch >= n_cols)");
  if (window < 2) return fail(GCWT_ERR_INVALID, "gcwt_coupling: window must be at least 2 columns");
  if (phase_first < 0 || n_phase < 1 || n_phase > n_scales - phase_first)
    return fail(GCWT_ERR_INVALID, "gcwt_coupling: the phase rows must be a non-empty range inside [0, n_scales)");
  if (amp_first < 0 || n_amp < 1 || n_amp > n_scales - amp_first)
    return fail(GCWT_ERR_INVALID, "gcwt_coupling: the amplitude rows must be a non-empty range inside [0, n_scales)");
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
    const int rc = check_and_cut(pitch, n_channels, n_scales, n_cols, phase_first, n_phase, amp_first, n_amp, window, &a);
    if (rc) return rc;
    if (!d_vector && !d_mvl && !d_amplitude) return fail(GCWT_ERR_INVALID, "gcwt_coupling: nothing to compute (no output)");
    if (out_pitch < a.n_bins) return fail(GCWT_ERR_INVALID, "gcwt_coupling: out_pitch is below the number of bins, ceil(n_cols / window)");

    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
      (void)hipGetLastError();
      return fail(GCWT_ERR_NO_DEVICE, "no HIP device: libghostcwt has no CPU path");
    }
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, d_rows) != hipSuccess || attr.type != hipMemoryTypeDevice) {
      (void)hipGetLastError();
      return fail(GCWT_ERR_INVALID, "gcwt_coupling: d_rows is not device memory");
    }
    const int device = attr.device;
    for (const void* out : {(const void*)d_vector, (const void*)d_mvl, (const void*)d_amplitude}) {
      if (!out) continue;
      if (hipPointerGetAttributes(&attr, out) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != device) {
        (void)hipGetLastError();
        return fail(GCWT_ERR_INVALID, "gcwt_coupling: an output is not memory of the device that holds d_rows");
      }
    }
    hipError_t e = hipSetDevice(device);                   // (the calling thread's device, from here on)
    if (e != hipSuccess) return fail(GCWT_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));

    a.rows = reinterpret_cast<const float2*>(d_rows);
    a.out_pitch = out_pitch;
    a.vector = reinterpret_cast<float2*>(d_vector); a.mvl = d_mvl; a.amplitude = d_amplitude;
    e = gcwt::launch_coupling(a, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(GCWT_ERR_HIP, std::string("gcwt_coupling: ") + hipGetErrorString(e));
    return (int)GCWT_OK;
  });
}

}  // extern "C"
