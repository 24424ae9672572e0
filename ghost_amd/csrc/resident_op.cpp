// resident_op.cpp -- the host side every row operator shares (resident_op.h).
#include "resident_op.h"

#include <cmath>
#include <cstring>
#include <string>

#include "errors.h"

namespace gcwt {

int check_channels(const char* op, int32_t n_channels) {
  if (n_channels < 1) return fail(GCWT_ERR_INVALID, std::string(op) + ": n_channels must be at least 1");
  return GCWT_OK;
}

int check_rows(const char* op, int32_t n_scales, int64_t n_cols, int64_t pitch) {
  if (n_scales < 1 || n_cols < 1 || pitch < n_cols)
    return fail(GCWT_ERR_INVALID, std::string(op) + ": bad rows (n_scales, n_cols >= 1, pitch >= n_cols)");
  return GCWT_OK;
}

int check_window(const char* op, int64_t window) {
  if (window < 2) return fail(GCWT_ERR_INVALID, std::string(op) + ": window must be at least 2 columns");
  return GCWT_OK;
}

int check_row_range(const char* op, const char* noun, int32_t first, int32_t count, int32_t n_scales) {
  if (first < 0 || count < 1 || count > n_scales - first)
    return fail(GCWT_ERR_INVALID, std::string(op) + ": the " + noun + " must be a non-empty range inside [0, n_scales)");
  return GCWT_OK;
}

int check_table(const char* op, const char* name, const float* w, int64_t n, Bound bound) {
  for (int64_t r = 0; r < n; ++r)
    if (!std::isfinite(w[r]) || (bound == Bound::kAbove0 && !(w[r] > 0.f)) || (bound == Bound::kAtLeast0 && w[r] < 0.f))
      return fail(GCWT_ERR_INVALID, std::string(op) + ": " + name + "[" + std::to_string(r) + "] must be finite" +
                                        (bound == Bound::kAbove0 ? " and above 0" : bound == Bound::kAtLeast0 ? " and at least 0" : ""));
  return GCWT_OK;
}

int check_band_list(const char* op, const int32_t* bands, int32_t n_bands, int32_t n_scales) {
  if (n_bands < 1) return fail(GCWT_ERR_INVALID, std::string(op) + ": n_bands must be at least 1");
  for (int32_t k = 0; k < n_bands; ++k) {
    const int rc = check_row_range(op, ("band " + std::to_string(k)).c_str(), bands[2 * k], bands[2 * k + 1], n_scales);
    if (rc) return rc;
  }
  return GCWT_OK;
}

int check_segments(const char* op, const int64_t* segments, int64_t n_segments, int64_t n_cols) {
  int64_t end = 0;                                           // where the segment before this one stops
  for (int64_t i = 0; i < n_segments; ++i) {
    const int64_t start = segments[2 * i], stop = segments[2 * i + 1];
    const std::string which = std::string(op) + ": segments[" + std::to_string(i) + "] = [" + std::to_string(start) + ", " +
                              std::to_string(stop) + ")";
    if (stop <= start) return fail(GCWT_ERR_INVALID, which + " holds no column");
    if (start != end)
      return fail(GCWT_ERR_INVALID, which + (start < end ? " starts before" : " leaves columns uncovered after") +
                                        " the end of the segment before it at " + std::to_string(end) +
                                        ": ascending, disjoint segments that cover [0, n_cols)");
    if (stop > n_cols) return fail(GCWT_ERR_INVALID, which + " ends past n_cols = " + std::to_string(n_cols));
    end = stop;
  }
  if (end != n_cols)
    return fail(GCWT_ERR_INVALID, std::string(op) + ": segments[" + std::to_string(n_segments - 1) + "] stops at " +
                                      std::to_string(end) + " and leaves the columns up to n_cols = " + std::to_string(n_cols) +
                                      " uncovered");
  return GCWT_OK;
}

int check_phase_advance(const char* op, float hz_per_cycle, const int64_t* segments, int64_t n_segments, int64_t n_cols) {
  if (!std::isfinite(hz_per_cycle) || !(hz_per_cycle > 0.f))
    return fail(GCWT_ERR_INVALID, std::string(op) + ": hz_per_cycle must be finite and above 0");
  if (n_segments > n_cols) return fail(GCWT_ERR_INVALID, std::string(op) + ": more segments than columns");
  return check_segments(op, segments, n_segments, n_cols);
}

int too_many_blocks(const char* op, const char* noun) {
  return fail(GCWT_ERR_INVALID, std::string(op) + ": channels x columns x " + noun + " need more than 2^31 - 1 workgroups: fewer " +
                                    noun + " or fewer channels per call");
}

int resolve_device(const char* op, const void* d_rows, std::initializer_list<const void*> outputs) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
    (void)hipGetLastError();
    return fail(GCWT_ERR_NO_DEVICE, "no HIP device: libghostcwt has no CPU path");
  }
  auto device_of = [](const void* p) {                     // -1: not device memory
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice) return attr.device;
    (void)hipGetLastError();
    return -1;
  };
  const int device = device_of(d_rows);
  if (device < 0) return fail(GCWT_ERR_INVALID, std::string(op) + ": d_rows is not device memory");
  for (const void* out : outputs)
    if (out && device_of(out) != device)
      return fail(GCWT_ERR_INVALID, std::string(op) + ": an output is not memory of the device that holds d_rows");
  const hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail(GCWT_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  return GCWT_OK;
}

bool rows_on16(const void* d_rows, int64_t pitch, int64_t out_pitch, std::initializer_list<const void*> outputs) {
  bool all = pitch % 2 == 0 && out_pitch % 2 == 0 && on16(d_rows);
  for (const void* out : outputs) all = all && on16(out);
  return all;
}

DeviceCopy::~DeviceCopy() {
  if (p) (void)hipFree(p);
}

hipError_t DeviceCopy::alloc(size_t bytes) {
  const hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    p = nullptr;
    (void)hipGetLastError();
  }
  return e;
}

hipError_t DeviceCopy::put(size_t offset, const void* host, size_t bytes) {
  return hipMemcpy(static_cast<char*>(p) + offset, host, bytes, hipMemcpyHostToDevice);
}

size_t DeviceTable::add(const void* host, size_t bytes, size_t align) {
  const size_t at = (staged_.size() + align - 1) / align * align;
  staged_.resize(at + bytes, 0);
  if (host && bytes) std::memcpy(staged_.data() + at, host, bytes);
  return at;
}

int DeviceTable::upload(const char* op, const char* what) {
  hipError_t e = copy_.alloc(staged_.size());
  if (e != hipSuccess)
    return fail(GCWT_ERR_NOMEM, std::string(op) + ": " + (what ? std::string("no device memory for ") + what + ": " : "") +
                                    hipGetErrorString(e));
  e = copy_.put(0, staged_.data(), staged_.size());
  return e == hipSuccess ? (int)GCWT_OK : hip_failed(op, e);
}

int hip_failed(const char* op, hipError_t e) { return fail(GCWT_ERR_HIP, std::string(op) + ": " + hipGetErrorString(e)); }

int finish(const char* op, hipError_t launched) {
  if (launched == hipSuccess) launched = hipStreamSynchronize(nullptr);
  return launched == hipSuccess ? (int)GCWT_OK : hip_failed(op, launched);
}

}  // namespace gcwt
