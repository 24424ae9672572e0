// resident_op.cpp -- the host side every row operator shares (resident_op.h).
#include "resident_op.h"

#include <cmath>
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

int check_table(const char* op, const char* name, const float* w, int32_t n_scales, bool strict) {
  for (int32_t r = 0; r < n_scales; ++r)
    if (!std::isfinite(w[r]) || (strict ? !(w[r] > 0.f) : w[r] < 0.f))
      return fail(GCWT_ERR_INVALID, std::string(op) + ": " + name + "[" + std::to_string(r) + "] must be finite and " +
                                        (strict ? "above 0" : "at least 0"));
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

}  // namespace gcwt
