// resident_op.h -- what the operators that reduce the rows of a resident complex result in place share (coherence,
// coupling, triggered, bandpass): the host's argument checks, the device that holds the rows, a temporary device copy of a host
// table, and the grid placement of tiles that read the same rows.  Includable from .hip (the placement).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace gcwt {

// ---- host: checks that need no device.  `op` is the entry point's name, the prefix of every message; each returns
// GCWT_OK or the code it has reported (errors.h).
int check_channels(const char* op, int32_t n_channels);
int check_rows(const char* op, int32_t n_scales, int64_t n_cols, int64_t pitch);
int check_window(const char* op, int64_t window);
// `noun`: what the message calls the range ("rows", "phase rows", ...)
int check_row_range(const char* op, const char* noun, int32_t first, int32_t count, int32_t n_scales);
// a per-row table `name` of n_scales float32: every entry finite and, with strict, > 0, else >= 0
int check_table(const char* op, const char* name, const float* w, int32_t n_scales, bool strict);
// (start, stop) pairs: ascending, each holding a column and starting where the one before stops, from 0 to n_cols
int check_segments(const char* op, const int64_t* segments, int64_t n_segments, int64_t n_cols);

// d_rows must be device memory and every non-NULL output memory of the same device; on GCWT_OK that device is the
// calling thread's, from here on.
int resolve_device(const char* op, const void* d_rows, std::initializer_list<const void*> outputs);

// A device allocation that lives as long as this object and is filled from host memory.  A failed allocation leaves
// no sticky HIP error behind.
struct DeviceCopy {
  void* p = nullptr;
  DeviceCopy() = default;
  DeviceCopy(const DeviceCopy&) = delete;
  DeviceCopy& operator=(const DeviceCopy&) = delete;
  ~DeviceCopy();
  hipError_t alloc(size_t bytes);
  hipError_t put(size_t offset, const void* host, size_t bytes);   // synchronous
};

// ---- the grid placement (host and device).  Workgroups b and b + kShare are dealt to the same XCD, so the tiles of
// one unit -- which read the same rows -- are placed kShare apart: index = (group of kShare units, tile, unit in the
// group).  They start together and meet their rows in one L2.  For speed only; nothing depends on the placement.
constexpr int kShare = 8;

// workgroups of the grid: every (unit, tile), units padded to a multiple of kShare
inline int64_t shared_blocks(int64_t n_units, int64_t n_tiles) {
  return (n_units + kShare - 1) / kShare * kShare * n_tiles;
}

struct TileOfUnit {
  int tile;
  int64_t unit;                // >= n_units in the last group's padding
};
__device__ __forceinline__ TileOfUnit shared_place(int n_tiles) {
  int64_t idx = blockIdx.x;
  const int member = (int)(idx % kShare);
  idx /= kShare;
  const int tile = (int)(idx % n_tiles);
  return {tile, idx / n_tiles * kShare + member};
}

}  // namespace gcwt
