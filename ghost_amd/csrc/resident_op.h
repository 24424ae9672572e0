// resident_op.h -- what the operators on the rows of a resident complex result and on traces share (coherence, coupling,
// triggered, bandpass, ridge, squeeze, the trace operators): the host's argument checks, the device that holds the
// rows, the packed device copy of an entry's host tables, the cut of a grid of regular column tiles, the launch tail;
// and for the kernels the grid placement of tiles that read the same rows and the loads of a host table.  Includable
// from .hip (the placement, the loads).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

namespace gcwt {

// ---- host: checks that need no device.  `op` is the entry point's name, the prefix of every message; each returns
// GCWT_OK or the code it has reported (errors.h).
int check_channels(const char* op, int32_t n_channels);
int check_rows(const char* op, int32_t n_scales, int64_t n_cols, int64_t pitch);
int check_window(const char* op, int64_t window);
// `noun`: what the message calls the range ("rows", "phase rows", ...)
int check_row_range(const char* op, const char* noun, int32_t first, int32_t count, int32_t n_scales);
// a table `name` of n float32, one per row or trace: every entry finite and inside the bound
enum class Bound { kNone, kAtLeast0, kAbove0 };
int check_table(const char* op, const char* name, const float* w, int64_t n, Bound bound);
// the (first row, rows) pairs of a band list: at least one, each a row range ("band k")
int check_band_list(const char* op, const int32_t* bands, int32_t n_bands, int32_t n_scales);
// (start, stop) pairs: ascending, each holding a column and starting where the one before stops, from 0 to n_cols
int check_segments(const char* op, const int64_t* segments, int64_t n_segments, int64_t n_cols);
// what a phase advance becomes a frequency with: hz_per_cycle finite and > 0, then n_segments >= 1 such segments
int check_phase_advance(const char* op, float hz_per_cycle, const int64_t* segments, int64_t n_segments, int64_t n_cols);

// d_rows must be device memory and every non-NULL output memory of the same device; on GCWT_OK that device is the
// calling thread's, from here on.
int resolve_device(const char* op, const void* d_rows, std::initializer_list<const void*> outputs);

// 16 bytes: what a float4 or longlong2 access needs of an address and an offset
inline bool on16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
inline size_t up16(size_t bytes) { return (bytes + 15) / 16 * 16; }
// every row of complex rows `pitch` apart at d_rows and every row of the (non-NULL) outputs, out_pitch apart, starts
// on 16 bytes: a lane's two columns move as one vector
bool rows_on16(const void* d_rows, int64_t pitch, int64_t out_pitch, std::initializer_list<const void*> outputs);

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

// The host tables of one entry, packed into one device allocation: add() the parts in the order the kernel's
// arguments expect them, upload() once, then at<T>() gives each part's device address.
class DeviceTable {
 public:
  // `bytes` of `host` (NULL: zeros) behind the parts so far, at the next multiple of `align` -> the part's offset
  size_t add(const void* host, size_t bytes, size_t align = 1);
  // one allocation, one copy; GCWT_OK or the code reported as "<op>: no device memory for <what>: ..." (without a
  // `what`, "<op>: ...") and "<op>: ..."
  int upload(const char* op, const char* what);
  template <class T>
  const T* at(size_t offset) const { return reinterpret_cast<const T*>(static_cast<const char*>(copy_.p) + offset); }

 private:
  std::vector<char> staged_;
  DeviceCopy copy_;
};

// GCWT_ERR_HIP, reported as "<op>: <what HIP says of e>"
int hip_failed(const char* op, hipError_t e);
// the end of an entry: waits for the kernels whose launch returned `launched`; GCWT_OK or hip_failed
int finish(const char* op, hipError_t launched);

// ---- the grid placement (host and device).  Workgroups b and b + kShare are dealt to the same XCD, so the tiles of
// one unit -- which read the same rows -- are placed kShare apart: index = (group of kShare units, tile, unit in the
// group).  They start together and meet their rows in one L2.  For speed only; nothing depends on the placement.
constexpr int kShare = 8;

// workgroups of the grid: every (unit, tile), units padded to a multiple of kShare
inline int64_t shared_blocks(int64_t n_units, int64_t n_tiles) {
  return (n_units + kShare - 1) / kShare * kShare * n_tiles;
}

// The grid of an operator whose units are (channel, `cols` columns counted from column 0), each cut into n_groups
// tiles (bandpass, ridge, squeeze), every number already checked: fills n_channels, n_cols, n_groups, n_ctiles and
// n_units of its arguments -> GCWT_OK or the code reported.  `blocks`: the operator's *_blocks; `noun`: what the
// message calls a group's members ("bands", "cells").
int too_many_blocks(const char* op, const char* noun);   // reports it; resident_op.cpp
template <class Args>
int cut_column_tiles(const char* op, const char* noun, int cols, int64_t (*blocks)(const Args&), int32_t n_channels,
                     int64_t n_cols, int32_t n_groups, Args* a) {
  a->n_channels = n_channels; a->n_cols = n_cols; a->n_groups = n_groups;
  a->n_ctiles = (n_cols - 1) / cols + 1;
  // (each factor is below 2^31 before it is multiplied)
  if (a->n_ctiles > 0x7fffffff || (a->n_units = a->n_ctiles * n_channels) > 0x7fffffff || blocks(*a) > 0x7fffffff)
    return too_many_blocks(op, noun);
  return 0;                                                  // GCWT_OK
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

// ---- device: a table that the host writes before the launch and nobody after it is read through the constant address
// space, where a wave-uniform index gives a scalar load.
template <class T>
using Const = const T __attribute__((address_space(4)))*;
template <class T>
__device__ __forceinline__ Const<T> constant(const T* p) { return (Const<T>)reinterpret_cast<uintptr_t>(p); }

}  // namespace gcwt
