// detect_runs.h -- threshold statistics and threshold-crossing runs of float32 traces on the device (include/ghostcwt.h:
// gcwt_trace_stats, gcwt_trace_runs).  detect_runs.cpp checks the arguments, copies the thresholds, owns the work arrays
// and sizes the grids; detect_runs.hip does the work.  The tiles are regular -- kRunCols columns counted from column 0 --
// so a workgroup finds its (trace, tile) from its index: unit = trace * n_tiles + tile.
//
// The order of the statistics (every operation one correctly rounded float64 one; v = 0 for a column at or past n_cols):
//   lane     a lane owns kRunLaneCols adjacent columns and adds them in ascending order from an exact 0:
//            s1 = s1 + v, s2 = s2 + v * v (the product is exact), n = n + (v != 0)
//   wave     the six-level butterfly over the 64 lanes (lane ^ 1, ^ 2, ^ 4, ^ 8, ^ 16, ^ 32): both partners add the same
//            two numbers, so every lane holds the same bits
//   tile     the four waves of the workgroup in ascending order, from the first wave's sum: ((w0 + w1) + w2) + w3
//   trace    k_stats_sum, one wave per trace: lane l adds the tiles l, l + 64, l + 128, ... in ascending order from an
//            exact 0, then the same butterfly over the lanes
// so a trace's sums depend on its own columns and n_cols alone.  The host divides: mean = s1 / n, sd = sqrt(max(s2 / n -
// mean^2, 0)).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace gcwt {

constexpr int kRunThreads = 256;                     // four waves
constexpr int kRunLaneCols = 4;                      // adjacent columns of a lane: one 16-byte load
constexpr int kRunCols = kRunThreads * kRunLaneCols; // columns per tile
constexpr int kRunScanEntries = 4;                   // consecutive (trace, tile) entries of a lane of k_run_scan
constexpr int kRunPeakWaves = 4;                     // runs per workgroup of k_run_peak: one wave each

struct TileSums {              // what a tile (and, after k_stats_sum, a trace) adds up to
  double s1, s2;
  long long n;
};

struct TraceArgs {
  const float* trace;          // [n_traces] rows, pitch elements apart
  int64_t pitch, n_cols, n_traces, n_tiles, n_units;   // n_units = n_traces * n_tiles < 2^31
  int32_t aligned;             // every row starts on 16 bytes: a lane's four columns move as one vector
};

struct RunArgs {
  TraceArgs t;
  const float* lo;             // device copy: n_traces thresholds
  int2* counts;                // [n_units] (starts, stops) of each tile
  longlong2* offsets;          // [n_units + 1] their exclusive scan in (trace, tile) order; the last entry: the totals
  long long* trace_first;      // [n_traces + 1] the first record of each trace; the last entry: the number of records
  int64_t capacity;            // records the four output arrays hold
  long long* start; long long* stop; long long* peak_col; float* peak;
};

// everything about the traces that needs no device (host; `op` prefixes the message): fills the grid's numbers
int check_and_cut(const std::string& op, const float* d_trace, int64_t pitch, int64_t n_traces, int64_t n_cols, TraceArgs* a);

struct Cols { float v[kRunLaneCols]; };

// the lane's columns c0 .. c0 + 3 of `row`; 0 for a column at or past n_cols
__device__ __forceinline__ Cols load_cols(const TraceArgs& a, const float* row, int64_t c0) {
  Cols c;
#pragma unroll
  for (int j = 0; j < kRunLaneCols; ++j) c.v[j] = 0.f;
  if (c0 >= a.n_cols) return c;
  if (a.aligned) {                                           // pitch and c0 are multiples of 4: c0 + 3 < pitch
    const float4 q = *reinterpret_cast<const float4*>(row + c0);
    c.v[0] = q.x; c.v[1] = q.y; c.v[2] = q.z; c.v[3] = q.w;
#pragma unroll
    for (int j = 1; j < kRunLaneCols; ++j)
      if (c0 + j >= a.n_cols) c.v[j] = 0.f;
  } else {
#pragma unroll
    for (int j = 0; j < kRunLaneCols; ++j)
      if (c0 + j < a.n_cols) c.v[j] = row[c0 + j];
  }
  return c;
}

hipError_t launch_trace_stats(const TraceArgs& a, TileSums* tiles, TileSums* traces, hipStream_t st);
// k_run_count, k_run_scan: fills counts, offsets and trace_first
hipError_t launch_run_count(const RunArgs& a, hipStream_t st);
// k_run_fill, k_run_peak: the n_runs (<= capacity) records
hipError_t launch_run_fill(const RunArgs& a, int64_t n_runs, hipStream_t st);

}  // namespace gcwt
