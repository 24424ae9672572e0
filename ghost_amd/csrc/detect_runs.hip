// detect_runs.hip -- the kernels of gcwt_trace_stats and gcwt_trace_runs (include/ghostcwt.h; detect_runs.h has the
// order of the statistics; profiles/detect.md).  Both work on float32 traces, kRunCols columns to a workgroup of four
// waves, a lane on kRunLaneCols adjacent columns: one 16-byte load where the rows start on 16 bytes (`aligned`, which the
// Python layer's pitches always give), else one load per column.  An aligned load may reach into a row's padding (never
// past pitch); what it brings from there is masked before it is used.  No atomics: every number has one writer.
//
// The runs.  Column t of a trace is above iff v[t] > lo, columns -1 and n_cols are not.  A start flag is above[t] &&
// !above[t - 1], a stop flag above[t] && !above[t + 1]; the k-th start and the k-th stop of a trace belong to the same
// run, so the two compact independently and no run is followed across tiles -- a tile reads one column of halo on
// either side instead.
//   k_run_count   per (trace, tile): the numbers of start and stop flags
//   k_run_scan    one workgroup: their exclusive scan in (trace, tile) order as int64, and each trace's first record
//   k_run_fill    per (trace, tile): start[offset + rank] = t, stop[offset + rank] = t + 1; the rank of a flag is the
//                 number of flags in lower columns of the tile: popcounts of the lower lanes' bits of a ballot, plus the
//                 totals of the lower waves from LDS
//   k_run_peak    one wave per run: lane l looks at the columns start + l, start + l + 64, ... and keeps (value, column)
//                 of the first largest with a strict >; the butterfly over the lanes takes the larger value and, where
//                 two are equal, the smaller column
// Everything written is an integer or a copy of an input value: the result does not depend on any of this.
#include <hip/hip_runtime.h>

#include <cmath>

#include "detect_runs.h"

namespace gcwt {

namespace {

constexpr int kWaves = kRunThreads / 64;

// ---- the statistics ------------------------------------------------------------------------------------------------
__device__ __forceinline__ TileSums wave_add(TileSums s) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    s.s1 = __dadd_rn(s.s1, __shfl_xor(s.s1, m));
    s.s2 = __dadd_rn(s.s2, __shfl_xor(s.s2, m));
    s.n += __shfl_xor(s.n, m);
  }
  return s;
}

__global__ void __launch_bounds__(kRunThreads) k_stats_tile(TraceArgs a, TileSums* tiles) {
  __shared__ TileSums part[kWaves];
  const int64_t unit = blockIdx.x;                           // (the grid has exactly n_units workgroups)
  const int64_t trace = unit / a.n_tiles, tile = unit % a.n_tiles;
  const Cols c = load_cols(a, a.trace + trace * a.pitch, tile * kRunCols + (int64_t)threadIdx.x * kRunLaneCols);
  TileSums s{0.0, 0.0, 0};
#pragma unroll
  for (int j = 0; j < kRunLaneCols; ++j) {
    const double v = (double)c.v[j];
    s.s1 = __dadd_rn(s.s1, v);
    s.s2 = __dadd_rn(s.s2, __dmul_rn(v, v));
    s.n += c.v[j] != 0.f;
  }
  s = wave_add(s);
  if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    TileSums t = part[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      t.s1 = __dadd_rn(t.s1, part[w].s1);
      t.s2 = __dadd_rn(t.s2, part[w].s2);
      t.n += part[w].n;
    }
    tiles[unit] = t;
  }
}

__global__ void __launch_bounds__(64) k_stats_sum(const TileSums* tiles, int64_t n_tiles, TileSums* traces) {
  const int64_t trace = blockIdx.x;
  TileSums s{0.0, 0.0, 0};
  for (int64_t t = threadIdx.x; t < n_tiles; t += 64) {
    const TileSums p = tiles[trace * n_tiles + t];
    s.s1 = __dadd_rn(s.s1, p.s1);
    s.s2 = __dadd_rn(s.s2, p.s2);
    s.n += p.n;
  }
  s = wave_add(s);
  if (threadIdx.x == 0) traces[trace] = s;
}

// ---- the runs ------------------------------------------------------------------------------------------------------
struct Flags { unsigned start, stop; };                      // bit j: column c0 + j

// The start and stop flags of the lane's columns.  Every lane of the workgroup must call it (a barrier inside).
__device__ __forceinline__ Flags tile_flags(const RunArgs& a, int64_t trace, int64_t tile, unsigned char* above) {
  const TraceArgs& t = a.t;
  const float* row = t.trace + trace * t.pitch;
  const float lo = a.lo[trace];
  const int64_t first = tile * kRunCols, c0 = first + (int64_t)threadIdx.x * kRunLaneCols;
  const Cols c = load_cols(t, row, c0);
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < kRunLaneCols; ++j)
    if (c0 + j < t.n_cols && c.v[j] > lo) m |= 1u << j;      // (a column past n_cols is not above, whatever lo is)
  // above[1 + lane] = the lane's bits; above[0] and above[kRunThreads + 1] = the halo columns first - 1 and first + kRunCols
  above[1 + threadIdx.x] = (unsigned char)m;
  if (threadIdx.x == 0) above[0] = first > 0 && row[first - 1] > lo ? 1u << (kRunLaneCols - 1) : 0;
  if (threadIdx.x == kRunThreads - 1) above[kRunThreads + 1] = first + kRunCols < t.n_cols && row[first + kRunCols] > lo ? 1 : 0;
  __syncthreads();
  const unsigned prev = (above[threadIdx.x] >> (kRunLaneCols - 1)) & 1u, next = above[threadIdx.x + 2] & 1u;
  const unsigned all = (1u << kRunLaneCols) - 1;
  Flags f;
  f.start = m & ~((m << 1) | prev) & all;
  f.stop = m & ~((m >> 1) | (next << (kRunLaneCols - 1))) & all;
  return f;
}

__device__ __forceinline__ int wave_add(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

__global__ void __launch_bounds__(kRunThreads) k_run_count(RunArgs a) {
  __shared__ unsigned char above[kRunThreads + 2];
  __shared__ int2 part[kWaves];
  const int64_t unit = blockIdx.x;
  const Flags f = tile_flags(a, unit / a.t.n_tiles, unit % a.t.n_tiles, above);
  const int starts = wave_add(__popc(f.start)), stops = wave_add(__popc(f.stop));
  if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = make_int2(starts, stops);
  __syncthreads();
  if (threadIdx.x == 0) {
    int2 t = part[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) { t.x += part[w].x; t.y += part[w].y; }
    a.counts[unit] = t;
  }
}

// One workgroup walks the n_units entries in chunks of kRunThreads * kRunScanEntries; `carry` is what lies before the chunk.
__global__ void __launch_bounds__(kRunThreads) k_run_scan(RunArgs a) {
  __shared__ longlong2 part[kWaves];
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  const int64_t n = a.t.n_units;
  longlong2 carry = make_longlong2(0, 0);
  for (int64_t base = 0; base < n; base += (int64_t)kRunThreads * kRunScanEntries) {
    const int64_t i0 = base + (int64_t)threadIdx.x * kRunScanEntries;
    int2 c[kRunScanEntries];
    longlong2 mine = make_longlong2(0, 0);
#pragma unroll
    for (int j = 0; j < kRunScanEntries; ++j) {
      c[j] = i0 + j < n ? a.counts[i0 + j] : make_int2(0, 0);
      mine.x += c[j].x; mine.y += c[j].y;
    }
    longlong2 incl = mine;                                   // the inclusive scan over the lanes of the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long x = __shfl_up(incl.x, d), y = __shfl_up(incl.y, d);
      if (lane >= d) { incl.x += x; incl.y += y; }
    }
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    longlong2 before = carry, total = carry;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) { before.x += part[w].x; before.y += part[w].y; }
      total.x += part[w].x; total.y += part[w].y;
    }
    longlong2 at = make_longlong2(before.x + incl.x - mine.x, before.y + incl.y - mine.y);
#pragma unroll
    for (int j = 0; j < kRunScanEntries; ++j) {
      if (i0 + j < n) a.offsets[i0 + j] = at;
      at.x += c[j].x; at.y += c[j].y;
    }
    carry = total;
    __syncthreads();                                         // part[] is written again in the next chunk
  }
  if (threadIdx.x == 0) a.offsets[n] = carry;
  __syncthreads();                                           // (orders the workgroup's own global writes too)
  for (int64_t i = threadIdx.x; i <= a.t.n_traces; i += kRunThreads) a.trace_first[i] = a.offsets[i * a.t.n_tiles].x;
}

// the number of set flags of bit j, j = 0 .. 3, in the lanes below this one / in the whole wave
__device__ __forceinline__ void wave_rank(unsigned flags, int lane, int* below, int* total) {
  const unsigned long long lower = (1ull << lane) - 1;
  int b = 0, t = 0;
#pragma unroll
  for (int j = 0; j < kRunLaneCols; ++j) {
    const unsigned long long ballot = __ballot((flags >> j) & 1u);
    b += __popcll(ballot & lower);
    t += __popcll(ballot);
  }
  *below = b; *total = t;
}

__global__ void __launch_bounds__(kRunThreads) k_run_fill(RunArgs a) {
  __shared__ unsigned char above[kRunThreads + 2];
  __shared__ int2 part[kWaves];
  const int64_t unit = blockIdx.x;
  const int64_t tile = unit % a.t.n_tiles;
  const Flags f = tile_flags(a, unit / a.t.n_tiles, tile, above);
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  int2 below, total;
  wave_rank(f.start, lane, &below.x, &total.x);
  wave_rank(f.stop, lane, &below.y, &total.y);
  if (lane == 0) part[wave] = total;
  __syncthreads();
  const longlong2 off = a.offsets[unit];
  long long at_start = off.x + below.x, at_stop = off.y + below.y;
  for (int w = 0; w < wave; ++w) { at_start += part[w].x; at_stop += part[w].y; }
  const int64_t c0 = tile * kRunCols + (int64_t)threadIdx.x * kRunLaneCols;
#pragma unroll
  for (int j = 0; j < kRunLaneCols; ++j) {
    // (at < capacity follows from the scan of the same flags; the test keeps a trace that changed in between inside the arrays)
    if ((f.start >> j) & 1u) { if (at_start < a.capacity) a.start[at_start] = c0 + j; ++at_start; }
    if ((f.stop >> j) & 1u) { if (at_stop < a.capacity) a.stop[at_stop] = c0 + j + 1; ++at_stop; }
  }
}

__global__ void __launch_bounds__(kRunPeakWaves * 64) k_run_peak(RunArgs a, int64_t n_runs) {
  const int lane = threadIdx.x % 64;
  const int64_t run = (int64_t)blockIdx.x * kRunPeakWaves + threadIdx.x / 64;          // wave-uniform
  if (run >= n_runs) return;
  // the trace of the run: the last one whose first record is not behind it
  int64_t lo = 0, hi = a.t.n_traces;                         // trace_first[lo] <= run < trace_first[hi]
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a.trace_first[mid] <= run) lo = mid; else hi = mid;
  }
  const float* row = a.t.trace + lo * a.t.pitch;
  const int64_t start = a.start[run], stop = a.stop[run];
  if (start < 0 || stop > a.t.n_cols) return;                // (cannot be: k_run_fill wrote them from the same trace)
  float best = -INFINITY;                                    // below every column of a run: they are above a finite lo
  long long col = 0x7fffffffffffffffll;
  for (int64_t t = start + lane; t < stop; t += 64) {
    const float v = row[t];
    if (v > best) { best = v; col = t; }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const float v = __shfl_xor(best, m);
    const long long c = __shfl_xor(col, m);
    if (v > best || (v == best && c < col)) { best = v; col = c; }
  }
  if (lane == 0) { a.peak[run] = best; a.peak_col[run] = col; }
}

bool launchable(int64_t blocks) { return blocks > 0 && blocks <= 0x7fffffff; }

}  // namespace

hipError_t launch_trace_stats(const TraceArgs& a, TileSums* tiles, TileSums* traces, hipStream_t st) {
  if (!launchable(a.n_units) || !launchable(a.n_traces)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_stats_tile, dim3((unsigned)a.n_units), dim3(kRunThreads), 0, st, a, tiles);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_stats_sum, dim3((unsigned)a.n_traces), dim3(64), 0, st, tiles, a.n_tiles, traces);
  return hipGetLastError();
}

hipError_t launch_run_count(const RunArgs& a, hipStream_t st) {
  if (!launchable(a.t.n_units)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_run_count, dim3((unsigned)a.t.n_units), dim3(kRunThreads), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_run_scan, dim3(1), dim3(kRunThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_run_fill(const RunArgs& a, int64_t n_runs, hipStream_t st) {
  const int64_t peak_blocks = (n_runs + kRunPeakWaves - 1) / kRunPeakWaves;
  if (!launchable(a.t.n_units) || !launchable(peak_blocks) || n_runs > a.capacity) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_run_fill, dim3((unsigned)a.t.n_units), dim3(kRunThreads), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_run_peak, dim3((unsigned)peak_blocks), dim3(kRunPeakWaves * 64), 0, st, a, n_runs);
  return hipGetLastError();
}

}  // namespace gcwt
