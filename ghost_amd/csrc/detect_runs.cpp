// detect_runs.cpp -- the host side of gcwt_trace_stats and gcwt_trace_runs (include/ghostcwt.h): argument checks, the
// grid (detect_runs.h: regular tiles), the device copy of the thresholds, the work arrays, the launches
// (detect_runs.hip) and the few numbers that come back.  Plan-independent, like gcwt_bandpass.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/ghostcwt_debug.h"
#include "detect_runs.h"
#include "errors.h"
#include "resident_op.h"

static_assert(gcwt::kRunCols == GCWT_RUNS_TILE_COLS, "ghostcwt_debug.h names the tile the kernels are built for");

using namespace gcwt;

namespace gcwt {

int check_and_cut(const std::string& op, const float* d_trace, int64_t pitch, int64_t n_traces, int64_t n_cols, TraceArgs* a) {
  if (!d_trace) return fail(GCWT_ERR_INVALID, op + ": d_trace is NULL");
  if (n_traces < 1) return fail(GCWT_ERR_INVALID, op + ": n_traces must be at least 1");
  if (n_cols < 1 || n_cols >= (int64_t)1 << 40 || pitch < n_cols)
    return fail(GCWT_ERR_INVALID, op + ": bad traces (1 <= n_cols < 2^40, pitch >= n_cols)");
  a->trace = d_trace; a->pitch = pitch; a->n_cols = n_cols; a->n_traces = n_traces;
  a->n_tiles = (n_cols - 1) / kRunCols + 1;
  // (each factor is below 2^31 before it is multiplied)
  if (n_traces > 0x7fffffff || (a->n_units = a->n_tiles * n_traces) > 0x7fffffff)
    return fail(GCWT_ERR_INVALID, op + ": traces x columns need more than 2^31 - 1 workgroups: fewer traces per call");
  a->aligned = pitch % kRunLaneCols == 0 && reinterpret_cast<uintptr_t>(d_trace) % 16 == 0;
  return GCWT_OK;
}

}  // namespace gcwt

extern "C" {

int gcwt_trace_stats(const float* d_trace, int64_t pitch, int64_t n_traces, int64_t n_cols, int64_t* n, double* mean,
                     double* sd) {
  return guarded([&] {
    const std::string op = "gcwt_trace_stats";
    TraceArgs a{};
    int rc = check_and_cut(op, d_trace, pitch, n_traces, n_cols, &a);
    if (rc) return rc;
    if (!n || !mean || !sd) return fail(GCWT_ERR_INVALID, op + ": n, mean or sd is NULL");
    rc = resolve_device(op.c_str(), d_trace, {});
    if (rc) return rc;

    // one allocation: the tiles' sums, then the traces'
    const size_t tiles = (size_t)a.n_units * sizeof(TileSums), traces = (size_t)n_traces * sizeof(TileSums);
    DeviceCopy work;
    hipError_t e = work.alloc(tiles + traces);
    if (e != hipSuccess) return fail(GCWT_ERR_NOMEM, op + ": no device memory for the tiles' sums: " + hipGetErrorString(e));
    TileSums* d_tiles = static_cast<TileSums*>(work.p);
    TileSums* d_traces = d_tiles + a.n_units;
    e = launch_trace_stats(a, d_tiles, d_traces, nullptr);
    std::vector<TileSums> sums((size_t)n_traces);
    if (e == hipSuccess) e = hipMemcpy(sums.data(), d_traces, traces, hipMemcpyDeviceToHost);      // (waits for the kernels)
    if (e != hipSuccess) return hip_failed(op.c_str(), e);
    for (int64_t i = 0; i < n_traces; ++i) {
      const TileSums& s = sums[(size_t)i];
      n[i] = s.n;
      mean[i] = sd[i] = 0.0;
      if (s.n == 0) continue;
      const double m = s.s1 / (double)s.n, var = s.s2 / (double)s.n - m * m;
      mean[i] = m;
      sd[i] = std::sqrt(var < 0.0 ? 0.0 : var);              // (a NaN passes through: NaN < 0 is false)
    }
    return (int)GCWT_OK;
  });
}

int gcwt_trace_runs(const float* d_trace, int64_t pitch, int64_t n_traces, int64_t n_cols, const float* lo, int64_t capacity,
                    int64_t* d_start, int64_t* d_stop, int64_t* d_peak_col, float* d_peak, int64_t* counts) {
  return guarded([&] {
    const std::string op = "gcwt_trace_runs";
    RunArgs a{};
    int rc = check_and_cut(op, d_trace, pitch, n_traces, n_cols, &a.t);
    if (rc) return rc;
    if (!lo) return fail(GCWT_ERR_INVALID, op + ": lo is NULL");
    if (!counts) return fail(GCWT_ERR_INVALID, op + ": counts is NULL");
    rc = check_table(op.c_str(), "lo", lo, n_traces, Bound::kNone);
    if (rc) return rc;
    if (capacity < 0) return fail(GCWT_ERR_INVALID, op + ": capacity must be at least 0");
    if (capacity > 0 && (!d_start || !d_stop || !d_peak_col || !d_peak))
      return fail(GCWT_ERR_INVALID, op + ": capacity is above 0 and d_start, d_stop, d_peak_col or d_peak is NULL");
    if (capacity == 0) d_start = d_stop = d_peak_col = nullptr, d_peak = nullptr;
    rc = resolve_device(op.c_str(), d_trace, {d_start, d_stop, d_peak_col, d_peak});
    if (rc) return rc;

    // one allocation: the tiles' counts, their scan, the traces' first records, the thresholds
    const size_t n_units = (size_t)a.t.n_units;
    const size_t at_offsets = up16(n_units * sizeof(int2)), at_first = at_offsets + (n_units + 1) * sizeof(longlong2);
    const size_t first_bytes = ((size_t)n_traces + 1) * sizeof(long long), at_lo = up16(at_first + first_bytes);
    DeviceCopy work;
    hipError_t e = work.alloc(at_lo + (size_t)n_traces * sizeof(float));
    if (e != hipSuccess) return fail(GCWT_ERR_NOMEM, op + ": no device memory for the tiles' counts: " + hipGetErrorString(e));
    e = work.put(at_lo, lo, (size_t)n_traces * sizeof(float));
    if (e != hipSuccess) return hip_failed(op.c_str(), e);
    char* base = static_cast<char*>(work.p);
    a.counts = reinterpret_cast<int2*>(base);
    a.offsets = reinterpret_cast<longlong2*>(base + at_offsets);
    a.trace_first = reinterpret_cast<long long*>(base + at_first);
    a.lo = reinterpret_cast<const float*>(base + at_lo);
    a.capacity = capacity;
    a.start = reinterpret_cast<long long*>(d_start); a.stop = reinterpret_cast<long long*>(d_stop);
    a.peak_col = reinterpret_cast<long long*>(d_peak_col); a.peak = d_peak;

    e = launch_run_count(a, nullptr);
    std::vector<long long> first((size_t)n_traces + 1);
    if (e == hipSuccess) e = hipMemcpy(first.data(), a.trace_first, first_bytes, hipMemcpyDeviceToHost);   // (waits)
    if (e != hipSuccess) return hip_failed(op.c_str(), e);
    for (int64_t i = 0; i < n_traces; ++i) counts[i] = first[(size_t)i + 1] - first[(size_t)i];
    const int64_t n_runs = first[(size_t)n_traces];
    if (n_runs == 0 || n_runs > capacity) return (int)GCWT_OK;                  // nothing to write / the caller sizes and returns

    return finish(op.c_str(), launch_run_fill(a, n_runs, nullptr));
  });
}

}  // extern "C"
