// trace_smooth.cpp -- the host side of gcwt_trace_smooth (include/ghostcwt.h): argument checks, the device copy of the
// taps, the segments and the members, the launch (trace_smooth.hip).  Plan-independent, like gcwt_trace_stats.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/ghostcwt_debug.h"
#include "errors.h"
#include "resident_op.h"
#include "trace_smooth.h"

static_assert(gcwt::kSmMaxHalf == GCWT_SMOOTH_MAX_HALF, "ghostcwt.h names the limit the kernel is built for");
static_assert(gcwt::kSmCols == GCWT_SMOOTH_TILE_COLS, "ghostcwt_debug.h names the tile the kernel is built for");

using namespace gcwt;

extern "C" {

int gcwt_trace_smooth(const float* d_trace, int64_t pitch, int64_t n_traces, int64_t n_cols, const float* taps, int32_t half,
                      const int64_t* segments, int64_t n_segments, const int32_t* members, int32_t n_members, float* d_out,
                      int64_t out_pitch) {
  return guarded([&] {
    const std::string op = "gcwt_trace_smooth";
    SmoothArgs a{};
    int rc = check_and_cut(op, d_trace, pitch, n_traces, n_cols, &a.t);
    if (rc) return rc;
    if (!taps) return fail(GCWT_ERR_INVALID, op + ": taps is NULL");
    if (half < 0) return fail(GCWT_ERR_INVALID, op + ": half must be at least 0, not " + std::to_string(half));
    if (half > kSmMaxHalf)
      return fail(GCWT_ERR_INVALID, op + ": half = " + std::to_string(half) + " is above GCWT_SMOOTH_MAX_HALF = " +
                                        std::to_string(kSmMaxHalf) + ": the kernel counts in columns, and an output_stride shortens it");
    rc = check_table(op.c_str(), "taps", taps, (int64_t)half + 1, Bound::kNone);
    if (rc) return rc;
    if ((segments == nullptr) != (n_segments == 0) || n_segments < 0)
      return fail(GCWT_ERR_INVALID, op + ": segments and n_segments must be given together (NULL and 0: one segment, every column)");
    int64_t end = 0;                                         // where the segment before this one stops
    for (int64_t i = 0; i < n_segments; ++i) {
      const int64_t start = segments[2 * i], stop = segments[2 * i + 1];
      const std::string which = op + ": segments[" + std::to_string(i) + "] = [" + std::to_string(start) + ", " + std::to_string(stop) + ")";
      if (start < 0 || stop > n_cols || start >= stop)
        return fail(GCWT_ERR_INVALID, which + " must hold a column and lie inside [0, " + std::to_string(n_cols) + ")");
      if (start < end)
        return fail(GCWT_ERR_INVALID, which + " starts before the segment before it stops at " + std::to_string(end) +
                                          ": ascending, disjoint segments");
      end = stop;
    }
    if ((members == nullptr) != (n_members == 0) || n_members < 0)
      return fail(GCWT_ERR_INVALID, op + ": members and n_members must be given together (NULL and 0: every trace on its own)");
    for (int32_t i = 0; i < n_members; ++i)
      if (members[i] < 0 || members[i] >= n_traces)
        return fail(GCWT_ERR_INVALID, op + ": members[" + std::to_string(i) + "] = " + std::to_string(members[i]) + " is no trace (0 .. " +
                                          std::to_string(n_traces - 1) + ")");
    if (!d_out) return fail(GCWT_ERR_INVALID, op + ": d_out is NULL");
    if (out_pitch < n_cols) return fail(GCWT_ERR_INVALID, op + ": out_pitch must be at least n_cols");
    a.n_out = n_members ? 1 : n_traces;
    const int64_t most = (int64_t)1 << 60;                   // elements: what follows is computed without overflow
    if (n_traces - 1 > most / pitch || a.n_out - 1 > most / out_pitch)
      return fail(GCWT_ERR_INVALID, op + ": n_traces x pitch (or out_pitch) is beyond 2^60 elements");
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(d_trace), out0 = reinterpret_cast<uintptr_t>(d_out);
    const uintptr_t in1 = in0 + (uintptr_t)((n_traces - 1) * pitch + n_cols) * sizeof(float);
    const uintptr_t out1 = out0 + (uintptr_t)((a.n_out - 1) * out_pitch + n_cols) * sizeof(float);
    if (in0 < out1 && out0 < in1) return fail(GCWT_ERR_INVALID, op + ": d_out overlaps d_trace: the smoothed traces need memory of their own");
    rc = resolve_device(op.c_str(), d_trace, {d_out});
    if (rc) return rc;

    a.half = half;
    a.halo = (half + kSmLaneCols - 1) / kSmLaneCols * kSmLaneCols;
    a.w0 = taps[0];
    a.n_members = n_members;
    a.inv_members = n_members ? (float)(1.0 / (double)n_members) : 1.f;
    a.out = d_out;
    a.out_pitch = out_pitch;
    a.out_aligned = out_pitch % kSmLaneCols == 0 && out0 % 16 == 0;
    const int64_t whole[2] = {0, n_cols};
    if (!segments) { segments = whole; n_segments = 1; }
    a.n_segments = n_segments;

    // one allocation: the taps w_1 .. (zeros up to a multiple of 4), the segments, the members
    std::vector<float> later((size_t)a.halo + kSmLaneCols, 0.f);          // (never empty)
    for (int32_t k = 1; k <= half; ++k) later[(size_t)k - 1] = taps[k];
    DeviceTable tab;
    const size_t at_taps = tab.add(later.data(), later.size() * sizeof(float));
    static_assert(sizeof(longlong2) == 2 * sizeof(int64_t), "the (start, stop) pairs are copied as they are");
    const size_t at_segments = tab.add(segments, (size_t)n_segments * 2 * sizeof(int64_t), 16);
    const size_t at_members = tab.add(members, (size_t)(n_members ? n_members : 1) * sizeof(int32_t), 16);
    rc = tab.upload(op.c_str(), "the taps and the segments");
    if (rc) return rc;
    a.taps = tab.at<float>(at_taps);
    a.segments = tab.at<longlong2>(at_segments);
    a.members = n_members ? tab.at<int32_t>(at_members) : nullptr;

    return finish(op.c_str(), launch_trace_smooth(a, nullptr));           // (the tables go when this returns)
  });
}

}  // extern "C"
