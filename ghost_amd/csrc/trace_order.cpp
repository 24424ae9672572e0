// trace_order.cpp -- the host side of gcwt_trace_order (include/ghostcwt.h): argument checks, the work arrays (the
// histograms of the three passes, the state of every (trace, rank), the centres), the launches (trace_order.hip) and the
// numbers that come back.  Plan-independent, like gcwt_trace_stats.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/ghostcwt_debug.h"
#include "errors.h"
#include "resident_op.h"
#include "trace_order.h"

static_assert(gcwt::kOrderChunkCols == GCWT_ORDER_CHUNK_COLS, "ghostcwt_debug.h names the chunk the kernels are built for");

using namespace gcwt;

extern "C" {

int gcwt_trace_order(const float* d_trace, int64_t pitch, int64_t n_traces, int64_t n_cols, const float* center,
                     const int64_t* ranks, int32_t n_ranks, int64_t* n, float* out) {
  return guarded([&] {
    const std::string op = "gcwt_trace_order";
    OrderArgs a{};
    int rc = check_and_cut(op, d_trace, pitch, n_traces, n_cols, &a.t);
    if (rc) return rc;
    if (!ranks || !n || !out) return fail(GCWT_ERR_INVALID, op + ": ranks, n or out is NULL");
    if (n_ranks < 1 || n_ranks > kOrderMaxRanks)
      return fail(GCWT_ERR_INVALID, op + ": n_ranks must be 1 .. " + std::to_string(kOrderMaxRanks) + ", not " + std::to_string(n_ranks));
    const int64_t n_states = n_traces * n_ranks;             // (below 2^33)
    if (n_states > 0x7fffffff)
      return fail(GCWT_ERR_INVALID, op + ": traces x ranks need more than 2^31 - 1 workgroups: fewer traces per call");
    for (int64_t i = 0; i < n_states; ++i)
      if (ranks[i] < 0) return fail(GCWT_ERR_INVALID, op + ": ranks[" + std::to_string(i) + "] must be at least 0");
    if (center) rc = check_table(op.c_str(), "center", center, n_traces, Bound::kNone);
    if (!rc) rc = resolve_device(op.c_str(), d_trace, {});
    if (rc) return rc;

    a.n_ranks = n_ranks;
    a.n_chunks = (n_cols - 1) / kOrderChunkCols + 1;
    // one allocation: the histograms (zeroed), then the states, n, the values and the centres
    const size_t hist0 = (size_t)n_traces * kOrderBins * sizeof(unsigned long long), hist_later = hist0 * (size_t)n_ranks;
    const size_t at_state = hist0 + 2 * hist_later, at_n = at_state + (size_t)n_states * sizeof(OrderState);
    const size_t at_out = at_n + (size_t)n_traces * sizeof(long long), at_center = up16(at_out + (size_t)n_states * sizeof(unsigned));
    DeviceCopy work;
    hipError_t e = work.alloc(at_center + (size_t)n_traces * sizeof(float));
    if (e != hipSuccess) return fail(GCWT_ERR_NOMEM, op + ": no device memory for the histograms: " + hipGetErrorString(e));
    char* base = static_cast<char*>(work.p);
    a.hist[0] = reinterpret_cast<unsigned long long*>(base);
    a.hist[1] = reinterpret_cast<unsigned long long*>(base + hist0);
    a.hist[2] = reinterpret_cast<unsigned long long*>(base + hist0 + hist_later);
    a.state = reinterpret_cast<OrderState*>(base + at_state);
    a.n = reinterpret_cast<long long*>(base + at_n);
    a.out = reinterpret_cast<unsigned*>(base + at_out);
    std::vector<OrderState> state((size_t)n_states);
    for (int64_t i = 0; i < n_states; ++i) state[(size_t)i] = OrderState{0u, 1, (long long)ranks[i]};
    e = hipMemset(base, 0, at_state);
    if (e == hipSuccess) e = work.put(at_state, state.data(), state.size() * sizeof(OrderState));
    if (e == hipSuccess && center) {
      e = work.put(at_center, center, (size_t)n_traces * sizeof(float));
      a.center = reinterpret_cast<const float*>(base + at_center);
    }
    if (e != hipSuccess) return hip_failed(op.c_str(), e);

    e = launch_trace_order(a, nullptr);
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(unsigned) == sizeof(float), "n and out are copied as they are");
    if (e == hipSuccess) e = hipMemcpy(n, a.n, (size_t)n_traces * sizeof(long long), hipMemcpyDeviceToHost);      // (waits)
    if (e == hipSuccess) e = hipMemcpy(out, a.out, (size_t)n_states * sizeof(unsigned), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_failed(op.c_str(), e);
    return (int)GCWT_OK;
  });
}

}  // extern "C"
