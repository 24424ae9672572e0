// trace_order.h -- exact order statistics of float32 traces on the device (include/ghostcwt.h: gcwt_trace_order).
// trace_order.cpp checks the arguments, owns the work arrays and launches; trace_order.hip does the work: a radix select
// from the most significant digit down over ord(key), the 32-bit pattern whose unsigned order is the order of the keys.
//
// kOrderPasses passes of kOrderDigitBits bits (11 / 11 / 10).  Each pass is two kernels:
//   k_order_hist  a workgroup takes one (trace, chunk of kOrderChunkTiles tiles of kRunCols columns): unit = trace *
//                 n_chunks + chunk.  It counts, in LDS, the pass's digit of every included column whose higher digits
//                 are those already chosen for a rank -- one histogram per rank; in the first pass nothing is chosen yet
//                 and the ranks share one -- and adds the bins that are not 0 to the trace's histogram in global memory
//                 (integer atomics: the sums are exact in any order)
//   k_order_pick  a workgroup per (trace, rank): scans the bins, finds the one that holds the rank, appends its digit to
//                 the rank's prefix and takes the columns below it off the rank.  The first pass's total is n.
// Prefixes and remaining ranks stay on the device (OrderState); six launches whatever the data; n and the values come
// to the host at the end.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "detect_runs.h"

namespace gcwt {

constexpr int kOrderChunkTiles = 8;                                  // tiles of kRunCols columns a workgroup walks
constexpr int kOrderChunkCols = kOrderChunkTiles * kRunCols;
constexpr int kOrderMaxRanks = 4;
constexpr int kOrderPasses = 3;
constexpr int kOrderBins = 2048;                                     // of the widest digit
constexpr int kOrderCopies = 4;                                      // first pass: copies of the one histogram, by lane
constexpr unsigned kOrderNoValue = 0x7fc00000u;                      // what a rank >= n returns

__host__ __device__ constexpr int order_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__host__ __device__ constexpr int order_bins(int pass) { return pass == 2 ? 1024 : 2048; }

struct OrderState {            // of one (trace, rank)
  unsigned prefix;             // the digits chosen so far, in place; the lower bits 0
  int active;                  // 0: the rank is >= n
  long long rank;              // among the included columns that share the prefix
};

struct OrderArgs {
  TraceArgs t;
  const float* center;         // device copy: n_traces centres, or NULL
  int32_t n_ranks;
  int64_t n_chunks;            // per trace
  unsigned long long* hist[kOrderPasses];   // pass 0: [n_traces][kOrderBins]; later: [n_traces][n_ranks][kOrderBins]; zeroed
  OrderState* state;           // [n_traces][n_ranks]
  long long* n;                // [n_traces]
  unsigned* out;               // [n_traces][n_ranks] bit patterns
};

// the six launches
hipError_t launch_trace_order(const OrderArgs& a, hipStream_t st);

}  // namespace gcwt
