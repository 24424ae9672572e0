// trace_order.hip -- the kernels of gcwt_trace_order (include/ghostcwt.h has the definition; trace_order.h how the work
// is cut).  Columns are read as in detect_runs.hip: kRunCols columns to a workgroup of four waves, a lane on kRunLaneCols
// adjacent ones.  Everything counted is an integer, so no result depends on the order of the atomic adds.
//
// The first pass's digit is the sign, the exponent and two bits of the mantissa: a trace that spans a few octaves puts
// nearly every column into a handful of bins.  Two things keep the lanes of a wave off one LDS word there: a lane adds a
// run of equal digits among its own columns (adjacent columns, and the same lane's columns of the next tile) as one
// number, and it adds to copy lane % kOrderCopies of the histogram, the copies of a bin in adjacent banks.
#include <hip/hip_runtime.h>

#include "trace_order.h"

namespace gcwt {

namespace {

constexpr int kWaves = kRunThreads / 64;
static_assert(kOrderCopies * kOrderBins == kOrderMaxRanks * kOrderBins, "one LDS array serves both layouts");
static_assert(kOrderChunkCols < (1 << 30), "a chunk's counts fit 32 bits");

__device__ __forceinline__ unsigned ord_of(unsigned bits) { return bits ^ (bits >> 31 ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ unsigned bits_of_ord(unsigned o) { return o >> 31 ? o ^ 0x80000000u : ~o; }

template <int PASS>
__global__ void __launch_bounds__(kRunThreads) k_order_hist(OrderArgs a) {
  __shared__ unsigned h[kOrderMaxRanks * kOrderBins];        // pass 0: [bin][copy]; later: [rank][bin]
  constexpr int kShift = order_shift(PASS), kBins = order_bins(PASS);
  constexpr int kAbove = PASS == 0 ? 0 : order_shift(PASS - 1);     // the bits from here up are the prefix
  const int64_t unit = blockIdx.x;                           // (the grid has exactly n_traces * n_chunks workgroups)
  const int64_t trace = unit / a.n_chunks, chunk = unit % a.n_chunks;
  const float* row = a.t.trace + trace * a.t.pitch;
  const bool centred = a.center != nullptr;
  const float centre = centred ? a.center[trace] : 0.f;

  unsigned prefix[kOrderMaxRanks];
  bool active[kOrderMaxRanks];
#pragma unroll
  for (int r = 0; r < kOrderMaxRanks; ++r) {
    active[r] = false; prefix[r] = 0;
    if (PASS > 0 && r < a.n_ranks) {
      const OrderState s = a.state[trace * a.n_ranks + r];
      active[r] = s.active != 0; prefix[r] = s.prefix >> kAbove;
    }
  }
  for (int i = threadIdx.x; i < kOrderMaxRanks * kOrderBins; i += kRunThreads) h[i] = 0;
  __syncthreads();

  const int copy = threadIdx.x % kOrderCopies;
  unsigned run_digit = 0, run = 0;                           // pass 0: the lane's current run of equal digits
  const int64_t first = chunk * kOrderChunkCols;
  for (int tile = 0; tile < kOrderChunkTiles; ++tile) {
    const int64_t c0 = first + (int64_t)tile * kRunCols + (int64_t)threadIdx.x * kRunLaneCols;
    if (first + (int64_t)tile * kRunCols >= a.t.n_cols) break;
    const Cols c = load_cols(a.t, row, c0);                  // 0, which is excluded, at and past n_cols
#pragma unroll
    for (int j = 0; j < kRunLaneCols; ++j) {
      const unsigned vb = __float_as_uint(c.v[j]);
      if ((vb & 0x7fffffffu) == 0) continue;                 // v == 0 under the IEEE comparison; a NaN stays
      const unsigned kb = centred ? __float_as_uint(__fsub_rn(c.v[j], centre)) & 0x7fffffffu : vb;
      const unsigned o = ord_of(kb);
      if (PASS == 0) {
        const unsigned d = o >> kShift;
        if (run && d == run_digit) { ++run; continue; }
        if (run) atomicAdd(&h[run_digit * kOrderCopies + copy], run);
        run_digit = d; run = 1;
      } else {
        const unsigned d = (o >> kShift) & (kBins - 1), above = o >> kAbove;
#pragma unroll
        for (int r = 0; r < kOrderMaxRanks; ++r)
          if (active[r] && above == prefix[r]) atomicAdd(&h[r * kOrderBins + d], 1u);
      }
    }
  }
  if (PASS == 0 && run) atomicAdd(&h[run_digit * kOrderCopies + copy], run);
  __syncthreads();

  if (PASS == 0) {
    unsigned long long* g = a.hist[0] + trace * kOrderBins;
    for (int b = threadIdx.x; b < kBins; b += kRunThreads) {
      unsigned s = 0;
#pragma unroll
      for (int k = 0; k < kOrderCopies; ++k) s += h[b * kOrderCopies + k];
      if (s) atomicAdd(&g[b], (unsigned long long)s);
    }
  } else {
    for (int r = 0; r < a.n_ranks; ++r) {
      if (!active[r]) continue;
      unsigned long long* g = a.hist[PASS] + (trace * a.n_ranks + r) * kOrderBins;
      for (int b = threadIdx.x; b < kBins; b += kRunThreads) {
        const unsigned s = h[r * kOrderBins + b];
        if (s) atomicAdd(&g[b], (unsigned long long)s);
      }
    }
  }
}

// One workgroup per (trace, rank).  A lane holds kBins / kRunThreads consecutive bins; an inclusive scan over the lanes
// of a wave, the waves' totals through LDS.  Exactly one lane holds the bin of the rank, and it alone writes the state.
template <int PASS>
__global__ void __launch_bounds__(kRunThreads) k_order_pick(OrderArgs a) {
  __shared__ long long part[kWaves];
  constexpr int kBins = order_bins(PASS), kMine = kBins / kRunThreads;
  const int64_t idx = blockIdx.x, trace = idx / a.n_ranks;
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  const OrderState s = a.state[idx];
  if (!s.active) {                                           // (uniform over the workgroup; never in pass 0)
    if (PASS == kOrderPasses - 1 && threadIdx.x == 0) a.out[idx] = kOrderNoValue;
    return;
  }
  const unsigned long long* g = a.hist[PASS] + (PASS == 0 ? trace : idx) * kOrderBins + threadIdx.x * kMine;
  long long c[kMine], mine = 0;
#pragma unroll
  for (int k = 0; k < kMine; ++k) { c[k] = (long long)g[k]; mine += c[k]; }
  long long incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long x = __shfl_up(incl, d);
    if (lane >= d) incl += x;
  }
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  long long before = incl - mine, total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) before += part[w];
    total += part[w];
  }
  if (PASS == 0 && idx % a.n_ranks == 0 && threadIdx.x == 0) a.n[trace] = total;
  if (s.rank >= total) {                                     // (uniform; after pass 0 the rank is inside by construction)
    if (threadIdx.x == 0) {
      a.state[idx].active = 0;
      if (PASS == kOrderPasses - 1) a.out[idx] = kOrderNoValue;
    }
    return;
  }
  if (s.rank < before || s.rank >= before + mine) return;
  long long at = before;
#pragma unroll
  for (int k = 0; k < kMine; ++k) {
    if (s.rank >= at && s.rank < at + c[k]) {
      const unsigned prefix = s.prefix | ((unsigned)(threadIdx.x * kMine + k) << order_shift(PASS));
      OrderState next;
      next.prefix = prefix; next.active = 1; next.rank = s.rank - at;
      a.state[idx] = next;
      if (PASS == kOrderPasses - 1) a.out[idx] = bits_of_ord(prefix);
    }
    at += c[k];
  }
}

bool launchable(int64_t blocks) { return blocks > 0 && blocks <= 0x7fffffff; }

template <int PASS>
hipError_t launch_pass(const OrderArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_order_hist<PASS>, dim3((unsigned)(a.t.n_traces * a.n_chunks)), dim3(kRunThreads), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_order_pick<PASS>, dim3((unsigned)(a.t.n_traces * a.n_ranks)), dim3(kRunThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_trace_order(const OrderArgs& a, hipStream_t st) {
  if (a.n_ranks < 1 || a.n_ranks > kOrderMaxRanks || !launchable(a.t.n_traces * a.n_chunks) || !launchable(a.t.n_traces * a.n_ranks))
    return hipErrorInvalidValue;
  hipError_t e = launch_pass<0>(a, st);
  if (e == hipSuccess) e = launch_pass<1>(a, st);
  if (e == hipSuccess) e = launch_pass<2>(a, st);
  return e;
}

}  // namespace gcwt
