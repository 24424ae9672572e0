// trace_smooth.hip -- the kernel of gcwt_trace_smooth (include/ghostcwt.h has the definition; trace_smooth.h how the
// work is cut; profiles/smooth.md).  Per output column c of a segment [a, b), every operation one correctly rounded
// float32 one, a term whose column lies outside [a, b) an exact 0.f:
//   acc = w_0 * v[c];   acc = fmaf(w_k, v[c - k] + v[c + k], acc) for k = 1 .. half in ascending order
// The chain of a column runs inside one lane and reads nothing but its own segment's columns and the taps: no atomics,
// no cross-lane sums, and the same bits whatever the tile, the pitch, the width of the loads or the other traces are.
//
// A workgroup of four waves takes one output trace and a tile of kSmCols columns.  It stages the tile and `halo` columns
// on either side (half rounded up to 4) in LDS, 0.f where the trace has no column; with members, the traces of the list
// are added in the list's order and scaled on the way in.  Loads are 16 bytes where the rows start on 16 bytes
// (`aligned`, which the Python layer's pitches always give), else one per column (detect_runs.h: load_cols).  A lane
// owns kSmLaneCols adjacent outputs and slides a window of 8 values to the left and one to the right through its
// registers: per 4 taps one aligned 16-byte LDS read per side -- lane l reads bytes 16 l .. 16 l + 15 of a contiguous
// run, which no two lanes of a group share a bank for -- and the 4 taps as one scalar load through the constant address
// space.  A tile whose whole window lies inside one segment takes the instantiation without segment tests; in any other
// each lane looks up the segment of each of its columns and a term past the segment's end is replaced by 0.f with a
// select, so a NaN or an inf beyond the end never enters.
#include <hip/hip_runtime.h>

#include "resident_op.h"
#include "trace_smooth.h"

namespace gcwt {

namespace {

// the segment that holds column c, or an empty one
__device__ __forceinline__ longlong2 segment_of(const SmoothArgs& a, int64_t c) {
  const Const<longlong2> seg = constant(a.segments);
  int64_t lo = 0, hi = a.n_segments;                         // lo: the segments that start at or before c
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (seg[mid].x <= c) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return make_longlong2(0, 0);
  const long long start = seg[lo - 1].x, stop = seg[lo - 1].y;
  return c < stop ? make_longlong2(start, stop) : make_longlong2(0, 0);
}

// x[i] = column first - halo + i of the (combined) trace, i < kSmCols + 2 halo; 0.f before column 0 and from n_cols on
__device__ __forceinline__ void stage(const SmoothArgs& a, int64_t trace, int64_t first, float4* x4) {
  const int n_quads = (kSmCols + 2 * a.halo) / kSmLaneCols;
  const Const<int32_t> members = constant(a.members);
  for (int q = threadIdx.x; q < n_quads; q += kSmThreads) {
    const int64_t c = first - a.halo + (int64_t)q * kSmLaneCols;       // a multiple of 4: below 0 with all its columns
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c >= 0 && c < a.t.n_cols) {
      if (a.n_members > 0) {
        Cols v = load_cols(a.t, a.t.trace + (int64_t)members[0] * a.t.pitch, c);
        for (int i = 1; i < a.n_members; ++i) {
          const Cols u = load_cols(a.t, a.t.trace + (int64_t)members[i] * a.t.pitch, c);
#pragma unroll
          for (int j = 0; j < kSmLaneCols; ++j) v.v[j] = __fadd_rn(v.v[j], u.v[j]);
        }
#pragma unroll
        for (int j = 0; j < kSmLaneCols; ++j) v.v[j] = __fmul_rn(v.v[j], a.inv_members);
        s = make_float4(v.v[0], v.v[1], v.v[2], v.v[3]);
      } else {
        const Cols v = load_cols(a.t, a.t.trace + trace * a.t.pitch, c);
        s = make_float4(v.v[0], v.v[1], v.v[2], v.v[3]);
      }
    }
    x4[q] = s;
  }
}

// The taps k = 4 m + 1 .. 4 m + count of the lane's four chains (WHOLE: count is 4).  lo = x[4 (q0 - m) ..] and hi =
// x[4 (q0 + m) ..], the nearer halves of the left and the right window, move on by one 16-byte read each.
template <bool CLIP, bool WHOLE>
__device__ __forceinline__ void four_taps(float (&acc)[kSmLaneCols], float (&lo)[kSmLaneCols], float (&hi)[kSmLaneCols],
                                          const float4* x4, int q0, Const<float> taps, int m, int count,
                                          const int (&kl)[kSmLaneCols], const int (&kr)[kSmLaneCols]) {
  const float4 nl = x4[q0 - m - 1], nr = x4[q0 + m + 1];
  const float w[kSmLaneCols] = {taps[4 * m], taps[4 * m + 1], taps[4 * m + 2], taps[4 * m + 3]};   // (16 bytes, on 16)
  const float l[2 * kSmLaneCols] = {nl.x, nl.y, nl.z, nl.w, lo[0], lo[1], lo[2], lo[3]};    // x[4 (q0 - m - 1) ..]
  const float r[2 * kSmLaneCols] = {hi[0], hi[1], hi[2], hi[3], nr.x, nr.y, nr.z, nr.w};    // x[4 (q0 + m) ..]
#pragma unroll
  for (int i = 1; i <= kSmLaneCols; ++i) {
    if (!WHOLE && i > count) break;                          // (uniform)
    const int k = m * kSmLaneCols + i;
#pragma unroll
    for (int j = 0; j < kSmLaneCols; ++j) {
      float vl = l[kSmLaneCols + j - i], vr = r[j + i];      // columns c0 + j - k and c0 + j + k
      if (CLIP) {
        vl = k > kl[j] ? 0.f : vl;
        vr = k > kr[j] ? 0.f : vr;
      }
      acc[j] = fmaf(w[i - 1], __fadd_rn(vl, vr), acc[j]);
    }
  }
  lo[0] = nl.x; lo[1] = nl.y; lo[2] = nl.z; lo[3] = nl.w;
  hi[0] = nr.x; hi[1] = nr.y; hi[2] = nr.z; hi[3] = nr.w;
}

// CLIP: some column of the tile's window lies outside the segment of some output, or past n_cols
template <bool CLIP>
__device__ __forceinline__ void smooth_tile(const SmoothArgs& a, int64_t trace, int64_t first, const float4* x4) {
  const int q0 = a.halo / kSmLaneCols + (int)threadIdx.x;    // the lane's outputs: x[4 q0 .. 4 q0 + 3]
  const int64_t c0 = first + (int64_t)threadIdx.x * kSmLaneCols;
  int kl[kSmLaneCols], kr[kSmLaneCols];                      // the last tap whose left / right term is inside the segment
  bool live[kSmLaneCols];
#pragma unroll
  for (int j = 0; j < kSmLaneCols; ++j) {
    kl[j] = kr[j] = a.half; live[j] = true;
    if (CLIP) {
      const longlong2 s = segment_of(a, c0 + j);
      live[j] = s.x < s.y;
      kl[j] = live[j] ? (int)min((long long)a.half, c0 + j - s.x) : 0;
      kr[j] = live[j] ? (int)min((long long)a.half, s.y - 1 - (c0 + j)) : 0;
    }
  }

  const float4 centre = x4[q0];
  float lo[kSmLaneCols] = {centre.x, centre.y, centre.z, centre.w};   // x[4 (q0 - m) ..]: the nearer half of the left window
  float hi[kSmLaneCols] = {centre.x, centre.y, centre.z, centre.w};   // x[4 (q0 + m) ..]: ... of the right one
  float acc[kSmLaneCols];
#pragma unroll
  for (int j = 0; j < kSmLaneCols; ++j) acc[j] = __fmul_rn(a.w0, lo[j]);

  const Const<float> taps = constant(a.taps);
  const int n_whole = a.half / kSmLaneCols;                  // blocks of 4 taps; then one of half % 4
  for (int m = 0; m < n_whole; ++m) four_taps<CLIP, true>(acc, lo, hi, x4, q0, taps, m, kSmLaneCols, kl, kr);
  if (a.half % kSmLaneCols) four_taps<CLIP, false>(acc, lo, hi, x4, q0, taps, n_whole, a.half % kSmLaneCols, kl, kr);

  if (c0 >= a.t.n_cols) return;
#pragma unroll
  for (int j = 0; j < kSmLaneCols; ++j)
    if (!live[j]) acc[j] = 0.f;                              // a column in no segment
  float* o = a.out + trace * a.out_pitch + c0;
  if (a.out_aligned && c0 + kSmLaneCols <= a.t.n_cols) {     // (c0 is a multiple of 4, out_pitch too)
    *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int j = 0; j < kSmLaneCols; ++j)
      if (c0 + j < a.t.n_cols) o[j] = acc[j];
  }
}

__global__ void __launch_bounds__(kSmThreads) k_trace_smooth(SmoothArgs a) {
  extern __shared__ float4 x4[];                             // smooth_lds_bytes(a)
  const int64_t unit = blockIdx.x;                           // (the grid has exactly n_out * n_tiles workgroups)
  const int64_t trace = unit / a.t.n_tiles, first = unit % a.t.n_tiles * kSmCols;
  stage(a, trace, first, x4);
  __syncthreads();
  const longlong2 s = segment_of(a, first);                  // (uniform)
  if (s.x <= first - a.half && first + kSmCols + a.half <= s.y) smooth_tile<false>(a, trace, first, x4);
  else smooth_tile<true>(a, trace, first, x4);
}

}  // namespace

hipError_t launch_trace_smooth(const SmoothArgs& a, hipStream_t st) {
  const int64_t blocks = a.n_out * a.t.n_tiles;
  if (blocks <= 0 || blocks > 0x7fffffff || a.half < 0 || a.half > kSmMaxHalf || a.halo < a.half || a.halo % kSmLaneCols ||
      a.halo > kSmMaxHalf || a.n_segments < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_trace_smooth, dim3((unsigned)blocks), dim3(kSmThreads), smooth_lds_bytes(a), st, a);
  return hipGetLastError();
}

}  // namespace gcwt
