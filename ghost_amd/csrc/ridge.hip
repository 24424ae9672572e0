// ridge.hip -- the spectral ridge of a band of a resident complex result and the instantaneous frequency on it
// (include/ghostcwt.h: gcwt_ridge; profiles/ridge.md).  A band is a run of rows first .. first + R - 1; e[r] > 0 is a
// per-row weight that makes rows comparable, nu[r] the phase advance that row r expects per column.  For a channel c, a
// band and a column t, every operation a single correctly rounded float32 one (wave_reduce.h: norm2; no fast-math, no
// contraction: the products, sums and quotients below are __fmul_rn, __fadd_rn, __fsub_rn, __fdiv_rn):
//   q_r = e[r] * norm2(W[c, r, t]), the rows walked in ascending r; the winner is the first row whose q is larger than
//     every earlier one and than 0 -- the lowest index among equal maxima; no winner where every q_r is 0 (a gap)
//   row = the winner's index, or -1;   amplitude = sqrt(q_win), 0 with no winner
//   offset: with qm, qp the q of rows row - 1, row + 1:  d1 = qm - qp;  s = qm + qp;  d2 = s - 2 * q_win;
//     offset = (0.5f * d1) / d2;  exactly 0 where the winner is the band's first or last row, d2 == 0, or no winner
//   frequency: tm = max(t - 1, seg.start), tp = min(t + 1, seg.stop - 1) inside the segment of t, span = tp - tm,
//     a = W[c, row, tp], b = W[c, row, tm]:
//       re = fmaf(a.x, b.x, a.y * b.y);   im = fmaf(a.y, b.x, -(a.x * b.y));   dphi = atan2f(im, re)
//       k = rintf(((float)span * nu[row] - dphi) / kTwoPi)                       3 roundings, then the integer
//       num = dphi + kTwoPi * k                                                  2 roundings
//       scale = hz_per_cycle / (kTwoPi * (float)span)                            the product is exact (span is 1 or 2); 1
//       frequency = num * scale                                                  1
//     with kTwoPi = float32(2 pi); NaN where row == -1, span == 0, or re and im are both 0.
// No atomics, no cross-lane traffic, no LDS: the state of a cell runs along the rows of its band inside one lane, and the
// cell depends on nothing but its own band's rows at the columns tm, t and tp -- not on the other bands of the list or
// their order, not on the column count, the pitch or the tiling, not on the width of the loads, not on which outputs are
// asked for.  A band gives the same bits alone and among any others, and two runs agree in bits.
//
// The cut is bandpass.hip's: a workgroup of four waves takes one channel, a tile of kRgCols columns and a group of up to
// kRgBands consecutive bands of the list; a lane owns two adjacent columns.  The workgroup walks the rows from the
// group's lowest to its highest; a row that no band of the group holds is skipped and every other one is read once,
// however many of the bands hold it -- 16 bytes per lane where rows and output rows start on 16 bytes (`aligned`), else
// 8 bytes per column; kRgDepth rows' loads are in flight.  The band table, e and nu are read through the constant address
// space.  Per (band, column) the lane carries the best q, its row, qm and qp; "the winner so far is the row before this
// one" says that this row's q is its qp.  The q of the row before is carried per column: it does not depend on the band,
// and a band's rows are consecutive, so for every row but a band's first it is the q of that band's row below (what a
// band's first row takes for qm is never used: there the offset is 0).  After the walk the lane fetches the two
// neighbours of each winner, a and b, from global memory -- gathers into lines that the tile, or the tile beside it,
// has just read -- and finds the segment of its first column by a binary search of the table; its second column lies in
// the same segment or in the next.  Without `frequency` neither the search nor the gathers nor the arctangent are made.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "phase_advance.h"
#include "ridge.h"
#include "wave_reduce.h"

// A product and the sum it feeds stay two roundings unless the code says fmaf (__fmul_rn and its kin are plain operators
// here, which the compiler's default would contract).
#pragma clang fp contract(off)

namespace gcwt {

namespace {

constexpr int kRgDepth = 4;                                 // rows whose loads are in flight

struct Best { float q, qm, qp; int row; };

// row r enters the ranking of one (band, column); q_below: the q of row r - 1 at this column
__device__ __forceinline__ void rank_row(Best& s, int r, float q, float q_below) {
  if (s.row == r - 1) s.qp = q;        // (before any winner row is -1: at r = 0 this sets a qp that nothing reads)
  if (q > s.q) { s.q = q; s.row = r; s.qm = q_below; }
}

__device__ __forceinline__ float ridge_offset(const Best& s, int first, int end) {
  if (!(s.row > first && s.row < end - 1)) return 0.f;       // the band's first or last row, or no winner
  const float d1 = __fsub_rn(s.qm, s.qp), sum = __fadd_rn(s.qm, s.qp);
  const float d2 = __fsub_rn(sum, __fmul_rn(2.f, s.q));
  return d2 == 0.f ? 0.f : __fdiv_rn(__fmul_rn(0.5f, d1), d2);
}

// chan: the channel's rows; [start, stop): the segment of column t, which holds it (phase_advance.h has the arithmetic)
__device__ __forceinline__ float ridge_frequency(const RgArgs& a, const float2* chan, Const<float> nu, int row, int64_t t,
                                                 int64_t start, int64_t stop) {
  if (row < 0) return __builtin_nanf("");
  const int64_t tm = std::max(t - 1, start), tp = std::min(t + 1, stop - 1);   // (start <= t < stop <= n_cols)
  const int span = (int)(tp - tm);
  if (span == 0) return __builtin_nanf("");
  const float2* w = chan + (int64_t)row * a.pitch;
  return phase_advance_hz(w[tp], w[tm], span, nu[row], a.hz_per_cycle);
}

// FULL: all kRgCols columns of the tile exist.  ALIGNED: RgArgs::aligned
template <bool FULL, bool ALIGNED>
__device__ __forceinline__ void run_tile(const RgArgs& a, int ch, int grp, int64_t ct) {
  const int64_t c0 = ct * kRgCols + (int64_t)threadIdx.x * kRgLaneCols;        // this lane's columns: c0 and c0 + 1
  const bool ok0 = FULL || c0 < a.n_cols, ok1 = FULL || c0 + 1 < a.n_cols;

  // the group's bands, as [first, end); a band the list does not have is empty
  const Const<int2> bands = constant(a.bands);
  const Const<float> we = constant(a.e);
  int first[kRgBands], end[kRgBands];
  int r_lo = a.n_scales, r_hi = 0;
#pragma unroll
  for (int k = 0; k < kRgBands; ++k) {
    const int b = grp * kRgBands + k;
    first[k] = end[k] = 0;
    if (b < a.n_bands) {
      const int fc_first = bands[b].x, fc_count = bands[b].y;
      first[k] = fc_first;
      end[k] = fc_first + fc_count;
      r_lo = std::min(r_lo, first[k]);
      r_hi = std::max(r_hi, end[k]);
    }
  }

  Best s[kRgBands][kRgLaneCols];
#pragma unroll
  for (int k = 0; k < kRgBands; ++k)
#pragma unroll
    for (int j = 0; j < kRgLaneCols; ++j) s[k][j] = Best{0.f, 0.f, 0.f, -1};
  float below0 = 0.f, below1 = 0.f;                          // the q of the row read before this one, per column

  // ALIGNED: pitch is even and c0 is, so c0 < n_cols <= pitch puts c0 + 1 inside the row's pitch
  const float2* chan = a.rows + (int64_t)ch * a.n_scales * a.pitch;
  const float2* base = chan + c0;
  for (int r = r_lo; r < r_hi; r += kRgDepth) {
    float4 v[kRgDepth];
    bool used[kRgDepth];
#pragma unroll
    for (int i = 0; i < kRgDepth; ++i) {
      used[i] = false;
#pragma unroll
      for (int k = 0; k < kRgBands; ++k) used[i] |= r + i >= first[k] && r + i < end[k];
      v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (used[i]) {                                         // (wave-uniform; r + i < r_hi <= n_scales follows)
        const float2* row = base + (int64_t)(r + i) * a.pitch;
        if (ALIGNED) {
          if (ok0) v[i] = *reinterpret_cast<const float4*>(row);
        } else {
          if (ok0) { const float2 w = row[0]; v[i].x = w.x; v[i].y = w.y; }
          if (ok1) { const float2 w = row[1]; v[i].z = w.x; v[i].w = w.y; }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kRgDepth; ++i) {
      if (!used[i]) continue;
      const float er = we[r + i];
      const float q0 = __fmul_rn(er, norm2(make_float2(v[i].x, v[i].y)));
      const float q1 = __fmul_rn(er, norm2(make_float2(v[i].z, v[i].w)));
#pragma unroll
      for (int k = 0; k < kRgBands; ++k)
        if (r + i >= first[k] && r + i < end[k]) {
          rank_row(s[k][0], r + i, q0, below0);
          rank_row(s[k][1], r + i, q1, below1);
        }
      below0 = q0;
      below1 = q1;
    }
  }

  if (!ok0) return;
  // the segments of the two columns (host-checked: ascending, each starting where the one before stops, covering
  // [0, n_cols)): the last one that starts at or before c0, and for c0 + 1 that one or the next
  int64_t start0 = 0, stop0 = 0, start1 = 0, stop1 = 0;
  const Const<float> nu = constant(a.nu);
  if (a.frequency) {
    const Const<longlong2> seg = constant(a.segments);
    int64_t lo = 0, hi = a.n_segments - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (seg[mid].x <= c0) lo = mid; else hi = mid - 1;
    }
    start0 = start1 = seg[lo].x;
    stop0 = stop1 = seg[lo].y;
    if (ok1 && c0 + 1 >= stop0 && lo + 1 < a.n_segments) { start1 = seg[lo + 1].x; stop1 = seg[lo + 1].y; }
  }

#pragma unroll
  for (int k = 0; k < kRgBands; ++k) {
    const int b = grp * kRgBands + k;
    if (b >= a.n_bands) break;
    const int64_t o = ((int64_t)ch * a.n_bands + b) * a.out_pitch + c0;
    const Best &s0 = s[k][0], &s1 = s[k][1];
    float f0 = 0.f, f1 = 0.f;
    if (a.frequency) {
      f0 = ridge_frequency(a, chan, nu, s0.row, c0, start0, stop0);
      if (ok1) f1 = ridge_frequency(a, chan, nu, s1.row, c0 + 1, start1, stop1);
    }
    if (ALIGNED && ok1) {                                    // (o is even: out_pitch and c0 are)
      if (a.row) *reinterpret_cast<int2*>(a.row + o) = make_int2(s0.row, s1.row);
      if (a.amplitude) *reinterpret_cast<float2*>(a.amplitude + o) = make_float2(__builtin_sqrtf(s0.q), __builtin_sqrtf(s1.q));
      if (a.offset)
        *reinterpret_cast<float2*>(a.offset + o) = make_float2(ridge_offset(s0, first[k], end[k]), ridge_offset(s1, first[k], end[k]));
      if (a.frequency) *reinterpret_cast<float2*>(a.frequency + o) = make_float2(f0, f1);
    } else {
      if (a.row) a.row[o] = s0.row;
      if (a.amplitude) a.amplitude[o] = __builtin_sqrtf(s0.q);
      if (a.offset) a.offset[o] = ridge_offset(s0, first[k], end[k]);
      if (a.frequency) a.frequency[o] = f0;
      if (ok1) {
        if (a.row) a.row[o + 1] = s1.row;
        if (a.amplitude) a.amplitude[o + 1] = __builtin_sqrtf(s1.q);
        if (a.offset) a.offset[o + 1] = ridge_offset(s1, first[k], end[k]);
        if (a.frequency) a.frequency[o + 1] = f1;
      }
    }
  }
}

__global__ void __launch_bounds__(kRgThreads) k_ridge(RgArgs a) {
  const TileOfUnit at = shared_place(a.n_groups);            // unit = (channel, column tile)
  if (at.unit >= a.n_units) return;                          // (the last group's padding)
  const int grp = at.tile, ch = (int)(at.unit / a.n_ctiles);
  const int64_t ct = at.unit % a.n_ctiles;
  const bool full = (ct + 1) * kRgCols <= a.n_cols;
  if (a.aligned) {
    if (full) run_tile<true, true>(a, ch, grp, ct);
    else run_tile<false, true>(a, ch, grp, ct);
  } else {
    if (full) run_tile<true, false>(a, ch, grp, ct);
    else run_tile<false, false>(a, ch, grp, ct);
  }
}

}  // namespace

hipError_t launch_ridge(const RgArgs& a, hipStream_t st) {
  const int64_t blocks = ridge_blocks(a);
  if (blocks <= 0 || blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ridge, dim3((unsigned)blocks), dim3(kRgThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace gcwt
