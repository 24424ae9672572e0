// bandpass.hip -- band-limited analytic signals from the rows of a resident complex result (include/ghostcwt.h:
// gcwt_bandpass; profiles/bandpass.md).  A band is a run of rows first .. first + R - 1; g and h are per-row weights.
// For a channel c, a band and a column t, with w_r = W[c, r, t], the rows in ascending r and each sum from an exact 0.f:
//   re = fmaf(g[r], w_r.re, re);  im = fmaf(g[r], w_r.im, im);  p = fmaf(h[r], norm2(w_r), p);
//   analytic = (re, im);  envelope = modulus(analytic);  power = p.
// Every operation is a single correctly rounded float32 one (wave_reduce.h: norm2, modulus; explicit fmaf; no
// fast-math).  No atomics, no cross-lane sums, no LDS: a cell's chain runs along the rows of its band inside one lane
// and depends on nothing else -- not on the other bands of the list or their order, not on the column count or the
// tiling, not on the width of the loads.  Columns that are zero (the gaps between epochs) stay exact zeros.
//
// The cut: a workgroup of four waves takes one channel, a tile of kBpCols columns and a group of up to kBpBands
// consecutive bands of the list.  A lane owns two adjacent columns outright: 3 accumulators per band and column.  The
// workgroup walks the rows from the group's lowest to its highest; a row that no band of the group holds is skipped
// and every other one is read once, however many of the bands hold it -- 16 bytes per lane where rows and output rows
// start on 16 bytes (`aligned`, which the Python layer's pitches always give), else 8 bytes per column.  kBpDepth rows'
// loads are in flight.  Which bands a row enters is a wave-uniform test on the band table, which like the weights is
// read with scalar loads.  A load may reach one column into a row's padding (never past pitch); what it brings is
// never stored.  A tile whose columns all exist takes an instantiation without column tests.
//
// The grid: the band groups of one (channel, column tile) read the same columns of neighbouring rows and are placed to
// meet them in one L2 (resident_op.h: the placement).  This is for speed only; nothing depends on it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bandpass.h"
#include "wave_reduce.h"

namespace gcwt {

namespace {

constexpr int kBpDepth = 4;                                 // rows whose loads are in flight

struct Acc { float re, im, p; };

// one row enters the chains of one column: the prescribed sequence
__device__ __forceinline__ void add_row(Acc& s, float g, float h, float2 w, float r2) {
  s.re = fmaf(g, w.x, s.re);
  s.im = fmaf(g, w.y, s.im);
  s.p = fmaf(h, r2, s.p);
}

// FULL: all kBpCols columns of the tile exist.  ALIGNED: BpArgs::aligned
template <bool FULL, bool ALIGNED>
__device__ __forceinline__ void run_tile(const BpArgs& a, int ch, int grp, int64_t ct) {
  const int64_t c0 = ct * kBpCols + (int64_t)threadIdx.x * kBpLaneCols;        // this lane's columns: c0 and c0 + 1
  const bool ok0 = FULL || c0 < a.n_cols, ok1 = FULL || c0 + 1 < a.n_cols;

  // the group's bands, as [first, end); a band the list does not have is empty
  const Const<int2> bands = constant(a.bands);
  const Const<float> wg = constant(a.g), wh = constant(a.h);
  int first[kBpBands], end[kBpBands];
  int r_lo = a.n_scales, r_hi = 0;
#pragma unroll
  for (int k = 0; k < kBpBands; ++k) {
    const int b = grp * kBpBands + k;
    first[k] = end[k] = 0;
    if (b < a.n_bands) {
      const int fc_first = bands[b].x, fc_count = bands[b].y;
      first[k] = fc_first;
      end[k] = fc_first + fc_count;
      r_lo = std::min(r_lo, first[k]);
      r_hi = std::max(r_hi, end[k]);
    }
  }

  Acc s[kBpBands][kBpLaneCols];
#pragma unroll
  for (int k = 0; k < kBpBands; ++k)
#pragma unroll
    for (int j = 0; j < kBpLaneCols; ++j) s[k][j] = Acc{0.f, 0.f, 0.f};

  // ALIGNED: pitch is even and c0 is, so c0 < n_cols <= pitch puts c0 + 1 inside the row's pitch
  const float2* base = a.rows + (int64_t)ch * a.n_scales * a.pitch + c0;
  for (int r = r_lo; r < r_hi; r += kBpDepth) {
    float4 v[kBpDepth];
    bool used[kBpDepth];
#pragma unroll
    for (int i = 0; i < kBpDepth; ++i) {
      used[i] = false;
#pragma unroll
      for (int k = 0; k < kBpBands; ++k) used[i] |= r + i >= first[k] && r + i < end[k];
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
    for (int i = 0; i < kBpDepth; ++i) {
      if (!used[i]) continue;
      const float g = wg[r + i], h = wh[r + i];
      const float2 w0 = make_float2(v[i].x, v[i].y), w1 = make_float2(v[i].z, v[i].w);
      const float n0 = norm2(w0), n1 = norm2(w1);
#pragma unroll
      for (int k = 0; k < kBpBands; ++k)
        if (r + i >= first[k] && r + i < end[k]) {
          add_row(s[k][0], g, h, w0, n0);
          add_row(s[k][1], g, h, w1, n1);
        }
    }
  }

  if (!ok0) return;
#pragma unroll
  for (int k = 0; k < kBpBands; ++k) {
    const int b = grp * kBpBands + k;
    if (b >= a.n_bands) break;
    const int64_t o = ((int64_t)ch * a.n_bands + b) * a.out_pitch + c0;
    const float2 z0 = make_float2(s[k][0].re, s[k][0].im), z1 = make_float2(s[k][1].re, s[k][1].im);
    if (ALIGNED && ok1) {                                    // (o is even: out_pitch and c0 are)
      if (a.analytic) *reinterpret_cast<float4*>(a.analytic + o) = make_float4(z0.x, z0.y, z1.x, z1.y);
      if (a.envelope) *reinterpret_cast<float2*>(a.envelope + o) = make_float2(modulus(z0), modulus(z1));
      if (a.power) *reinterpret_cast<float2*>(a.power + o) = make_float2(s[k][0].p, s[k][1].p);
    } else {
      if (a.analytic) a.analytic[o] = z0;
      if (a.envelope) a.envelope[o] = modulus(z0);
      if (a.power) a.power[o] = s[k][0].p;
      if (ok1) {
        if (a.analytic) a.analytic[o + 1] = z1;
        if (a.envelope) a.envelope[o + 1] = modulus(z1);
        if (a.power) a.power[o + 1] = s[k][1].p;
      }
    }
  }
}

__global__ void __launch_bounds__(kBpThreads) k_bandpass(BpArgs a) {
  const TileOfUnit at = shared_place(a.n_groups);            // unit = (channel, column tile)
  if (at.unit >= a.n_units) return;                          // (the last group's padding)
  const int grp = at.tile, ch = (int)(at.unit / a.n_ctiles);
  const int64_t ct = at.unit % a.n_ctiles;
  const bool full = (ct + 1) * kBpCols <= a.n_cols;
  if (a.aligned) {
    if (full) run_tile<true, true>(a, ch, grp, ct);
    else run_tile<false, true>(a, ch, grp, ct);
  } else {
    if (full) run_tile<true, false>(a, ch, grp, ct);
    else run_tile<false, false>(a, ch, grp, ct);
  }
}

}  // namespace

hipError_t launch_bandpass(const BpArgs& a, hipStream_t st) {
  const int64_t blocks = bandpass_blocks(a);
  if (blocks <= 0 || blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_bandpass, dim3((unsigned)blocks), dim3(kBpThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace gcwt
