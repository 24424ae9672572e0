// coherence.hip -- binned cross-spectra of channel pairs from a resident complex result (include/ghostcwt.h:
// gcwt_coherence; profiles/coherence.md).  With bins of `window` columns, for a pair (a, b) of channels, per scale
// and bin:  Sxy = sum W[a] conj(W[b]),  Sxx = sum |W[a]|^2,  Syy likewise;  cross = Sxy / cnt, power = Sxx / cnt,
// coherence = |Sxy|^2 / (Sxx Syy).
//
// Work is cut by channel tiles, not by pairs (coherence.cpp: coherence_tasks): a workgroup takes one (tile A, tile B,
// scale, run of bins), reads each of its at most 16 rows once and accumulates every wanted cell of the 8 x 8 tile pair
// in registers.  All pairs of 128 channels read 136 x 16 rows instead of 8128 x 2.
//
// The order of every sum is fixed and does not depend on the tiling: a bin belongs to ONE wave; lane l accumulates the
// bin's columns l, l + 64, ... one after the other (re = fma(ar, br, re); re = fma(ai, bi, re); im = fma(ai, br, im);
// im = fma(-ar, bi, im): 2 ceil(window / 64) roundings per component), then a six-level butterfly adds the 64 lanes
// (lane ^ 1, ^ 2, the other quad, the other 8, ^ 16, ^ 32 -- both partners add the same two numbers, so every lane ends
// with the same bits).  No atomics.  A pair asked for alone and the same pair among all pairs run the same
// instructions on the same numbers.  Power: |w|^2 = fma(im, im, re * re) per column, one add each into the lane's
// chain (ceil(window / 64) - 1 roundings), the same tree.
//
// Loads are 8 bytes per lane -- one complex column -- so a wave reads 512 contiguous bytes of a row per load.  16-byte
// loads would give a lane two adjacent columns (a chain of 2 ceil(window / 128) columns, longer than the order above
// for window <= 64 or 129 .. 192 ...) and bins start on odd columns whenever window is odd.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "coherence.h"
#include "wave_reduce.h"

namespace gcwt {

namespace {

constexpr int kWaves = 4;                                   // per workgroup; each takes every fourth bin of the run
constexpr int kRedFloats = 2 * kCohCells + 2 * kCohTile;    // a wave's reduced sums: (re, im) per cell, Sxx per row of A, of B

template <bool ALL>
__device__ __forceinline__ void run_task(const CohArgs& a, const CohTask& tk, int s, int64_t run, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool diag = tk.tile_a == tk.tile_b;
  const uint64_t cells = ALL ? ~0ull : tk.cells;
  const uint32_t rows_a = ALL ? 0xffu : tk.rows_a, rows_b = ALL ? 0xffu : tk.rows_b;
  const float2* row_a = a.rows + ((int64_t)tk.tile_a * kCohTile * a.n_scales + s) * a.pitch;
  const float2* row_b = a.rows + ((int64_t)tk.tile_b * kCohTile * a.n_scales + s) * a.pitch;
  const int64_t chan = (int64_t)a.n_scales * a.pitch;       // from a channel's row of this scale to the next channel's

  const int64_t m_end = std::min<int64_t>((run + 1) * a.run_bins, a.n_bins);
  for (int64_t m = run * a.run_bins + wave; m < m_end; m += kWaves) {
    const int64_t c_begin = m * a.window, c_end = std::min<int64_t>(c_begin + a.window, a.n_cols);
    float re[kCohCells], im[kCohCells], pa[kCohTile], pb[kCohTile];
#pragma unroll
    for (int k = 0; k < kCohCells; ++k) re[k] = im[k] = 0.f;
#pragma unroll
    for (int k = 0; k < kCohTile; ++k) pa[k] = pb[k] = 0.f;

    for (int64_t c0 = c_begin; c0 < c_end; c0 += 64) {
      const bool ok = c0 + lane < c_end;                     // (lanes past the bin add exact zeros)
      const float2* col_a = row_a + c0;                      // uniform: a wave's load is base + lane
      const float2* col_b = row_b + c0;
      float2 va[kCohTile], vb[kCohTile];
#pragma unroll
      for (int i = 0; i < kCohTile; ++i) {
        va[i] = make_float2(0.f, 0.f);
        if ((rows_a >> i) & 1)
          if (ok) va[i] = (col_a + i * chan)[lane];
      }
      if (diag) {
#pragma unroll
        for (int j = 0; j < kCohTile; ++j) vb[j] = va[j];
      } else {
#pragma unroll
        for (int j = 0; j < kCohTile; ++j) {
          vb[j] = make_float2(0.f, 0.f);
          if ((rows_b >> j) & 1)
            if (ok) vb[j] = (col_b + j * chan)[lane];
        }
      }
#pragma unroll
      for (int i = 0; i < kCohTile; ++i) {
        if ((rows_a >> i) & 1) pa[i] = __fadd_rn(pa[i], norm2(va[i]));
        if ((rows_b >> i) & 1) pb[i] = __fadd_rn(pb[i], norm2(vb[i]));
      }
#pragma unroll
      for (int i = 0; i < kCohTile; ++i) {
#pragma unroll
        for (int j = 0; j < kCohTile; ++j) {
          const int k = i * kCohTile + j;
          if (ALL || ((cells >> k) & 1)) {
            re[k] = fmaf(va[i].x, vb[j].x, re[k]);
            re[k] = fmaf(va[i].y, vb[j].y, re[k]);
            im[k] = fmaf(va[i].y, vb[j].x, im[k]);
            im[k] = fmaf(-va[i].x, vb[j].y, im[k]);
          }
        }
      }
    }

    // the tree; lane 0 leaves the sums in the wave's own piece of LDS for the lanes that write the outputs
#pragma unroll
    for (int k = 0; k < kCohCells; ++k) {
      if (ALL || ((cells >> k) & 1)) {
        const float r = wave_sum(re[k]), q = wave_sum(im[k]);
        if (lane == 0) { red[2 * k] = r; red[2 * k + 1] = q; }
      }
    }
#pragma unroll
    for (int k = 0; k < kCohTile; ++k) {
      if ((rows_a >> k) & 1) {
        const float r = wave_sum(pa[k]);
        if (lane == 0) red[2 * kCohCells + k] = r;
      }
      if ((rows_b >> k) & 1) {
        const float r = wave_sum(pb[k]);
        if (lane == 0) red[2 * kCohCells + kCohTile + k] = r;
      }
    }
    wave_lds_sync();

    const float cnt = (float)(c_end - c_begin);
    for (int e = lane; e < tk.n_entries; e += 64) {
      const CohEntry en = a.entries[tk.entry_first + e];
      const float r = red[2 * en.cell], q = red[2 * en.cell + 1];
      const float sxx = red[2 * kCohCells + en.cell / kCohTile];
      const float syy = red[2 * kCohCells + kCohTile + en.cell % kCohTile];
      const int64_t o = ((int64_t)en.out_row * a.n_scales + s) * a.out_pitch + m;
      if (a.cross) a.cross[o] = make_float2(r / cnt, (en.conjugate ? -q : q) / cnt);
      if (a.coherence) {
        const float den = sxx * syy;
        a.coherence[o] = den > 0.f ? fminf((r * r + q * q) / den, 1.f) : 0.f;
      }
    }
    if (a.power && lane < 2 * kCohTile) {
      const int side = lane / kCohTile;
      const int64_t ch = (int64_t)(side ? tk.tile_b : tk.tile_a) * kCohTile + lane % kCohTile;
      if (((tk.flags >> side) & 1) && ch < a.n_channels)
        a.power[(ch * a.n_scales + s) * a.out_pitch + m] = red[2 * kCohCells + lane] / cnt;
    }
    // (the next bin's sums go to the same piece of LDS: not before these reads)
    wave_lds_sync();
  }
}

__global__ void __launch_bounds__(64 * kWaves, 2) k_coherence(CohArgs a) {
  __shared__ float s_red[kWaves][kRedFloats];
  int64_t idx = blockIdx.x;                                  // task fastest: the tile pairs of one (scale, run) share rows
  const int t = (int)(idx % a.n_tasks);
  idx /= a.n_tasks;
  const int64_t run = idx % a.n_runs;
  const int s = (int)(idx / a.n_runs);
  const CohTask tk = a.tasks[t];
  float* red = s_red[threadIdx.x >> 6];
  if (tk.cells == ~0ull && tk.rows_a == 0xffu && tk.rows_b == 0xffu)
    run_task<true>(a, tk, s, run, red);
  else
    run_task<false>(a, tk, s, run, red);
}

}  // namespace

hipError_t launch_coherence(const CohArgs& a, hipStream_t st) {
  const int64_t blocks = (int64_t)a.n_tasks * a.n_runs * a.n_scales;
  if (blocks <= 0 || blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_coherence, dim3((unsigned)blocks), dim3(64 * kWaves), 0, st, a);
  return hipGetLastError();
}

}  // namespace gcwt
