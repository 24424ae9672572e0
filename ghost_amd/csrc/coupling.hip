// coupling.hip -- binned phase-amplitude coupling inside a channel of a resident complex result (include/ghostcwt.h:
// gcwt_coupling; profiles/coupling.md).  With bins of `window` columns, for a channel c, a phase row p and an amplitude
// row a, over the columns t of a bin of cnt columns:
//   u_p(t) = W[c,p,t] / |W[c,p,t]| (0 where that is 0),   M = sum |W[c,a,t]| u_p(t),   S = sum |W[c,a,t]|;
//   vector = M / cnt,   mvl = |M| / S clamped to [0, 1] (0 where S == 0),   amplitude = S / cnt.
//
// Work is cut by tiles of rows, not by cells: a workgroup takes one (channel, run of bins, tile of kCplPhase phase rows
// x kCplAmp amplitude rows), loads each of its at most 12 rows once, makes u of a phase element and |w| of an amplitude
// element once, and keeps the 32 cells (re, im) and the 8 sums S in 72 registers per lane.
//
// The normalisation is prescribed, every operation a single correctly rounded float32 one (sqrt and divide are IEEE:
// the build keeps the compiler's correctly rounded expansions, no fast-math):
//   r2 = fmaf(im, im, re * re);  |w| = sqrt(r2);  inv = 1 / |w_p| (0 where |w_p| == 0);  u = (re * inv, im * inv);
//   M.re = fmaf(|w_a|, u.x, M.re);  M.im = fmaf(|w_a|, u.y, M.im);  S = S + |w_a|.
// Roundings a term carries when it enters the chain, relative to |w_a|: |w_p| 2 (r2 has two, the root halves them and
// adds its own), inv 1, the product 1 -- u has 4 -- and |w_a| 2: k = 6.  The fmaf's own rounding belongs to the chain.
//
// The order of every sum is that of coherence.hip and does not depend on the tiling: a bin belongs to ONE wave; lane l
// accumulates the bin's columns l, l + 64, ... one after the other (one fmaf per component and column: ceil(window / 64)
// roundings), then a six-level butterfly adds the 64 lanes (lane ^ 1, ^ 2, the other quad, the other 8, ^ 16, ^ 32 --
// both partners add the same two numbers, so every lane ends with the same bits).  No atomics.  u depends on its phase
// row alone and |w| on its amplitude row alone, so a cell (p, a) asked for alone and the same cell inside any larger
// ranges run the same instructions on the same numbers: the same bits.
//
// The grid: the tiles of one (channel, run) read the same rows and are placed to meet them in one L2 (resident_op.h:
// the placement).  This is for speed only; nothing depends on it.
//
// Loads are 8 bytes per lane -- one complex column, 512 contiguous bytes of a row per wave and load -- for the reason
// coherence.hip gives: a 16-byte load would change a lane's chain.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "coupling.h"
#include "wave_reduce.h"

namespace gcwt {

namespace {

constexpr int kWaves = 4;                                   // per workgroup; each takes every fourth bin of the run
constexpr int kRedFloats = 2 * kCplCells + kCplAmp;         // a wave's reduced sums: (re, im) per cell, S per amplitude row

// FULL: all kCplPhase x kCplAmp rows exist (no row tests in the column loop)
template <bool FULL>
__device__ __forceinline__ void run_tile(const CplArgs& a, int ch, int tp, int ta, int64_t run, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_p = FULL ? kCplPhase : std::min(kCplPhase, a.n_phase - tp * kCplPhase);
  const int n_a = FULL ? kCplAmp : std::min(kCplAmp, a.n_amp - ta * kCplAmp);
  const float2* row_p = a.rows + ((int64_t)ch * a.n_scales + a.phase_first + tp * kCplPhase) * a.pitch;
  const float2* row_a = a.rows + ((int64_t)ch * a.n_scales + a.amp_first + ta * kCplAmp) * a.pitch;

  const int64_t m_end = std::min<int64_t>((run + 1) * a.run_bins, a.n_bins);
  for (int64_t m = run * a.run_bins + wave; m < m_end; m += kWaves) {
    const int64_t c_begin = m * a.window, c_end = std::min<int64_t>(c_begin + a.window, a.n_cols);
    float re[kCplCells], im[kCplCells], sa[kCplAmp];
#pragma unroll
    for (int k = 0; k < kCplCells; ++k) re[k] = im[k] = 0.f;
#pragma unroll
    for (int k = 0; k < kCplAmp; ++k) sa[k] = 0.f;

    for (int64_t c0 = c_begin; c0 < c_end; c0 += 64) {
      const bool ok = c0 + lane < c_end;                     // (lanes past the bin add exact zeros)
      const float2* col_p = row_p + c0;                      // uniform: a wave's load is base + lane
      const float2* col_a = row_a + c0;
      float2 vp[kCplPhase], va[kCplAmp];
#pragma unroll
      for (int i = 0; i < kCplPhase; ++i) {
        vp[i] = make_float2(0.f, 0.f);
        if (FULL || i < n_p)
          if (ok) vp[i] = (col_p + i * a.pitch)[lane];
      }
#pragma unroll
      for (int j = 0; j < kCplAmp; ++j) {
        va[j] = make_float2(0.f, 0.f);
        if (FULL || j < n_a)
          if (ok) va[j] = (col_a + j * a.pitch)[lane];
      }
      float2 u[kCplPhase];
      float w[kCplAmp];
#pragma unroll
      for (int i = 0; i < kCplPhase; ++i) {
        const float r = modulus(vp[i]);
        const float inv = r > 0.f ? 1.0f / r : 0.f;
        u[i] = make_float2(__fmul_rn(vp[i].x, inv), __fmul_rn(vp[i].y, inv));
      }
#pragma unroll
      for (int j = 0; j < kCplAmp; ++j) {
        w[j] = modulus(va[j]);
        if (FULL || j < n_a) sa[j] = __fadd_rn(sa[j], w[j]);
      }
#pragma unroll
      for (int i = 0; i < kCplPhase; ++i) {
        if (FULL || i < n_p) {
#pragma unroll
          for (int j = 0; j < kCplAmp; ++j) {
            const int k = i * kCplAmp + j;
            re[k] = fmaf(w[j], u[i].x, re[k]);
            im[k] = fmaf(w[j], u[i].y, im[k]);
          }
        }
      }
    }

    // the tree; lane 0 leaves the sums in the wave's own piece of LDS for the lanes that write the outputs
#pragma unroll
    for (int k = 0; k < kCplCells; ++k) {
      const float r = wave_sum(re[k]), q = wave_sum(im[k]);
      if (lane == 0) { red[2 * k] = r; red[2 * k + 1] = q; }
    }
#pragma unroll
    for (int k = 0; k < kCplAmp; ++k) {
      const float r = wave_sum(sa[k]);
      if (lane == 0) red[2 * kCplCells + k] = r;
    }
    wave_lds_sync();

    const float cnt = (float)(c_end - c_begin);
    if (lane < kCplCells) {                                  // lane = cell
      const int i = lane / kCplAmp, j = lane % kCplAmp;
      if (i < n_p && j < n_a) {
        const float r = red[2 * lane], q = red[2 * lane + 1], s = red[2 * kCplCells + j];
        const int64_t o = (((int64_t)ch * a.n_phase + tp * kCplPhase + i) * a.n_amp + ta * kCplAmp + j) * a.out_pitch + m;
        if (a.vector) a.vector[o] = make_float2(r / cnt, q / cnt);
        if (a.mvl) a.mvl[o] = s > 0.f ? fminf(modulus(make_float2(r, q)) / s, 1.f) : 0.f;
      }
    }
    if (a.amplitude && tp == 0 && lane < n_a)                // the first phase tile writes the amplitude rows
      a.amplitude[((int64_t)ch * a.n_amp + ta * kCplAmp + lane) * a.out_pitch + m] = red[2 * kCplCells + lane] / cnt;
    // (the next bin's sums go to the same piece of LDS: not before these reads)
    wave_lds_sync();
  }
}

__global__ void __launch_bounds__(64 * kWaves, 3) k_coupling(CplArgs a) {
  __shared__ float s_red[kWaves][kRedFloats];
  const TileOfUnit at = shared_place(a.n_ptiles * a.n_atiles);   // unit = (channel, run)
  if (at.unit >= a.n_units) return;                          // (the last group's padding)
  const int ch = (int)(at.unit / a.n_runs);
  const int64_t run = at.unit % a.n_runs;
  const int tp = at.tile / a.n_atiles, ta = at.tile % a.n_atiles;
  float* red = s_red[threadIdx.x >> 6];
  if ((tp + 1) * kCplPhase <= a.n_phase && (ta + 1) * kCplAmp <= a.n_amp)
    run_tile<true>(a, ch, tp, ta, run, red);
  else
    run_tile<false>(a, ch, tp, ta, run, red);
}

}  // namespace

hipError_t launch_coupling(const CplArgs& a, hipStream_t st) {
  const int64_t blocks = coupling_blocks(a);
  if (blocks <= 0 || blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_coupling, dim3((unsigned)blocks), dim3(64 * kWaves), 0, st, a);
  return hipGetLastError();
}

}  // namespace gcwt
