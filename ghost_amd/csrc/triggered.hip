// triggered.hip -- event-locked averages of the rows of a resident complex result (include/ghostcwt.h: gcwt_triggered;
// profiles/triggered.md).  With event columns e_0 .. e_{E-1} in the order given, nb columns before and na after an
// event, L = nb + na + 1 lags, and w_k = W[c, r, e_k - nb + l] for a channel c, a row r and a lag l:
//   r2_k = fmaf(im, im, re * re);  a_k = sqrt(r2_k);  inv_k = a_k > 0 ? 1 / a_k : 0;  u_k = (re * inv_k, im * inv_k);
//   A = sum a_k,  P = sum r2_k,  Ev = sum w_k,  V = sum u_k;
//   amplitude = A / E,  power = P / E,  evoked = Ev / E,  vector = V / E,
//   itpc = min(sqrt(fmaf(V.y, V.y, V.x * V.x)) / E, 1).
// Every operation is a single correctly rounded float32 one (sqrt and divide are IEEE: the build keeps the compiler's
// correctly rounded expansions, no fast-math; __fadd_rn / __fmul_rn where the compiler could contract).
//
// The order of every sum is prescribed and depends on the event list alone, not on the grid, the tiling, or which rows,
// lags or channels are asked for: four interleaved chains, chain j adding the terms of the events k = j, j + 4,
// j + 8, ... one after the other from an exact 0.f, combined as (X0 + X1) + (X2 + X3); a chain without events is an
// exact 0.f.  No atomics.  A cell (c, r, l) therefore has the same bits alone, inside any larger run of rows, and at
// the same absolute lag inside any other (nb, na).  PERMUTING THE EVENTS CHANGES THE CHAINS and with them the low bits:
// the order given is part of the definition.  E <= 2^24, so (float)E is exact.  Columns that are zero (the gaps between
// epochs) add exact zeros.
//
// The cut: a workgroup of four waves takes one channel, a tile of kTrgRows rows and a tile of 64 lags.  Lane = lag,
// wave j runs chain j: per event a wave issues kTrgRows independent 8-byte-per-lane loads -- 512 contiguous bytes of a
// row each, at whatever alignment the event column has -- and two events are in flight.  The event list is
// wave-uniform and is read from a device copy.  Six accumulators per row and lane: A, P, Ev.re, Ev.im, V.x, V.y.  The
// four waves meet through LDS; wave i then combines the chains of row i, divides and stores.  A tile whose rows and
// lags all exist takes an instantiation without tests in the event loop.
//
// The grid: the row tiles of one (channel, lag tile) read the same columns of neighbouring rows and the same events, and
// are placed to meet them in one L2 (resident_op.h: the placement).  This is for speed only; nothing depends on it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "triggered.h"
#include "wave_reduce.h"

namespace gcwt {

namespace {

constexpr int kSums = 6;                                    // A, P, Ev.re, Ev.im, V.x, V.y

struct Acc { float a, p, er, ei, vx, vy; };

// one term enters its chain: the prescribed sequence
__device__ __forceinline__ void add_term(Acc& s, float2 w) {
  const float r2 = norm2(w);
  const float r = __builtin_sqrtf(r2);
  const float inv = r > 0.f ? 1.0f / r : 0.f;
  s.a = __fadd_rn(s.a, r);
  s.p = __fadd_rn(s.p, r2);
  s.er = __fadd_rn(s.er, w.x);
  s.ei = __fadd_rn(s.ei, w.y);
  s.vx = __fadd_rn(s.vx, __fmul_rn(w.x, inv));
  s.vy = __fadd_rn(s.vy, __fmul_rn(w.y, inv));
}

// FULL: all kTrgRows rows and all 64 lags of the tile exist (no tests in the event loop)
template <bool FULL>
__device__ __forceinline__ void run_tile(const TrgArgs& a, int ch, int rt, int64_t lt, float (*red)[kTrgRows][kSums][kTrgLags]) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_r = FULL ? kTrgRows : std::min(kTrgRows, a.n_rows - rt * kTrgRows);
  const int64_t lag = lt * kTrgLags + lane;
  const bool ok = FULL || lag < a.n_lags;
  // column of lag `lag` around an event at column e: e - before + lag, inside [0, n_cols) for every event (checked
  // on the host) and every lag < n_lags
  const float2* base = a.rows + ((int64_t)ch * a.n_scales + a.row_first + rt * kTrgRows) * a.pitch + (lag - a.before);

  Acc s[kTrgRows];
#pragma unroll
  for (int i = 0; i < kTrgRows; ++i) s[i] = Acc{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  int64_t k = wave;
  for (; k + kTrgChains < a.n_events; k += 2 * kTrgChains) {   // two events of the chain in flight
    const int64_t e0 = a.events[k], e1 = a.events[k + kTrgChains];
    float2 v0[kTrgRows], v1[kTrgRows];
#pragma unroll
    for (int i = 0; i < kTrgRows; ++i) {
      v0[i] = v1[i] = make_float2(0.f, 0.f);
      if ((FULL || i < n_r) && ok) {
        v0[i] = (base + i * a.pitch)[e0];
        v1[i] = (base + i * a.pitch)[e1];
      }
    }
#pragma unroll
    for (int i = 0; i < kTrgRows; ++i) add_term(s[i], v0[i]);
#pragma unroll
    for (int i = 0; i < kTrgRows; ++i) add_term(s[i], v1[i]);
  }
  if (k < a.n_events) {
    const int64_t e0 = a.events[k];
    float2 v0[kTrgRows];
#pragma unroll
    for (int i = 0; i < kTrgRows; ++i) {
      v0[i] = make_float2(0.f, 0.f);
      if ((FULL || i < n_r) && ok) v0[i] = (base + i * a.pitch)[e0];
    }
#pragma unroll
    for (int i = 0; i < kTrgRows; ++i) add_term(s[i], v0[i]);
  }

  // the chains meet: wave j leaves chain j of every row
#pragma unroll
  for (int i = 0; i < kTrgRows; ++i) {
    red[wave][i][0][lane] = s[i].a;
    red[wave][i][1][lane] = s[i].p;
    red[wave][i][2][lane] = s[i].er;
    red[wave][i][3][lane] = s[i].ei;
    red[wave][i][4][lane] = s[i].vx;
    red[wave][i][5][lane] = s[i].vy;
  }
  __syncthreads();

  // wave i: row i of the tile
  if (wave >= n_r || !ok) return;
  float x[kSums];
#pragma unroll
  for (int q = 0; q < kSums; ++q)
    x[q] = __fadd_rn(__fadd_rn(red[0][wave][q][lane], red[1][wave][q][lane]),
                     __fadd_rn(red[2][wave][q][lane], red[3][wave][q][lane]));
  const float cnt = (float)a.n_events;
  const int64_t o = ((int64_t)ch * a.n_rows + rt * kTrgRows + wave) * a.out_pitch + lag;
  if (a.amplitude) a.amplitude[o] = x[0] / cnt;
  if (a.power) a.power[o] = x[1] / cnt;
  if (a.evoked) a.evoked[o] = make_float2(x[2] / cnt, x[3] / cnt);
  if (a.vector) a.vector[o] = make_float2(x[4] / cnt, x[5] / cnt);
  if (a.itpc) a.itpc[o] = fminf(modulus(make_float2(x[4], x[5])) / cnt, 1.f);
}

__global__ void __launch_bounds__(64 * kTrgChains) k_triggered(TrgArgs a) {
  __shared__ float s_red[kTrgChains][kTrgRows][kSums][kTrgLags];
  const TileOfUnit at = shared_place(a.n_rtiles);            // unit = (channel, lag tile)
  if (at.unit >= a.n_units) return;                          // (the last group's padding)
  const int rt = at.tile, ch = (int)(at.unit / a.n_ltiles);
  const int64_t lt = at.unit % a.n_ltiles;
  if ((rt + 1) * kTrgRows <= a.n_rows && (lt + 1) * kTrgLags <= a.n_lags)
    run_tile<true>(a, ch, rt, lt, s_red);
  else
    run_tile<false>(a, ch, rt, lt, s_red);
}

}  // namespace

hipError_t launch_triggered(const TrgArgs& a, hipStream_t st) {
  const int64_t blocks = triggered_blocks(a);
  if (blocks <= 0 || blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_triggered, dim3((unsigned)blocks), dim3(64 * kTrgChains), 0, st, a);
  return hipGetLastError();
}

}  // namespace gcwt
