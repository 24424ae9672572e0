// phase_advance.h -- device only: the instantaneous frequency of a row at a column from the phase advance between its two
// neighbours, the one sequence of float32 operations that ridge.hip (on the winning row) and squeeze.hip (on every row)
// prescribe in the same words.  x = W[row, tp], y = W[row, tm], span = tp - tm (0, 1 or 2), nu_row the advance the row
// expects per column:
//   re = fmaf(x.x, y.x, x.y * y.y);   im = fmaf(x.y, y.x, -(x.x * y.y));   dphi = atan2f(im, re)
//   k = rintf(((float)span * nu_row - dphi) / kTwoPi)                        3 roundings, then the integer
//   num = dphi + kTwoPi * k                                                  2 roundings
//   scale = hz_per_cycle / (kTwoPi * (float)span)                            the product is exact (span is 1 or 2); 1
//   frequency = num * scale                                                  1
// with kTwoPi = float32(2 pi); NaN where span == 0 or re and im are both 0.  tests/ridge_model.py counts the bound.
#pragma once
#include <hip/hip_runtime.h>

namespace gcwt {

constexpr float kTwoPi = 6.28318530717958647692f;

// A product and the sum it feeds stay two roundings unless the code says fmaf.
__device__ __forceinline__ float phase_advance_hz(float2 x, float2 y, int span, float nu_row, float hz_per_cycle) {
#pragma clang fp contract(off)
  const float nan = __builtin_nanf("");
  if (span == 0) return nan;
  const float re = fmaf(x.x, y.x, __fmul_rn(x.y, y.y));
  const float im = fmaf(x.y, y.x, -__fmul_rn(x.x, y.y));
  if (re == 0.f && im == 0.f) return nan;
  const float dphi = atan2f(im, re);
  const float span_f = (float)span;
  const float k = rintf(__fdiv_rn(__fsub_rn(__fmul_rn(span_f, nu_row), dphi), kTwoPi));
  const float num = __fadd_rn(dphi, __fmul_rn(kTwoPi, k));
  const float scale = __fdiv_rn(hz_per_cycle, __fmul_rn(kTwoPi, span_f));
  return __fmul_rn(num, scale);
}

}  // namespace gcwt
