// wave_reduce.h -- device only: the pieces of float32 arithmetic and wave-level synchronisation that the row operators
// (coherence.hip, coupling.hip, triggered.hip, bandpass.hip) prescribe in the same words.  Every function is one fixed sequence of
// correctly rounded operations; the kernels' own comments count the roundings.
#pragma once
#include <hip/hip_runtime.h>

namespace gcwt {

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// The fixed tree: a six-level butterfly adds the 64 lanes (lane ^ 1, ^ 2, the other quad, the other 8, ^ 16, ^ 32).  Both
// partners of a level add the same two numbers, so every lane returns the same bits: the sum over the wave.
__device__ __forceinline__ float wave_sum(float v) {
  v = __fadd_rn(v, dpp<0xB1>(v));        // quad_perm [1, 0, 3, 2]: lane ^ 1
  v = __fadd_rn(v, dpp<0x4E>(v));        // quad_perm [2, 3, 0, 1]: lane ^ 2
  v = __fadd_rn(v, dpp<0x141>(v));       // row_half_mirror: the other quad of the 8 (quads are uniform by now)
  v = __fadd_rn(v, dpp<0x140>(v));       // row_mirror: the other 8 of the 16
  v = __fadd_rn(v, __shfl_xor(v, 16));
  v = __fadd_rn(v, __shfl_xor(v, 32));
  return v;
}

// |w|^2 as prescribed: r2 = fmaf(im, im, re * re), two roundings
__device__ __forceinline__ float norm2(float2 v) { return fmaf(v.y, v.y, __fmul_rn(v.x, v.x)); }
// |w| as prescribed: sqrt(r2), one more rounding (who needs r2 as well takes the root of norm2() itself)
__device__ __forceinline__ float modulus(float2 v) { return __builtin_sqrtf(norm2(v)); }

// Between a wave's writes to its own piece of LDS and its reads of it (either way round): no other wave touches the
// piece, so a wave-level barrier between a release and an acquire fence is enough.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace gcwt
