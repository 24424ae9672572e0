// coupling_surrogates.hip -- shift surrogates of gcwt_coupling's mean vector length (include/ghostcwt.h:
// gcwt_coupling_surrogates; profiles/coupling_surrogates.md).  Bins, u_p, |w_a|, M, S and cnt are coupling.hip's.  For a
// shift L (columns, 0 <= L < window) the surrogate of a bin with first column b and cnt columns moves the amplitude row
// circularly inside the bin:
//   M_L = sum_{r=0}^{cnt-1} |W[c,a, b + (r + L') mod cnt]| u_p(b + r),   L' = L mod cnt,
//   mvl_L = min(|M_L| / S, 1), 0 where S == 0  (S does not change under the shift).
// Over the K shifts of the list, per cell and bin: T = sum mvl_k, Q = sum mvl_k^2 (float64),
//   mean = T / K,   sd = sqrt(max(0, (Q - T^2 / K) / (K - 1))),   both rounded to float32 once,
//   count_ge = the number of k with mvl_k >= mvl_0 as float32, mvl_0 the L = 0 value.
//
// A workgroup owns one (channel, bin, tile of kSurPhase phase rows x kSurAmp amplitude rows).  It makes u of each phase
// element and |w| of each amplitude element once (wave_reduce.h: modulus; inv and u as coupling.hip has them) and parks
// them in LDS as planes: float2 u[phase row][column], float |w|[amplitude row][column].  Rows a ragged tile lacks are
// planes of zeros: their cells are computed and not written.  Its kSurWaves waves then share the shifts.
//
// The prescribed order.  A term and every float32 sum are coupling.hip's, unchanged:
//   M.re = fmaf(|w_a|, u.x, M.re);  M.im = fmaf(|w_a|, u.y, M.im)   (here the two halves of one packed fma);
//   lane l takes the bin-relative columns r = l, l + 64, ... one after the other (lanes past the bin add exact zeros),
//   then wave_sum's butterfly;  mvl = S > 0 ? fminf(modulus(M) / S, 1) : 0, and S is the chain S = S + |w_a| in the same
//   lane order, then the butterfly.  So mvl_L at L = 0 has the bits of gcwt_coupling's mvl.
// The float64 sums: wave v takes the shifts k = v, v + kSurWaves, v + 2 kSurWaves, ... in ascending order and adds, from
// an exact 0, T_v = T_v + (double)mvl_k and Q_v = Q_v + (double)mvl_k * (double)mvl_k (the product of two float32 is
// exact in float64).  Then T = (((T_0 + T_1) + T_2) + ...) + T_{kSurWaves - 1}, Q likewise, and the counts are added.
// The order depends on K alone, never on timing.  No atomics.
//
// mvl_0 is made once per workgroup, before the shifts: wave v computes the kSurCells / kSurWaves cells v owns (the same
// chains on the same numbers as in the full tile: the same bits) and S of their amplitude rows.
//
// LDS reads in a shift's pass: u at column r is 8 bytes per lane, consecutive lanes on consecutive addresses; |w| at
// (r + L') mod cnt is 4 bytes per lane in at most two contiguous runs -- no bank conflict within a run at any L.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "coupling_surrogates.h"
#include "wave_reduce.h"

namespace gcwt {

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int kOwn = kSurCells / kSurWaves;                  // cells of a wave when mvl_0 is made: a run inside one phase row
static_assert(kSurCells % kSurWaves == 0 && kSurAmp % kOwn == 0, "a wave's cells for mvl_0 lie in one phase row");

// |M| / S as coupling.hip forms mvl
__device__ __forceinline__ float mvl_of(float re, float im, float s) {
  return s > 0.f ? fminf(modulus(make_float2(re, im)) / s, 1.f) : 0.f;
}

// m[i * NA + j] = M_shift of (phase plane i, amplitude plane j), this lane's chain only: columns lane, lane + 64, ...
template <int NP, int NA>
__device__ __forceinline__ void lane_chains(const float2* su, const float* sw, int wp, int cnt, int shift, int lane,
                                            v2f (&m)[NP * NA]) {
#pragma unroll
  for (int k = 0; k < NP * NA; ++k) m[k] = (v2f)(0.f);
  int c0 = 0;
  for (; c0 + 64 <= cnt; c0 += 64) {
    const int r = c0 + lane;
    int q = r + shift;
    if (q >= cnt) q -= cnt;
    v2f u[NP];
    float w[NA];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const float2 t = su[i * wp + r];
      u[i].x = t.x; u[i].y = t.y;
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) w[j] = sw[j * wp + q];
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
      for (int j = 0; j < NA; ++j) m[i * NA + j] = __builtin_elementwise_fma((v2f)(w[j]), u[i], m[i * NA + j]);
  }
  if (c0 < cnt) {                                            // the last 64: lanes past the bin add exact zeros
    const bool ok = c0 + lane < cnt;
    const int r = ok ? c0 + lane : 0;                        // (an address inside the plane either way)
    int q = r + shift;
    if (q >= cnt) q -= cnt;
    v2f u[NP];
    float w[NA];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const float2 t = su[i * wp + r];
      u[i].x = ok ? t.x : 0.f; u[i].y = ok ? t.y : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const float t = sw[j * wp + q];
      w[j] = ok ? t : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
      for (int j = 0; j < NA; ++j) m[i * NA + j] = __builtin_elementwise_fma((v2f)(w[j]), u[i], m[i * NA + j]);
  }
}

__global__ void __launch_bounds__(64 * kSurWaves) k_coupling_surrogates(SurArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const TileOfUnit at = shared_place(a.n_ptiles * a.n_atiles);   // unit = (channel, bin)
  if (at.unit >= a.n_units) return;                          // (the last group's padding; the whole workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ch = (int)(at.unit / a.n_bins);
  const int64_t bin = at.unit % a.n_bins;
  const int tp = at.tile / a.n_atiles, ta = at.tile % a.n_atiles;
  const int n_p = std::min(kSurPhase, a.n_phase - tp * kSurPhase);
  const int n_a = std::min(kSurAmp, a.n_amp - ta * kSurAmp);
  const int64_t c_begin = bin * a.window;
  const int cnt = (int)std::min<int64_t>(a.window, a.n_cols - c_begin);
  const int wp = (int)surrogates_plane_cols(a.window);

  float2* su = reinterpret_cast<float2*>(smem);              // [kSurPhase][wp]
  float* sw = reinterpret_cast<float*>(smem + (size_t)wp * 8 * kSurPhase);   // [kSurAmp][wp]
  char* tail = smem + (size_t)wp * kSurColBytes;
  double* s_t = reinterpret_cast<double*>(tail);             // [kSurWaves][kSurCells]
  double* s_q = s_t + kSurWaves * kSurCells;                 // [kSurWaves][kSurCells]
  float* s_red = reinterpret_cast<float*>(s_q + kSurWaves * kSurCells);      // [kSurWaves][2 kSurCells]
  int* s_n = reinterpret_cast<int*>(s_red + kSurWaves * 2 * kSurCells);      // [kSurWaves][kSurCells]
  float* s_s = reinterpret_cast<float*>(s_n + kSurWaves * kSurCells);        // [kSurAmp]
  float* s_mvl0 = s_s + kSurAmp;                             // [kSurCells]

  // u and |w| of the bin, once
  {
    const float2* row_p = a.rows + ((int64_t)ch * a.n_scales + a.phase_first + tp * kSurPhase) * a.pitch + c_begin;
    const float2* row_a = a.rows + ((int64_t)ch * a.n_scales + a.amp_first + ta * kSurAmp) * a.pitch + c_begin;
    for (int r = threadIdx.x; r < cnt; r += 64 * kSurWaves) {
      float2 vp[kSurPhase], va[kSurAmp];
#pragma unroll
      for (int i = 0; i < kSurPhase; ++i) vp[i] = i < n_p ? (row_p + i * a.pitch)[r] : make_float2(0.f, 0.f);
#pragma unroll
      for (int j = 0; j < kSurAmp; ++j) va[j] = j < n_a ? (row_a + j * a.pitch)[r] : make_float2(0.f, 0.f);
#pragma unroll
      for (int i = 0; i < kSurPhase; ++i) {
        const float mod = modulus(vp[i]);
        const float inv = mod > 0.f ? 1.0f / mod : 0.f;
        su[i * wp + r] = make_float2(__fmul_rn(vp[i].x, inv), __fmul_rn(vp[i].y, inv));
      }
#pragma unroll
      for (int j = 0; j < kSurAmp; ++j) sw[j * wp + r] = modulus(va[j]);
    }
  }
  __syncthreads();

  // S of the amplitude rows and mvl_0 of the cells, each wave its own
  {
    const int i = wave * kOwn / kSurAmp, j0 = wave * kOwn % kSurAmp;
    v2f m[kOwn];
    lane_chains<1, kOwn>(su + i * wp, sw + j0 * wp, wp, cnt, 0, lane, m);
    float sa[kOwn];
#pragma unroll
    for (int j = 0; j < kOwn; ++j) sa[j] = 0.f;
    for (int c0 = 0; c0 < cnt; c0 += 64) {
      const bool ok = c0 + lane < cnt;
      const int r = ok ? c0 + lane : 0;
#pragma unroll
      for (int j = 0; j < kOwn; ++j) {
        const float t = sw[(j0 + j) * wp + r];
        sa[j] = __fadd_rn(sa[j], ok ? t : 0.f);
      }
    }
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const float re = wave_sum(m[j].x), im = wave_sum(m[j].y), s = wave_sum(sa[j]);
      if (lane == 0) {
        s_mvl0[wave * kOwn + j] = mvl_of(re, im, s);
        if (i == 0) s_s[j0 + j] = s;
      }
    }
  }
  __syncthreads();

  // the shifts of this wave; lane < kSurCells judges cell `lane`
  const int ci = lane / kSurAmp, cj = lane % kSurAmp;
  const bool cell = lane < kSurCells && ci < n_p && cj < n_a;
  const float s_cell = s_s[cj], mvl0 = s_mvl0[lane & (kSurCells - 1)];
  const int64_t o_cell = (((int64_t)ch * a.n_phase + tp * kSurPhase + ci) * a.n_amp + ta * kSurAmp + cj) * a.out_pitch + bin;
  const int64_t plane = (int64_t)a.n_channels * a.n_phase * a.n_amp * a.out_pitch;
  float* red = s_red + wave * 2 * kSurCells;
  double t_sum = 0.0, q_sum = 0.0;
  int n_ge = 0;
  for (int k = wave; k < a.n_shifts; k += kSurWaves) {
    const int shift = a.shifts[k] % cnt;                     // uniform
    v2f m[kSurCells];
    lane_chains<kSurPhase, kSurAmp>(su, sw, wp, cnt, shift, lane, m);
#pragma unroll
    for (int c = 0; c < kSurCells; ++c) {
      const float re = wave_sum(m[c].x), im = wave_sum(m[c].y);
      if (lane == 0) { red[2 * c] = re; red[2 * c + 1] = im; }
    }
    wave_lds_sync();
    if (cell) {
      const float v = mvl_of(red[2 * lane], red[2 * lane + 1], s_cell);
      t_sum += (double)v;
      q_sum += (double)v * (double)v;
      n_ge += v >= mvl0 ? 1 : 0;
      if (a.surrogates) a.surrogates[k * plane + o_cell] = v;
    }
    wave_lds_sync();                                         // (the next shift's sums go to the same piece of LDS)
  }
  if (lane < kSurCells) {
    s_t[wave * kSurCells + lane] = t_sum;
    s_q[wave * kSurCells + lane] = q_sum;
    s_n[wave * kSurCells + lane] = n_ge;
  }
  __syncthreads();

  if (wave == 0 && cell) {                                   // the waves' partial sums, in wave order
    double t = s_t[lane], q = s_q[lane];
    int n = s_n[lane];
#pragma unroll
    for (int v = 1; v < kSurWaves; ++v) {
      t += s_t[v * kSurCells + lane];
      q += s_q[v * kSurCells + lane];
      n += s_n[v * kSurCells + lane];
    }
    const double kk = (double)a.n_shifts;
    if (a.mean) a.mean[o_cell] = (float)(t / kk);
    if (a.sd) a.sd[o_cell] = (float)sqrt(fmax(0.0, (q - t * t / kk) / (kk - 1.0)));
    if (a.count_ge) a.count_ge[o_cell] = n;
  }
}

}  // namespace

hipError_t launch_coupling_surrogates(const SurArgs& a, hipStream_t st) {
  const int64_t blocks = surrogates_blocks(a);
  if (blocks <= 0 || blocks > 0x7fffffff || a.window > kSurMaxWindow) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_coupling_surrogates),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)surrogates_lds_bytes(kSurMaxWindow));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_coupling_surrogates, dim3((unsigned)blocks), dim3(64 * kSurWaves),
                     (size_t)surrogates_lds_bytes(a.window), st, a);
  return hipGetLastError();
}

}  // namespace gcwt
