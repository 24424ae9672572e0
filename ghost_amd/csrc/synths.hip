// synths.hip -- the spectral synthesis with an output stride K > 1 (gcwt_plan_set_output_stride): only the samples n
// of the recording that K divides are made and stored, at column n / K.  The prologue, scale walk and first transform
// of k_synth7s / k_synthis are those of k_synth7 (synth.hip) / k_synthi (synthi.hip), copied; the two kernels they come
// from, and the K = 1 launches, are left as they are.
//   k_synth7s  a column (block, phase r) is transformed only if its phase can hold a kept sample: with g = gcd(R, K)
//              >= 4 the columns are dealt phase-major and the waves of the other phases skip both halves of the
//              256-point transform (R | K: one phase of R).  Rows are stored when kept; a store's column is one
//              multiply-high by ceil(2^32 / K).
//   k_synthis  pass A (the q phases per block and scale) as k_synthi; pass B deals the kept samples one per lane: the
//              FIR and |.| run once per kept sample, and the lanes of a store write consecutive columns.
// (transforms.py:203-204 per scale, then [..., ::K] of the result.)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "interp.h"
#include "kernels.h"
#include "synth_math.h"

#ifndef GCWT_STORE_AUX
#define GCWT_STORE_AUX 2   // nt: the rows are written once and not read by this launch
#endif

namespace gcwt {

namespace {
// exp(-2 pi i shift r / (256 R)): what phase r of a level whose band starts `shift` bins below zero
// carries (shift r < 2^24: exact in float before the division by a power of two)
__device__ __forceinline__ v2f phase_carrier(int shift, int r, int R) {
  float sn, cs;
  sincospif(-2.0f * (float)(shift * r) / (256.0f * (float)R), &sn, &cs);
  return (v2f){cs, sn};
}

// One column's sixteen first-stage outputs times W256^(t j) (tw: this lane's sixteen, two per 16-byte
// read; j = 0 is 1) into the exchange planes, STRIDE elements apart (0: run-time stride).
template <int STRIDE>
__device__ __forceinline__ void twiddle_to_planes(v2f* exw, const v2f (&v)[16], const v2f* tw, int stride = STRIDE) {
  const int st = STRIDE ? STRIDE : stride;
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    const v4f w2 = *reinterpret_cast<const v4f*>(tw + 2 * jj);
    exw[(2 * jj) * st] = jj == 0 ? v[0] : cmulv(v[dft16_pos(2 * jj)], (v2f){w2.x, w2.y});
    exw[(2 * jj + 1) * st] = cmulv(v[dft16_pos(2 * jj + 1)], (v2f){w2.z, w2.w});
  }
}

constexpr int kT = kInterpTaps;
static_assert(kT == 8, "the FIR loop below is written for 8 taps");
// Columns per pass.  16 (256 threads, three workgroups and 12 waves per CU, up to 168 VGPRs: the
// persistent operand, the FIR coefficients and both transforms' working sets fit without spills);
// 32 (512 threads, two workgroups and 16 waves per CU, 128 VGPRs) spilled 32 dwords and was slower.
constexpr int kColsI = kInterpCols;
constexpr int kLgColsI = kColsI == 32 ? 5 : kColsI == 16 ? 4 : 3;
constexpr int kThreadsI = 16 * kColsI;
constexpr int kWavesI = kThreadsI / 64;
constexpr int kPlaneI = kThreadsI + 1;
constexpr int kZPad = 4;                         // v2f entries between the slots of the z buffer: their
                                                 // writes fall on different banks
constexpr int kSlotsMax = kColsI / 2;            // z slots and scale slots of a pass: q >= 2
static_assert(kColsI == kInterpCols, "the host cuts the passes for this many columns (interp.h)");
constexpr int kZElems = 256 * kColsI + kSlotsMax * kZPad;     // z buffer
constexpr int kExElems = kZElems > 16 * kPlaneI ? kZElems : 16 * kPlaneI;   // ... in place of the 16 exchange planes
constexpr int kGainRowI = 16 * 20;
constexpr int kLdsBytes = kExElems * 8 + 256 * 8 + kSlotsMax * kGainRowI * 4 + 2 * 256 * 4;

}  // namespace


// CG: complex gain rows, as in k_synth7 (synth.hip) -- Morlet plans
template <int MODE, int NCOL, bool CG = false>
__global__ void __launch_bounds__(16 * NCOL, NCOL == 32 ? 4 : 3) k_synth7s(const Synth7Args a) {
  constexpr int kThreads = 16 * NCOL;
  constexpr int kPlane = kThreads + 1;
  constexpr int kLgN = NCOL == 32 ? 5 : 4;
  // gains of one scale in LDS: lane t's sixteen (bins t + 16 j) side by side, 20 floats per lane so
  // that the four 16-byte reads of the 16 lanes of a column fall on distinct banks
  // CG (complex rows): lane t's sixteen float2, 36 floats per lane -- eight 16-byte reads, the 16 lanes of a column on
  // distinct banks again -- and four scales to a chunk, so that the staging area stays the 10 KB it is
  constexpr int kGainRow = CG ? 16 * 36 : 16 * 20;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v2f* const ex = reinterpret_cast<v2f*>(smem);
  // W256 twiddles of the inter-stage multiply, lane t's sixteen side by side (pitch 18: 144 bytes, so
  // that they come in as 16-byte reads and the 16 lanes of a column fall on distinct banks)
  constexpr int kTwPitch = 18;
  v2f* const twl = ex + 16 * kPlane;
  float* const stage = reinterpret_cast<float*>(twl + 16 * kTwPitch);   // gains of kChunk scales
  int* const sc_lds = reinterpret_cast<int*>(stage + 8 * 320);   // this level's scale indices
  v2f* const half_lds = reinterpret_cast<v2f*>(sc_lds + 256);         // the level's half-sample factors

  const Synth7Item it = a.items[blockIdx.x];
  const Synth7Level lv = a.levels[it.level];
  const int c = blockIdx.y;               // workspace slot: segment * n_channels + channel
  const int seg = c / a.seg.n_channels, ch = c - seg * a.seg.n_channels;
  const int R = lv.decimation, lg = lv.log2r, hop = lv.hop, halo = lv.halo, sh = lv.band_shift;
  {
    // The level grids are the union over the batch's segments: leave at once if this
    // group of blocks keeps no sample inside this segment's window (workgroup-uniform).
    const int64_t span = (int64_t)hop * R;
    const int64_t first = (int64_t)(lv.blk_base + it.blk0) * span;
    const int64_t last = first + (int64_t)(R > NCOL ? 1 : NCOL / R) * span;
    if (last <= a.seg.w_lo[seg] || first >= a.seg.w_hi[seg]) return;
  }
  const int tid = threadIdx.x;
  const int colw = tid >> 4, t = tid & 15;
  const bool wide = R > NCOL;
  // Phase selection.  The sample a column (block, phase r) makes at block position m is n = G + R (m_b + m) + r (G: the
  // segment's first sample in the recording), and K divides n only if g = gcd(R, K) divides G + r: a column whose
  // phase fails that makes nothing that is kept (R | K: one phase of R is left).  With g > 1 the columns are dealt
  // phase-major -- column c is phase c / nb of block c mod nb, nb = NCOL / R blocks per workgroup -- so that a wave's
  // columns share a phase (or hold consecutive ones, R >= 16), and the waves of the phases nothing needs skip both
  // halves of the transform.  With g < 4 the layout is k_synth7's: every phase is needed (odd K), or half of them
  // (g = 2), where the phase-major layout measured slower than computing them all (its stores come in 64-byte pieces).
  const int64_t seg0 = a.seg.seg_col[seg] + a.seg.os.r0;          // recording sample of segment sample 0
  const int g = min(R, a.seg.os.k & -a.seg.os.k);                 // gcd(R, K): R is a power of two
  const bool by_phase = g >= 4;                                   // workgroup-uniform
  const int lgnb = wide ? 0 : kLgN - lg;                          // log2 of the blocks per workgroup
  const int blk_l = wide ? 0 : by_phase ? (colw & ((1 << lgnb) - 1)) : (colw >> lg);
  const int r = wide ? it.rtile * NCOL + colw : by_phase ? (colw >> lgnb) : (colw & (R - 1));
  const bool need1 = (((int)(seg0 & (g - 1)) + r) & (g - 1)) == 0;   // this thread's column makes a kept sample
  const int* const scales = a.scale_list + lv.scale_offset;
  constexpr int kChunk = CG ? 4 : 8;
  // ---- every global load of the prologue is issued here, before anything waits for one: the
  // workgroup pays one trip to memory, not one per table ----
  // this level's scale entries (read from LDS inside the loop: a global load there would have to
  // wait for vmcnt(0), i.e. for every store still in flight); at most 256 per level
  const int sc_v = tid < lv.n_scales ? scales[tid] : 0;
  // W256^((t - shift) j), parked as [t][j]
  const float2 tw_v = tid < 256 ? a.tw256[(((tid & 15) - sh) * (tid >> 4)) & 255] : make_float2(0.f, 0.f);
  // The filter enters as its real gain |H_s[k]|; the half-sample phase that even kernel
  // lengths carry is folded into P when the walk reaches those scales (they come last in
  // the level's list; its 256 factors wait in LDS).  Gains of kChunk scales at a time are
  // parked in LDS (10 KB), lane t's sixteen side by side; gain_lv holds them in that order
  // (k_scale_windows), one 16-byte load per thread and chunk, the next chunk's issued as soon as
  // the current one is parked.
  constexpr int kRowVec = CG ? 128 : 64;                 // float4 per scale's row
  constexpr int kGainLoads = kChunk * kRowVec / kThreads;   // float4 per thread and chunk: 1 (2 for 16 columns)
  static_assert(kGainLoads * kThreads == kChunk * kRowVec, "one chunk = a whole number of loads per thread");
  const float4* const gain_rows = reinterpret_cast<const float4*>(a.gain_lv + (int64_t)lv.scale_offset * (4 * kRowVec));
  static_assert(kGainLoads == 1 || kGainLoads == 2, "one or two 16-byte loads per thread and chunk");
  // (two named registers, not an array: captured by the lambdas below an array of two went to scratch memory -- 48 bytes
  // of private segment per lane and a scratch set-up for every wave of the 16-column instantiation)
  float4 g_v0 = make_float4(0.f, 0.f, 0.f, 0.f), g_v1 = g_v0;
  auto load_gains = [&](int b0) {
    g_v0 = gain_rows[b0 * kRowVec + tid];
    if constexpr (kGainLoads > 1) g_v1 = gain_rows[b0 * kRowVec + kThreads + tid];
  };
  auto park_one = [&](int f, const float4& g) {          // float4 f of the chunk: scale f >> 6, lane (f >> 2) & 15
    if constexpr (CG)                                    // ... scale f >> 7, lane (f >> 3) & 15
      *reinterpret_cast<float4*>(stage + (f >> 7) * kGainRow + ((f >> 3) & 15) * 36 + (f & 7) * 4) = g;
    else
      *reinterpret_cast<float4*>(stage + (f >> 6) * kGainRow + ((f >> 2) & 15) * 20 + (f & 3) * 4) = g;
  };
  auto park_gains = [&]() {
    park_one(tid, g_v0);
    if constexpr (kGainLoads > 1) park_one(kThreads + tid, g_v1);
  };
  load_gains(0);
  const bool has_half = lv.n_plain < lv.n_scales;        // workgroup-uniform
  const float2 half_v = has_half && tid < 256 ? a.level_half_tw[lv.half_offset + tid] : make_float2(1.f, 0.f);
  const float2* ltw = a.level_tw + lv.tw_offset;
  const float2 b0 = ltw[t * r], st = ltw[16 * r];
  v2f pw[16];
  if (a.xr) {
    // Block spectra made here: XB_b = FFT_256(x_R[(b hop - halo + n) mod M]) / (256 P) for the
    // workgroup's 32/R blocks (one for R > 32), 16 threads per block, forward transform as
    // conj(IFFT(conj .)) on the packed inverse DFT16; the result goes through LDS to every
    // column (phase) of its block.  Saves the XB array's round trip through HBM and a launch
    // per level.  `ex` is free until the scale loop starts: [NCOL/2][16][16] exchange (element
    // (t, m2) at t*16 + (m2 ^ t): conflict-free without padding) + [NCOL/2][256] spectra
    // (at most NCOL/2 blocks per workgroup: R = 2).
    const int nblk_wg = wide ? 1 : (NCOL >> lg);
    v2f* const fx = ex;
    v2f* const xbs = ex + (NCOL / 2) * 256;
    static_assert(NCOL * 256 <= 16 * (16 * NCOL + 1), "prologue buffers must fit the exchange planes");
    v2f v[16];
    const int blkx = min(it.blk0 + colw, lv.nblk - 1);
    const int64_t m_b = (int64_t)(lv.blk_base + blkx) * hop - halo;       // the block's first decimated sample
    // the block's carrier: exp(-2 pi i shift m_b / 256)
    float2 cb = make_float2(1.f, 0.f);
    if (colw < nblk_wg) {
      if (sh) cb = a.tw256[(-(int64_t)sh * m_b) & 255];
      const float2* xr = a.xr + (int64_t)c * a.xr_cstride + lv.xr_offset;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float2 q = xr[(m_b + t + 16 * j) & lv.m_mask];
        v[j] = (v2f){q.x, -q.y};
      }
    }
    // the small tables first (they were asked for first), the samples stay in flight meanwhile
    if (tid < lv.n_scales) sc_lds[tid] = sc_v;
    if (tid < 256) { twl[(tid & 15) * kTwPitch + (tid >> 4)] = (v2f){tw_v.x, tw_v.y}; half_lds[tid] = (v2f){half_v.x, half_v.y}; }
    park_gains();
    if (lv.n_scales > kChunk) load_gains(kChunk);
    if (colw < nblk_wg) {
      idft16v(v);
#pragma unroll
      for (int m = 0; m < 16; ++m) fx[colw * 256 + t * 16 + (m ^ t)] = v[dft16_pos(m)];
    }
    __syncthreads();
    if (colw < nblk_wg) {
      // element (writer k1, index t) arrives without its twiddle exp(+2 pi i k1 t / 256): with no
      // band shift that is twl[t][k1], just parked
#pragma unroll
      for (int k1 = 0; k1 < 16; ++k1) v[k1] = fx[colw * 256 + k1 * 16 + (t ^ k1)];
      if (sh) {                              // workgroup-uniform
#pragma unroll
        for (int k1 = 1; k1 < 16; ++k1) {
          const float2 w = a.tw256[(t * k1) & 255];
          v[k1] = cmulv(v[k1], (v2f){w.x, w.y});
        }
      } else {
#pragma unroll
        for (int k1 = 1; k1 < 16; ++k1) v[k1] = cmulv(v[k1], twl[t * kTwPitch + k1]);
      }
      idft16v(v);
      const float xs = a.xb_scale;
      if (sh) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const v2f z = v[dft16_pos(j)];
          xbs[colw * 256 + t + 16 * j] = cmulv((v2f){z.x * xs, -z.y * xs}, (v2f){cb.x, cb.y});
        }
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const v2f z = v[dft16_pos(j)];
          xbs[colw * 256 + t + 16 * j] = (v2f){z.x * xs, -z.y * xs};
        }
      }
    }
    __syncthreads();
    v2f wcur = (v2f){b0.x, b0.y};
    if (sh) wcur = cmulv(wcur, phase_carrier(sh, r, R));
    const v2f wstep = (v2f){st.x, st.y};
    const v2f* const mine = xbs + blk_l * 256 + t;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      pw[j] = cmulv(mine[16 * j], wcur);
      wcur = cmulv(wcur, wstep);
    }
  } else {
    // it.blk0 counts from the level's first computed block (lv.blk_base); columns past
    // the last block reuse it and are never stored
    const int blk = min(it.blk0 + blk_l, lv.nblk - 1);
    const float2* xb = a.xb + (int64_t)c * a.xb_cstride + lv.xb_offset + (int64_t)blk * 256 + t;
    v2f wcur = (v2f){b0.x, b0.y};
    if (sh) {   // the phase's and the block's carriers (the XB pass knows nothing of the shift)
      const float2 cb = a.tw256[(-(int64_t)sh * ((int64_t)(lv.blk_base + blk) * hop - halo)) & 255];
      wcur = cmulv(cmulv(wcur, phase_carrier(sh, r, R)), (v2f){cb.x, cb.y});
    }
    const v2f wstep = (v2f){st.x, st.y};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float2 q = xb[16 * j];
      pw[j] = cmulv((v2f){q.x, q.y}, wcur);
      wcur = cmulv(wcur, wstep);
    }
    if (tid < lv.n_scales) sc_lds[tid] = sc_v;
    if (tid < 256) { twl[(tid & 15) * kTwPitch + (tid >> 4)] = (v2f){tw_v.x, tw_v.y}; half_lds[tid] = (v2f){half_v.x, half_v.y}; }
    park_gains();
    if (lv.n_scales > kChunk) load_gains(kChunk);
  }
  const int sstride = wide ? NCOL : R;
  v2f* const exw = ex + ((t - sh) & 15) * kPlane + (wide ? colw : (blk_l << (4 + lg)) + r);
  // second half: thread -> (block, phase, m2).  k_synth7's order (consecutive threads, consecutive samples) for odd K;
  // with phase selection 16 threads per column, columns in the same phase-major order as the first half
  const int c2 = tid >> 4;
  const int blk_l2 = wide ? 0 : by_phase ? (c2 & ((1 << lgnb) - 1)) : (tid >> (4 + lg));
  const int m2 = by_phase ? (tid & 15) : wide ? (tid >> kLgN) : ((tid & ((16 << lg) - 1)) >> lg);
  const int r2 = wide ? it.rtile * NCOL + (by_phase ? c2 : (tid & (NCOL - 1))) : by_phase ? (c2 >> lgnb) : (tid & (R - 1));
  const int idx2 = wide ? (m2 << kLgN) + (r2 - it.rtile * NCOL) : (blk_l2 << (4 + lg)) + (m2 << lg) + r2;
  const v2f* const exr = ex + idx2;
  const int off0 = (blk_l2 * hop + m2 - halo) * R + r2;   // sample offset of row m1 = 0
  const int m1step = 16 * R;

  // ---- what differs from k_synth7: the stores ----
  // Row m1 of a thread (block position 16 m1 + m2, window-relative sample sw = s0 + m1 m1step) is stored when it lies
  // in the block's kept part [halo, 256 - halo), inside the window [w_lo, w_hi) and on the output grid (K divides its
  // recording sample n = nw0 + sw); it goes to column n / K.  Which rows those are depends on the thread alone: a
  // 14-bit mask made once.  A thread's samples are its lane's position in the block plus multiples of 16 R, so the
  // kept lanes of one store hold consecutive recording samples and write consecutive columns.  The descriptor spans
  // exactly the window's columns.
  constexpr int kElem = MODE == GCWT_OUT_COMPLEX_C64 ? 2 : 1;   // floats per output sample
  const OutStride os = a.seg.os;
  const int64_t n_b = (int64_t)(lv.blk_base + it.blk0) * hop * R;   // first sample of the block group
  const int64_t w_lo = a.seg.w_lo[seg];
  const int64_t w_len = a.seg.w_hi[seg] - w_lo;
  const int64_t nw0 = a.seg.seg_col[seg] + os.r0 + w_lo;            // recording sample of the window's first
  const int64_t q_lo = (nw0 + os.k - 1) / os.k, q_hi = (nw0 + w_len + os.k - 1) / os.k;
  const unsigned ext_bytes = q_hi > q_lo ? (unsigned)((q_hi - q_lo) * (4 * kElem)) : 0u;
  float* const out0 = a.out + ((int64_t)ch * a.n_scales * a.row_len + (q_lo - os.c0)) * kElem;
  const int sw0 = (int)(n_b - w_lo) + off0;
  const uint32_t nw0_lo = (uint32_t)nw0, q_lo32 = (uint32_t)q_lo;
  unsigned keep_rows = 0;
#pragma unroll
  for (int m1 = 1; m1 < 15; ++m1) {
    const int m = 16 * m1 + m2, sw = sw0 + m1 * m1step;
    const uint32_t n = nw0_lo + (uint32_t)sw;
    const bool keep = m >= halo && m < 256 - halo && (unsigned)sw < (unsigned)w_len &&
                      __umulhi(n, os.magic) * (uint32_t)os.k == n;
    keep_rows |= keep ? 1u << m1 : 0u;
  }
  const float* const st_rd = stage + t * (CG ? 36 : 20);
  __syncthreads();

  for (int b = 0; b < lv.n_scales; ++b) {
    if (b > 0 && (b & (kChunk - 1)) == 0) {    // wave-uniform
      __syncthreads();                         // everyone is done with the previous chunk
      park_gains();                            // asked for eight scales ago
      if (b + kChunk < lv.n_scales) load_gains(b + kChunk);
      __syncthreads();
    }
    if (b == lv.n_plain) {                     // wave-uniform; at most once per workgroup
#pragma unroll
      for (int j = 0; j < 16; ++j) pw[j] = cmulv(pw[j], half_lds[t + 16 * j]);
    }
    const float4* const hs = reinterpret_cast<const float4*>(st_rd + (b & (kChunk - 1)) * kGainRow);
    [[maybe_unused]] const v4f* const hc = reinterpret_cast<const v4f*>(hs);
    const int entry = __builtin_amdgcn_readfirstlane(sc_lds[b]);
    v2f v[16];
    if (need1) {                               // (wave-uniform but for R >= 16 with g < 4)
    switch ((unsigned)entry >> 24) {             // wave-uniform; 16 - j_hi
#define GCWT_WINDOW(hi) case 16 - (hi): if constexpr (CG) gain_first_layer_c<hi>(v, pw, hc); else gain_first_layer<hi>(v, pw, hs); break;
      GCWT_WINDOW(15) GCWT_WINDOW(14) GCWT_WINDOW(13) GCWT_WINDOW(12) GCWT_WINDOW(11) GCWT_WINDOW(10) GCWT_WINDOW(9)
#undef GCWT_WINDOW
      default: if constexpr (CG) gain_first_layer_c<16>(v, pw, hc); else gain_first_layer<16>(v, pw, hs); break;
    }
    idft16v_tail(v);
    switch (sstride) {                         // workgroup-uniform: R, or the column count for R > columns
      case 2: twiddle_to_planes<2>(exw, v, twl + t * kTwPitch); break;
      case 4: twiddle_to_planes<4>(exw, v, twl + t * kTwPitch); break;
      case 8: twiddle_to_planes<8>(exw, v, twl + t * kTwPitch); break;
      case 16: twiddle_to_planes<16>(exw, v, twl + t * kTwPitch); break;
      case 32: twiddle_to_planes<32>(exw, v, twl + t * kTwPitch); break;
      default: twiddle_to_planes<0>(exw, v, twl + t * kTwPitch, sstride); break;
    }
    }
    __syncthreads();
    if (keep_rows) {
#pragma unroll
      for (int k1 = 0; k1 < 16; ++k1) v[k1] = exr[k1 * kPlane];
    }
    __syncthreads();
    if (!keep_rows) continue;                  // nothing of this thread's sixteen rows is kept
    idft16v<true>(v);                          // strict: the rows are k_synth7's every K-th column bit for bit

    // descriptor built from provably wave-uniform words (else hipcc waterfalls every store)
    const int srow = entry & kScaleIndexMask;
    const uint64_t dst_bits = reinterpret_cast<uint64_t>(out0 + (int64_t)srow * a.row_len * kElem);
    const uint32_t dst_lo = __builtin_amdgcn_readfirstlane((uint32_t)dst_bits);
    const uint32_t dst_hi = __builtin_amdgcn_readfirstlane((uint32_t)(dst_bits >> 32));
    float* const dst = reinterpret_cast<float*>(((uint64_t)dst_hi << 32) | dst_lo);
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        dst, 0, __builtin_amdgcn_readfirstlane(ext_bytes), 0x00020000);
#pragma unroll
    for (int m1 = 1; m1 < 15; ++m1) {     // (rows 0 and 15 are never kept: halo >= 16)
      if (!((keep_rows >> m1) & 1u)) continue;
      const v2f z = v[dft16_pos(m1)];
      const uint32_t n = nw0_lo + (uint32_t)(sw0 + m1 * m1step);
      const unsigned vo = (__umulhi(n, os.magic) - q_lo32) * (unsigned)(4 * kElem);
      if (MODE == GCWT_OUT_COMPLEX_C64) {
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, z), rsrc, vo, 0, GCWT_STORE_AUX);
      } else {
        const float p2 = __builtin_fmaf(z.y, z.y, z.x * z.x);
        const float val = MODE == GCWT_OUT_AMPLITUDE_F32 ? __builtin_amdgcn_sqrtf(p2) : p2;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), rsrc, vo, 0, GCWT_STORE_AUX);
      }
    }
  }
}

template <int NCOL, bool CG>
static hipError_t launch_synth7s_n(int mode, const Synth7Args& a, int n_items, int n_channels, hipStream_t st) {
  constexpr int lds = 16 * (16 * NCOL + 1) * 8 + 16 * 18 * 8 + 8 * 320 * 4 + 256 * 4 + 256 * 8;
  static bool attr_done[64] = {};            // per device: one process may drive several
  int dev_ = 0;
  (void)hipGetDevice(&dev_);
  bool& attr_set = attr_done[dev_ & 63];
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_synth7s<GCWT_OUT_AMPLITUDE_F32, NCOL, CG>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)k_synth7s<GCWT_OUT_POWER_F32, NCOL, CG>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)k_synth7s<GCWT_OUT_COMPLEX_C64, NCOL, CG>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  dim3 grid(n_items, n_channels), block(16 * NCOL);
  if (mode == GCWT_OUT_AMPLITUDE_F32)
    hipLaunchKernelGGL((k_synth7s<GCWT_OUT_AMPLITUDE_F32, NCOL, CG>), grid, block, lds, st, a);
  else if (mode == GCWT_OUT_POWER_F32)
    hipLaunchKernelGGL((k_synth7s<GCWT_OUT_POWER_F32, NCOL, CG>), grid, block, lds, st, a);
  else
    hipLaunchKernelGGL((k_synth7s<GCWT_OUT_COMPLEX_C64, NCOL, CG>), grid, block, lds, st, a);
  return hipGetLastError();
}

// (the complex-gain instantiations: a code object of their own, as in synth.hip -- synth_morlet.hip)
hipError_t launch_synth7s_morlet(int mode, int ncol, const Synth7Args& a, int n_items, int n_channels, hipStream_t st);
#ifdef GCWT_SYNTH_MORLET_TU
hipError_t launch_synth7s_morlet(int mode, int ncol, const Synth7Args& a, int n_items, int n_channels, hipStream_t st) {
  return ncol == 16 ? launch_synth7s_n<16, true>(mode, a, n_items, n_channels, st)
                    : launch_synth7s_n<32, true>(mode, a, n_items, n_channels, st);
}
#else
hipError_t launch_synth7s(int mode, int ncol, const Synth7Args& a, int n_items, int n_channels, hipStream_t st) {
  if (n_items == 0) return hipSuccess;
  if (a.seg.os.k < 2) return hipErrorInvalidValue;
  if (a.complex_gains) return launch_synth7s_morlet(mode, ncol, a, n_items, n_channels, st);
  return ncol == 16 ? launch_synth7s_n<16, false>(mode, a, n_items, n_channels, st)
                    : launch_synth7s_n<32, false>(mode, a, n_items, n_channels, st);
}
#endif

#ifndef GCWT_SYNTH_MORLET_TU       // (the interpolating kernel has no complex-gain form)
template <int MODE>
__global__ void __launch_bounds__(kThreadsI, kColsI == 32 ? 4 : 3) k_synthis(const SynthiArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v2f* const ex = reinterpret_cast<v2f*>(smem);
  v2f* const twl = ex + kExElems;                                   // exp(+2 pi i n / 256)
  float* const stage = reinterpret_cast<float*>(twl + 256);         // gains of the pass's scales
  int* const sc_lds = reinterpret_cast<int*>(stage + kSlotsMax * kGainRowI);
  int* const aux_lds = sc_lds + 256;

  const SynthiItem it = a.items[a.channels_fastest ? blockIdx.y : blockIdx.x];
  const SynthiLevel lv = a.levels[it.level];
  const int c = a.channels_fastest ? blockIdx.x : blockIdx.y;   // workspace slot: segment * n_channels + channel
  const int seg = c / a.seg.n_channels, ch = c - seg * a.seg.n_channels;
  const int R = lv.decimation, q = lv.q, lgq = lv.log2q, hop = lv.hop, halo = lv.halo;
  const int lgnb = lv.log2nb, nb = 1 << lgnb;                       // blocks per workgroup
  const int64_t n_b = (int64_t)(lv.blk_base + it.blk0) * hop * R;   // first kept sample of the first block
  const int64_t w_lo = a.seg.w_lo[seg];
  const int64_t w_len = a.seg.w_hi[seg] - w_lo;
  // the level grids are the union over the batch's segments: nothing of these blocks inside the
  // segment's window -> leave (workgroup-uniform)
  if (n_b + (int64_t)nb * hop * R <= w_lo || n_b >= w_lo + w_len) return;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int colw = tid >> 4, t = tid & 15;
  // column -> (block of the group, scale slot of the pass, phase); a "z slot" is a (block, scale) pair
  const int lgns = kLgColsI - lgq - lgnb, ns = 1 << lgns;
  const int zslot = colw >> lgq, p = colw & (q - 1);
  const int slot = zslot & (ns - 1), blk_l = zslot >> lgns;
  const int nzs = kColsI >> lgq;
  const int n_scales = lv.n_scales;
  const int* const scales = a.scale_list + lv.scale_offset;
  const int* const auxs = a.scale_aux + lv.scale_offset;
  for (int i = tid; i < n_scales; i += kThreadsI) { sc_lds[i] = scales[i]; aux_lds[i] = auxs[i]; }
  if (tid < 256) {
    const float2 w = a.tw256[tid];
    twl[tid] = (v2f){w.x, w.y};
  }
  // gains of one pass in LDS, lane t's sixteen values (bins t + 16 j) side by side at a pitch of
  // 20 floats (four conflict-free 16-byte reads per thread), as k_synth7 parks them
  auto stage_slot = [&](int i) { return (i >> 8) * kGainRowI + (i & 15) * 20 + ((i >> 4) & 15); };
  for (int i = tid; i < ns * 256; i += kThreadsI) {
    const int sb = min(it.pass0 * ns + (i >> 8), n_scales - 1);
    stage[stage_slot(i)] = a.gain[(int64_t)(scales[sb] & kScaleIndexMask) * 256 + (i & 255)];
  }

  // Block spectrum XB = FFT_256(x_R[(b hop - halo + n) mod M]) / (256 P), made by 16 threads as
  // conj(IFFT(conj .)) on the packed inverse DFT16 (k_synth7's prologue), left in LDS for all.
  v2f* const fx = ex;
  v2f* const xbs = ex + kSlotsMax * 256;
  {
    v2f v[16];
    if (colw < nb) {
      // blocks past the level's last one reuse it and are never stored
      const int64_t base = (int64_t)(lv.blk_base + min(it.blk0 + colw, lv.nblk - 1)) * hop - halo + t;
      const float2* xr = a.xr + (int64_t)c * a.xr_cstride + lv.xr_offset;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float2 u = xr[(base + 16 * j) & lv.m_mask];
        v[j] = (v2f){u.x, -u.y};
      }
      idft16v(v);
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const float2 w = a.tw256[(t * m) & 255];
        fx[colw * 256 + t * 16 + (m ^ t)] = cmulv(v[dft16_pos(m)], (v2f){w.x, w.y});
      }
    }
    __syncthreads();
    if (colw < nb) {
#pragma unroll
      for (int k1 = 0; k1 < 16; ++k1) v[k1] = fx[colw * 256 + k1 * 16 + (t ^ k1)];
      idft16v(v);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const v2f z = v[dft16_pos(j)];
        xbs[colw * 256 + t + 16 * j] = (v2f){z.x * a.xb_scale, -z.y * a.xb_scale};
      }
    }
    __syncthreads();
  }
  // what never changes for a thread: P[k] = XB[k] W^{k r}, k = t + 16 j, r = p I the phase of its column
  v2f pw[16];
  {
    const int r = p * lv.factor;
    const float2* ltw = a.level_tw + lv.tw_offset;
    const float2 b0 = ltw[t * r], st = ltw[16 * r];
    v2f wcur = (v2f){b0.x, b0.y};
    const v2f wstep = (v2f){st.x, st.y};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      pw[j] = cmulv(xbs[blk_l * 256 + t + 16 * j], wcur);
      wcur = cmulv(wcur, wstep);
    }
  }

  // second half of the transform: thread (a2, col2) takes output samples a2 + 16 c of its column
  const int a2 = tid >> kLgColsI, col2 = tid & (kColsI - 1);
  const int zslot2 = col2 >> lgq, p2 = col2 & (q - 1);
  const int zstride = (256 << lgq) + kZPad;
  v2f* const zw = ex + zslot2 * zstride + (a2 << lgq) + p2;   // + 16 q c

  // phase B geometry: lane-tasks of 4 consecutive samples, 64 of them per wave-task
  const int I = lv.factor;
  const bool six = lv.taps == 6;
  int lgi4 = 0;
  while ((4 << lgi4) < I) ++lgi4;                             // I / 4 = 1 << lgi4
  const int tps = hop * (R >> 2);                             // lane-tasks per (block, scale)
  const float* const coef_lv = a.coef + lv.coef_offset;
  constexpr int kElem = 1;
  // output stride: the descriptor spans the window's columns; window-relative sample sw is recording sample nw0 + sw
  const OutStride os = a.seg.os;
  const int64_t nw0 = a.seg.seg_col[seg] + os.r0 + w_lo;
  const int64_t q_lo = (nw0 + os.k - 1) / os.k, q_hi = (nw0 + w_len + os.k - 1) / os.k;
  const unsigned ext_bytes = q_hi > q_lo ? (unsigned)((q_hi - q_lo) * (4 * kElem)) : 0u;
  float* const out0 = a.out + ((int64_t)ch * a.n_scales * a.row_len + (q_lo - os.c0)) * kElem;
  const int s_base = (int)(n_b - w_lo);                       // window-relative sample of the block's first
  const int pass_end = it.pass0 + it.n_pass;   // of the (n_scales + ns - 1) >> lgns passes of the level's walk
  __syncthreads();

  for (int pass = it.pass0; pass < pass_end; ++pass) {
    const int b0 = pass * ns;
    const bool has_next = pass + 1 < pass_end;
    // next pass's gains: loaded now (nothing of this pass is in flight yet), parked after the exchange
    float nxt[kSlotsMax];
    if (has_next) {
#pragma unroll
      for (int u = 0; u < kSlotsMax; ++u) {
        const int i = tid + kThreadsI * u;
        if (i < ns * 256) {
          const int sb = min(b0 + ns + (i >> 8), n_scales - 1);
          nxt[u] = a.gain[(int64_t)(sc_lds[sb] & kScaleIndexMask) * 256 + (i & 255)];
        }
      }
    }
    // ---- A: 32 columns through the 256-point inverse transform --------------------------------
    {
      const int bs = min(b0 + slot, n_scales - 1);
      const int entry = sc_lds[bs];
      const int kc = aux_lds[bs] & 0xffff;
      const float4* const hs = reinterpret_cast<const float4*>(stage + slot * kGainRowI + t * 20);
      v2f v[16];
      // (16 - j_hi) in the entry's top byte: first-pass inputs j >= j_hi are left out (kernels.h).
      // A wave's four columns belong to one scale slot (q >= 4) or two (q = 2): the smaller window
      // cut of the two, so that the choice is wave-uniform
      unsigned cut = (unsigned)__builtin_amdgcn_readfirstlane(entry) >> 24;
      if (q == 2) {
        const int other = sc_lds[min(b0 + (((colw ^ 2) >> lgq) & (ns - 1)), n_scales - 1)];
        cut = min(cut, (unsigned)__builtin_amdgcn_readfirstlane(min((unsigned)entry >> 24, (unsigned)other >> 24)));
        cut = (unsigned)__builtin_amdgcn_readfirstlane(cut);
      }
      switch (cut) {
#define GCWT_WINDOW(hi) case 16 - (hi): gain_first_layer<hi>(v, pw, hs); break;
        GCWT_WINDOW(15) GCWT_WINDOW(14) GCWT_WINDOW(13) GCWT_WINDOW(12) GCWT_WINDOW(11) GCWT_WINDOW(10) GCWT_WINDOW(9)
#undef GCWT_WINDOW
        default: gain_first_layer<16>(v, pw, hs); break;
      }
      idft16v_tail(v);
      // twiddle W256^{(t - k_c) a - (k_c / q) p}: bins counted from the demodulation centre; the
      // column's values go to exchange plane (t - k_c) mod 16, so that the second half reads its
      // sixteen planes in order (index arithmetic in bytes: one add and one mask per twiddle)
      const unsigned step8 = (unsigned)((t - kc) & 255) << 3;
      unsigned idx8 = (unsigned)((-(kc >> lgq) * p) & 255) << 3;
      v2f* const exw = ex + ((t - kc) & 15) * kPlaneI + colw;
      const char* const twb = reinterpret_cast<const char*>(twl);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        exw[j * kColsI] = cmulv(v[dft16_pos(j)], *reinterpret_cast<const v2f*>(twb + idx8));
        idx8 = (idx8 + step8) & 0x7f8u;
      }
    }
    __syncthreads();
    if (has_next) {
#pragma unroll
      for (int u = 0; u < kSlotsMax; ++u) {
        const int i = tid + kThreadsI * u;
        if (i < ns * 256) stage[stage_slot(i)] = nxt[u];
      }
    }
    {
      v2f v[16];
#pragma unroll
      for (int k1 = 0; k1 < 16; ++k1) v[k1] = ex[k1 * kPlaneI + tid];
      __syncthreads();                      // every plane is read before z takes their place
      idft16v(v);
#pragma unroll
      for (int m1 = 0; m1 < 16; ++m1) zw[(16 * m1) << lgq] = v[dft16_pos(m1)];
    }
    __syncthreads();

    // ---- B: one lane per kept sample: FIR, |.|, one store --------------------------------------------
    // The kept samples of a (block, scale) slot are p = p0 + K j (block-local, inside the window and the workgroup's
    // wave-tasks); they are dealt 64 to a wave, lane j of a run making the j-th.  A lane reads the I-th-rate z window
    // of its sample (element p / I) and the FIR row of its sub-sample position (p mod I) and runs the taps as k_synthi
    // runs them for that sample -- the same products and fused adds in the same order, scalar instead of paired -- so
    // the FIR and |.| run once per kept sample and the kept lanes of a store write consecutive columns.
    {
      const int lgI = lgi4 + 2;
      for (int zi = 0; zi < nzs; ++zi) {                      // everything here is wave-uniform
        const int sl = zi & (ns - 1), bl = zi >> lgns;
        if (b0 + sl >= n_scales || it.blk0 + bl >= lv.nblk) continue;
        const int entry = __builtin_amdgcn_readfirstlane(sc_lds[b0 + sl]);
        const int par = (__builtin_amdgcn_readfirstlane(aux_lds[b0 + sl]) >> 16) & 1;
        const int srow = entry & kScaleIndexMask;
        const uint64_t dst_bits = reinterpret_cast<uint64_t>(out0 + (int64_t)srow * a.row_len * kElem);
        const uint32_t dst_lo = __builtin_amdgcn_readfirstlane((uint32_t)dst_bits);
        const uint32_t dst_hi = __builtin_amdgcn_readfirstlane((uint32_t)(dst_bits >> 32));
        float* const dst = reinterpret_cast<float*>(((uint64_t)dst_hi << 32) | dst_lo);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            dst, 0, __builtin_amdgcn_readfirstlane(ext_bytes), 0x00020000);
        const v2f* const zs = ex + zi * zstride + (halo << lgq) - (kT / 2 - 1);
        const int s_blk = s_base + bl * hop * R;              // window-relative sample of this block's first
        // block-local samples this workgroup stores: the block's kept run, the window, its wave-tasks
        const int p_lo = max(max(0, -s_blk), 256 * it.wt_lo);
        const int p_hi = (int)min(min((int64_t)tps * 4, w_len - s_blk), (int64_t)256 * it.wt_hi);
        if (p_hi <= p_lo) continue;
        const int64_t n_lo = nw0 + s_blk + p_lo;              // recording sample of p_lo
        const int p0 = p_lo + (int)(((-n_lo) % os.k + os.k) % os.k);
        if (p0 >= p_hi) continue;
        const int count = (p_hi - 1 - p0) / os.k + 1;
        const int col0 = (int)((nw0 + s_blk + p0) / os.k - q_lo);   // descriptor column of the slot's first kept
        const float* const coef_p = coef_lv + (int64_t)par * I * kT;
        // a lane's runs are 64 kWavesI kept samples apart: when I divides 256 K its FIR row stays the same along the
        // slot and is loaded once
        const int c_first = (wave + zi) & (kWavesI - 1);
        const bool fixed_row = ((os.k * 64 * kWavesI) & (I - 1)) == 0;
        float4 c0, c1;
        if (fixed_row) {
          const float4* const cp = reinterpret_cast<const float4*>(coef_p + ((p0 + os.k * (c_first * 64 + lane)) & (I - 1)) * kT);
          c0 = cp[0]; c1 = cp[1];
        }
        for (int c = c_first; c * 64 < count; c += kWavesI) {
          const int j = c * 64 + lane;
          if (j >= count) continue;
          const int p = p0 + os.k * j;
          const v2f* const zp = zs + (p >> lgI);
          if (!fixed_row) {
            const float4* const cp = reinterpret_cast<const float4*>(coef_p + (p & (I - 1)) * kT);
            c0 = cp[0]; c1 = cp[1];
          }
          const float cw[kT] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
          float re, im;
          auto taps = [&](auto j0c, auto j1c) {
            constexpr int j0 = decltype(j0c)::value, j1 = decltype(j1c)::value;
            re = zp[j0].x * cw[j0]; im = zp[j0].y * cw[j0];
#pragma unroll
            for (int t2 = j0 + 1; t2 < j1; ++t2) {
              re = __builtin_fmaf(zp[t2].x, cw[t2], re);
              im = __builtin_fmaf(zp[t2].y, cw[t2], im);
            }
          };
          if (six) taps(std::integral_constant<int, 1>(), std::integral_constant<int, kT - 1>());
          else taps(std::integral_constant<int, 0>(), std::integral_constant<int, kT>());
          const float p2v = __builtin_fmaf(im, im, re * re);
          const float res = MODE == GCWT_OUT_AMPLITUDE_F32 ? __builtin_amdgcn_sqrtf(p2v) : p2v;
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, res), rsrc, (unsigned)(col0 + j) * 4u, 0,
                                                GCWT_STORE_AUX);
        }
      }
    }
    __syncthreads();                        // z is read out before the next pass's exchange overwrites it
  }
}

hipError_t launch_synthis(int mode, const SynthiArgs& a, int n_items, int n_channels, hipStream_t st) {
  if (n_items == 0) return hipSuccess;
  if (mode != GCWT_OUT_AMPLITUDE_F32 && mode != GCWT_OUT_POWER_F32) return hipErrorInvalidValue;
  if (a.seg.os.k < 2) return hipErrorInvalidValue;
  static bool attr_done[64] = {};            // per device: one process may drive several
  int dev_ = 0;
  (void)hipGetDevice(&dev_);
  bool& attr_set = attr_done[dev_ & 63];
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_synthis<GCWT_OUT_AMPLITUDE_F32>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)k_synthis<GCWT_OUT_POWER_F32>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  if ((a.channels_fastest ? n_items : n_channels) > 65535) return hipErrorInvalidValue;
  const dim3 grid = a.channels_fastest ? dim3(n_channels, n_items) : dim3(n_items, n_channels), block(kThreadsI);
  if (mode == GCWT_OUT_AMPLITUDE_F32)
    hipLaunchKernelGGL((k_synthis<GCWT_OUT_AMPLITUDE_F32>), grid, block, kLdsBytes, st, a);
  else
    hipLaunchKernelGGL((k_synthis<GCWT_OUT_POWER_F32>), grid, block, kLdsBytes, st, a);
  return hipGetLastError();
}

#endif

}  // namespace gcwt
