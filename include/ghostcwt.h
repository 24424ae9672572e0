/* ghostcwt.h -- C ABI of libghostcwt.so, the MI355X (gfx950) engine behind
 * ghost_amd.wave.ContinuousWaveletTransform.transform().
 *
 * The reference (nelpy/ghost) has no FFI of its own: it is pure Python.  The
 * seam this library replaces is the body of
 *   ghost/wave/transforms.py:142-231   (mean removal, per-scale loop, abs)
 * including everything that loop calls:
 *   ghost/wave/morse.py:84-91, ghost/wave/morseutils.py:93-198   (Morse kernel)
 *   ghost/sigtools/convolution.py:16-87 / 89-216                 (FFT convolution)
 * Each entry point below names the reference lines whose work it does.  The
 * Python class in ghost_amd/wave/transforms.py binds these with ctypes;
 * INTEGRATION.md shows the stub a ghost maintainer would add.
 *
 * Conventions: plain C types only; every function returns 0 on success or a
 * negative gcwt_status; nothing throws across the boundary; the message for the
 * last failure on the calling thread is gcwt_last_error().  The caller owns all
 * buffers it passes in.  A plan owns its device workspace and stream and must be
 * used from one host thread at a time; different plans are independent.
 */
#ifndef GHOSTCWT_H
#define GHOSTCWT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCWT_ABI_VERSION 5

typedef enum {
  GCWT_OK = 0,
  GCWT_ERR_INVALID = -1,     /* bad argument (the reference raises ValueError)   */
  GCWT_ERR_UNSUPPORTED = -2, /* valid request outside what this build handles     */
  GCWT_ERR_NO_DEVICE = -3,   /* no HIP device / HIP runtime failure at init       */
  GCWT_ERR_HIP = -4,         /* a HIP call failed; text in gcwt_last_error()      */
  GCWT_ERR_NOMEM = -5,
  GCWT_ERR_COMM = -6,        /* RCCL unavailable, or a collective could not be ENQUEUED (bad
                                communicator / library state: the same on every rank)          */
  GCWT_ERR_COMM_INCOMPLETE = -7 /* a collective was enqueued and did not complete: a peer rank
                                is gone (or the device failed under it); the communicator is
                                unusable                                                       */
} gcwt_status;

/* What transform() keeps per coefficient.  The reference keeps abs() only
 * (transforms.py:204); power is np.square of it (transforms.py:510). */
typedef enum {
  GCWT_OUT_AMPLITUDE_F32 = 0, /* |W|       float32 [C][S][N]                     */
  GCWT_OUT_POWER_F32 = 1,     /* |W|^2     float32 [C][S][N]                     */
  GCWT_OUT_COMPLEX_C64 = 2    /* W         float32 pairs (re,im) [C][S][N]       */
} gcwt_out_mode;

/* How a scale is evaluated (reported by gcwt_plan_scale_info).  Every method computes
 * the convolution with the reference's own L-tap kernel (morseutils.py:117-149): the
 * choice is made per scale from the measured support of that kernel's exact response. */
typedef enum {
  GCWT_SCALE_SPECTRAL = 0, /* exact response on a decimated band, block IFFT (fast path) */
  GCWT_SCALE_DIRECT = 1,   /* literal L-tap kernel, time domain: short kernels whose
                              response reaches Nyquist           */
  GCWT_SCALE_FULLBAND = 2, /* one FFT convolution over the whole band: kernels whose
                              truncation leaks at every frequency (small beta)   */
  GCWT_SCALE_BLOCKCONV = 3 /* the same convolution by overlap-save: 4096-sample blocks of
                              the recording, all scales of a group per block while its
                              spectrum sits in registers (kernels up to 2560 taps)    */
} gcwt_scale_method;

enum {
  GCWT_X_ON_DEVICE = 1,   /* gcwt_execute: x is a device pointer                 */
  GCWT_OUT_ON_DEVICE = 2, /* gcwt_execute: out is a device pointer               */
  GCWT_REUSE_MEANS = 4,   /* gcwt_execute_block: keep the channel means of the
                             previous call on this plan (same x)                 */
  GCWT_OUT_F64 = 8,       /* host output only: out is float64 (amplitude, power) or
                             float64 pairs (complex), the reference's result dtype
                             (transforms.py:185); widened while the copy is in flight */
  GCWT_HOST_PINNED = 16   /* gcwt_rows_to_host: dst is page-locked (gcwt_host_alloc): the copy goes
                             straight into it, no staging                         */
};

typedef struct gcwt_plan gcwt_plan;

typedef struct {
  int64_t n_samples;           /* N, samples per channel                          */
  int32_t n_channels;          /* C                                               */
  int32_t n_freqs;             /* S                                               */
  double fs;                   /* Hz                                              */
  double gamma, beta;          /* Morse parameters (morse.py:45-51)               */
  const double* freqs_hz;      /* [S] analysis (peak) frequencies, any order      */
  int32_t n_epochs;            /* E >= 1                                          */
  int32_t out_mode;            /* gcwt_out_mode                                   */
  const int64_t* epoch_bounds; /* [2E] start,stop index pairs (transforms.py:202) */
  int32_t device;              /* HIP ordinal; -1 = leave the current device      */
  int32_t block;               /* decimated block length B; 0 = default (256)     */
  double band_eps;             /* response the fast path may ignore outside a scale's
                                  band, relative to the peak; 0 = 2e-7             */
  int32_t max_fft_log2;        /* longest FFT the plan may use, 12..24; 0 = 22, or 23 / 24 when the
                                  longest kernel does not fit time blocks of 2^22 samples (below
                                  0.13 Hz at 30 kHz).  Epochs that need more are cut into overlapping
                                  time blocks                                                          */
  int32_t wavelet_flags;       /* 0 = what transform() uses: first wavelet, 'bandpass'
                                  (morse.py:84-91).  Bits 0-7: order k of the orthogonal
                                  family (0 = first; morseutils.py:181-196); bit 8: 'energy'
                                  normalisation (morseutils.py:119-124, 186-189)         */
  int32_t precision;           /* gcwt_precision; 0 = default (high)                                     */
  int32_t reserved0;           /* must be 0                                                              */
  double support_tol;          /* share of a kernel's energy (L2, relative) a block halo may cut off;
                                  0 = 4.5e-6                                                              */
} gcwt_params;

#define GCWT_WAVELET_ENERGY 0x100
/* Bit 9: the Morlet wavelet instead of a Morse one (morlet.py:56-76).  `gamma` then carries w0, the
 * non-dimensional frequency (> 0; below 5 the wavelet is not admissible but is computed as asked), `beta`
 * is ignored, and the order bits and GCWT_WAVELET_ENERGY must be 0 (else GCWT_ERR_INVALID).  freqs_hz are
 * the frequencies `freq` of Morlet(w0, freq, fs); row f is the 'same'-mode convolution of the recording with
 * Morlet(w0, freq, fs).get_wavelet(), as it is with the Morse kernel otherwise.  Morlet plans do not use the
 * interpolating synthesis (gcwt_plan_info.n_interp = 0).                                                */
#define GCWT_WAVELET_MORLET 0x200

/* The reference computes in float64 (transforms.py:142-143, convolution.py:68-77).  HIGH (the
 * default): x - mean and the forward FFT of every epoch in float64, and every decimation level cuts
 * its slice of the spectrum to zero below the band of its scales (where every gain is under 2e-8 of
 * its peak) before the float32 stages: content BELOW the analysed bands (drift, offsets, 1/f^n
 * backgrounds) up to ~1000 x the quietest band still meets 1e-5 (FAST: ~65 x).  Interference INSIDE a
 * level's band (a mains line between its scales) is good to ~65 x in both (profiles/r04_dynamic_range.md);
 * EXACT below lifts both limits at 3.4 x the time.  FAST: float32 throughout (rounds 1-3). */
typedef enum {
  GCWT_PRECISION_DEFAULT = 0,
  GCWT_PRECISION_FAST = 1,
  GCWT_PRECISION_HIGH = 2,
  GCWT_PRECISION_AUTO = 4,   /* what DEFAULT means since ABI 5: HIGH, watched -- while the float64 spectrum is made,
                              * every scale's loss to the float32 stages of its decimation level is predicted from
                              * the band energies of that spectrum (the level's content against the scale's own), and
                              * the scales predicted above 1.5e-6 of their peak (a mains line inside an analysed band at
                              * more than ~10 x the recording's spread) are made again by EXACT's paths, the others
                              * keep the fast one: the reference's float64 dynamic range (transforms.py:142-143,
                              * convolution.py:68-77) without asking for it.  gcwt_plan_precision_report tells what
                              * happened.  HIGH itself predicts and reports but never reroutes. */
  GCWT_PRECISION_EXACT = 3   /* no decimated path: every scale through the block convolution (kernels up to 1024
                              * taps, block edges faded) or the full-band path -- float64 forward transforms, and
                              * the float32 stages after them only ever see what the scale's own filter lets
                              * through, so an error stays relative to the scale's own output whatever else the
                              * recording holds: a mains line or a drift 1e4 x the recording's std reads 5e-7 /
                              * 2e-6 (profiles/r04_dynamic_range.md).  3.4 x the time of HIGH on the default
                              * wavelet at the headline shape. */
} gcwt_precision;

typedef struct {
  int32_t abi_version;
  int32_t n_levels;            /* distinct decimation factors in use              */
  int32_t n_spectral, n_direct;
  int32_t block;               /* B                                               */
  int32_t max_decimation;      /* largest R                                       */
  int64_t fft_length;          /* P of the longest epoch                          */
  int64_t workspace_bytes;     /* device workspace the plan will allocate         */
  int64_t out_bytes;           /* size of the out buffer gcwt_execute fills       */
  int32_t n_fullband;          /* scales on the full-band path                    */
  int32_t n_interp;            /* of n_spectral: scales made by the interpolating
                                  synthesis (amplitude / power, R >= 16)          */
  int32_t n_blockconv;         /* scales on the block-convolution path            */
  int32_t reserved;
} gcwt_plan_info;

/* Stage timings of the last gcwt_execute on a plan created with profiling on,
 * in milliseconds, measured with HIP events on the plan's stream. */
typedef struct {
  float mean_ms;        /* per-channel mean (transforms.py:143)                   */
  float fwd_fft_ms;     /* forward FFT of every epoch                             */
  float decimate_ms;    /* per-level inverse FFTs producing x_R                   */
  float block_fft_ms;   /* block spectra                                          */
  float synth_ms;       /* fused filter * twiddle * IFFT * |.| * store  (dominant)*/
  float direct_ms;      /* time-domain scales                                     */
  float total_ms;       /* first kernel start to last kernel end                  */
  int32_t synth_launches;
  float fullband_ms;    /* full-band scales (filter, product, inverse FFT, store) */
  float interp_ms;      /* of synth_ms: the interpolating synthesis kernel        */
  float blockconv_ms;   /* block-convolution scales (block spectra, scales)        */
} gcwt_timings;

/* Library / device ------------------------------------------------------- */
int gcwt_abi_version(void);
const char* gcwt_last_error(void);
int gcwt_device_count(int* count);
int gcwt_device_name(int device, char* buf, size_t buflen);
/* PCI bus id of a device ("0000:c1:00.0"): a launcher looks its NUMA node up in sysfs to pin the
 * rank's host threads beside its GPU. */
int gcwt_device_pci_bus_id(int device, char* buf, size_t buflen);
int gcwt_set_device(int device);
int gcwt_current_device(int* device);
int gcwt_device_malloc(void** ptr, size_t bytes);
int gcwt_device_free(void* ptr);
int gcwt_memcpy_h2d(void* dst, const void* src, size_t bytes);
int gcwt_memcpy_d2h(void* dst, const void* src, size_t bytes);
int gcwt_device_memset(void* dst, int value, size_t bytes);
int gcwt_device_synchronize(void);
/* Free and total bytes of the current device's memory (for sizing time blocks). */
int gcwt_device_memory(size_t* free_bytes, size_t* total_bytes);
/* Page-locked host memory for results: a destination the device's copy engines write at the link's
 * rate, with no staging copy and no first-touch page faults (what a fresh array of the reference's
 * result size, transforms.py:185, costs on the host). */
int gcwt_host_alloc(void** ptr, size_t bytes);
int gcwt_host_free(void* ptr);
/* A rectangle of a device-resident result (gcwt_execute with GCWT_OUT_ON_DEVICE) to the host: n_rows rows of
 * row_elems float32 (complex results: two per sample), src_pitch elements apart on the device, to rows dst_pitch
 * elements apart in dst.  flags: GCWT_OUT_F64 -- dst is float64, the reference's result dtype (transforms.py:185,
 * 203-204): float32 over the link, widened by a standing pool of host threads; GCWT_HOST_PINNED -- dst is
 * page-locked (else it goes through a pinned staging ring and dst_pitch must equal row_elems).  What ContinuousWaveletTransform.amplitude does on first
 * access, and how any (scale, sample) range of a result is read without moving the rest (transforms.py:496-527). */
int gcwt_rows_to_host(const float* d_src, int64_t src_pitch, int64_t n_rows, int64_t row_elems, void* dst,
                      int64_t dst_pitch, int flags);
/* Binned cross-spectra of channel pairs from a device-resident complex result, on the device that holds it
 * (csrc/coherence.hip).  pairs: n_pairs x 2 channel indices (a != b, both < n_channels).  d_rows: complex64 rows
 * [channel][scale] pitch elements apart, as gcwt_execute leaves them with GCWT_OUT_ON_DEVICE and out_mode complex.
 * Bin m holds the columns [m window, min((m + 1) window, n_cols)), window >= 2; there are B = ceil(n_cols / window)
 * bins of cnt_m columns.  With Sxy = sum W[a] conj(W[b]), Sxx = sum |W[a]|^2 and Syy = sum |W[b]|^2 over a bin:
 *   d_cross [P][S][B]     complex64  Sxy / cnt_m   (angle > 0: channel b lags channel a)
 *   d_power [C][S][B]     float32    Sxx / cnt_m, every channel
 *   d_coherence [P][S][B] float32    |Sxy|^2 / (Sxx Syy) in [0, 1]; exactly 0 where Sxx Syy == 0 (bins inside an
 *                                    epoch gap: all three outputs are 0 there)
 * Any of the three may be NULL; their rows are out_pitch (>= B) elements apart.  The sums are float32 in a fixed order
 * that does not depend on which other pairs are asked for: a pair gives the same bits alone and among all pairs.
 * A bin shorter than the wavelet's duration at a scale reads close to 1 whatever the signals: a property of the
 * estimator.  Plan-independent, like gcwt_rows_to_host; the device is the one that holds d_rows.  Arguments are
 * checked before any device call (GCWT_ERR_INVALID). */
int gcwt_coherence(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                   const int32_t* pairs, int32_t n_pairs, int64_t window,
                   float* d_power, float* d_cross, float* d_coherence, int64_t out_pitch);
/* Binned phase-amplitude coupling inside every channel of a device-resident complex result, on the device that holds
 * it (csrc/coupling.hip): does the amplitude of row a ride on the phase of row p?  d_rows, pitch, n_cols, window and
 * the bins are those of gcwt_coherence.  Phase rows [phase_first, phase_first + n_phase) = P rows and amplitude rows
 * [amp_first, amp_first + n_amp) = A rows, both inside [0, n_scales); they may overlap.  With u_p = W[c][p] / |W[c][p]|
 * (0 where that is 0), M = sum |W[c][a]| u_p and S = sum |W[c][a]| over a bin:
 *   d_vector [C][P][A][B]  complex64  M / cnt_m    (its angle: the phase of row p at which row a is strongest)
 *   d_mvl [C][P][A][B]     float32    |M| / S in [0, 1], the normalised mean vector length; exactly 0 where S == 0
 *   d_amplitude [C][A][B]  float32    S / cnt_m
 * Any of the three may be NULL; their rows are out_pitch (>= B) elements apart.  Bins inside an epoch gap are exactly
 * 0 in all three.  The sums are float32 in gcwt_coherence's fixed order and the normalisation is a prescribed sequence
 * of correctly rounded operations (coupling.hip), neither depending on which other rows are asked for: a cell (p, a)
 * gives the same bits alone and inside any larger ranges.  A bin shorter than about one period of the phase row reads
 * high whatever the signal (one effective sample): a property of the estimator, and the reason a raw mvl is read
 * against its shift surrogates (gcwt_coupling_surrogates below).  Plan-independent; the device is the one that holds
 * d_rows.  Arguments are checked before any device call (GCWT_ERR_INVALID). */
int gcwt_coupling(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                  int32_t phase_first, int32_t n_phase, int32_t amp_first, int32_t n_amp, int64_t window,
                  float* d_vector, float* d_mvl, float* d_amplitude, int64_t out_pitch);
/* Shift-surrogate statistics of gcwt_coupling's mvl, on the device that holds the rows (csrc/coupling_surrogates.hip).
 * d_rows ... window, the bins, u_p, |W[c][a]|, M, S and cnt_m are exactly those of gcwt_coupling, with window <=
 * GCWT_COUPLING_SURROGATES_MAX_WINDOW (a bin is held in the LDS of one compute unit).  shifts: n_shifts = K (2 .. 4096)
 * shifts in columns, each in [0, window), in HOST memory; one list serves every channel, cell and bin.  For a shift L
 * the surrogate of a bin with first column b moves the amplitude row circularly inside the bin:
 *   M_L = sum_{r = 0}^{cnt_m - 1} |W[c][a][b + (r + L') mod cnt_m]| u_p(b + r),   L' = L mod cnt_m
 *   mvl_L = min(|M_L| / S, 1), exactly 0 where S == 0   (S does not change under the shift)
 * (L' differs from L only in the short last bin.)  With T = sum_k mvl_k and Q = sum_k mvl_k^2 over the list, accumulated
 * in float64 in a fixed order that depends on K alone (coupling_surrogates.hip), each result rounded to float32 once:
 *   d_mean [C][P][A][B]           float32  T / K
 *   d_sd [C][P][A][B]             float32  sqrt(max(0, (Q - T^2 / K) / (K - 1)))
 *   d_count_ge [C][P][A][B]       int32    the number of k with mvl_k >= mvl_0 as float32, mvl_0 the L = 0 value: the
 *                                          p-value of the observed mvl is (1 + count_ge) / (K + 1)
 *   d_surrogates [K][C][P][A][B]  float32  every mvl_k, or NULL
 * Any may be NULL, but not all; their rows are out_pitch (>= B) elements apart.  The arithmetic of a term and the order
 * of every float32 sum are gcwt_coupling's: mvl_L at L = 0 has the bits of its d_mvl, a cell (p, a) gives the same bits
 * alone and inside any larger ranges, and two runs give the same bits.  The shift is bin-local and circular: it keeps
 * the non-stationarity of the recording out of the null, never reads across an epoch gap and leaves S fixed.  The price:
 * the surrogates decorrelate only if the bin spans several coherence times of the phase rhythm -- a perfectly periodic
 * rhythm gives z near 0 however strong its coupling; a bin partly inside a gap has surrogates biased low; a bin wholly
 * inside a gap is 0 in every output but count_ge = K (p = 1, z = 0).  Plan-independent; the device is the one that
 * holds d_rows.  Arguments -- every shift among them -- are checked before any device call (GCWT_ERR_INVALID); a device
 * that does not grant the kernel its LDS is GCWT_ERR_HIP. */
enum { GCWT_COUPLING_SURROGATES_MAX_WINDOW = 2048 };
int gcwt_coupling_surrogates(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                             int32_t phase_first, int32_t n_phase, int32_t amp_first, int32_t n_amp, int64_t window,
                             const int64_t* shifts, int32_t n_shifts, float* d_mean, float* d_sd, int32_t* d_count_ge,
                             float* d_surrogates, int64_t out_pitch);
/* Event-locked averages of the rows of a device-resident complex result, on the device that holds it
 * (csrc/triggered.hip).  d_rows, pitch and n_cols are those of gcwt_coherence; the rows are [row_first, row_first +
 * n_rows) inside [0, n_scales).  events: n_events (1 .. 2^24 = E) event columns in HOST memory, in any order, repeats
 * allowed; the entry copies them to the device and frees the copy.  before, after >= 0 columns around an event: L =
 * before + after + 1 <= n_cols lags, lag l standing for column e_k - before + l, and every event must satisfy before
 * <= e_k and e_k + after < n_cols.  For every channel c, row r and lag l, with w_k = (re, im) = W[c][r][e_k - before
 * + l], every operation a single correctly rounded float32 one:
 *   r2_k = fmaf(im, im, re * re)     a_k = sqrt(r2_k)
 *   inv_k = a_k > 0 ? 1 / a_k : 0    u_k = (re * inv_k, im * inv_k)
 *   A = sum a_k    P = sum r2_k    Ev = sum w_k    V = sum u_k
 *   d_amplitude [C][n_rows][L]  float32    A / E        d_power [C][n_rows][L]   float32    P / E
 *   d_evoked [C][n_rows][L]     complex64  Ev / E       d_vector [C][n_rows][L]  complex64  V / E
 *   d_itpc [C][n_rows][L]       float32    min(sqrt(fmaf(V.y, V.y, V.x * V.x)) / E, 1), the inter-trial phase coherence
 * Every sum is made of four interleaved chains -- chain j adds the terms of the events k = j, j + 4, j + 8, ... one
 * after the other, from an exact 0 -- combined as (X0 + X1) + (X2 + X3).  The order depends on the event list alone: a
 * cell (c, r, l) has the same bits alone, inside any larger run of rows, and at the same absolute lag inside any other
 * (before, after).  Permuting the events changes the chains and with them the low bits.  Zero columns (the gaps between
 * epochs) add exact zeros.  Any output may be NULL, but not all; their rows are out_pitch (>= L) elements apart.  The
 * ITPC of E independent phases reads about 0.89 / sqrt(E), not 0: a property of the estimator; no surrogate statistics
 * are made.  Plan-independent; the device is the one that holds d_rows.  Arguments -- every event among them -- are
 * checked before any device call (GCWT_ERR_INVALID; the message names the first offending event's index). */
int gcwt_triggered(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                   int32_t row_first, int32_t n_rows, const int64_t* events, int64_t n_events,
                   int64_t before, int64_t after,
                   float* d_amplitude, float* d_power, float* d_evoked, float* d_vector, float* d_itpc,
                   int64_t out_pitch);
/* Band-limited analytic signals from the rows of a device-resident complex result, on the device that holds it
 * (csrc/bandpass.hip): the weighted sum of a band's rows at every column, i.e. the inverse transform restricted to the
 * band.  d_rows, pitch and n_cols are those of gcwt_coherence.  bands: n_bands (first, count) pairs in HOST memory, band
 * k the rows first .. first + count - 1 = R rows inside [0, n_scales); bands may overlap and repeat.  g, h: n_scales
 * float32 weights each in HOST memory, finite, h >= 0 (ghost_amd.engine.band_weights makes them so that a sinusoid of
 * amplitude A well inside a band reads envelope = A and power = A^2).  The entry copies table and weights to the device
 * and frees the copy.  For every channel c, band b and column t, with w_r = (re, im) = W[c][r][t], the rows taken in
 * ascending r, each sum starting from an exact 0 and every operation a single correctly rounded float32 one:
 *   x = fmaf(g[r], w_r.re, x)    y = fmaf(g[r], w_r.im, y)    p = fmaf(h[r], fmaf(w_r.im, w_r.im, w_r.re * w_r.re), p)
 *   d_analytic [C][n_bands][n_cols]  complex64  (x, y)     (its angle: the band's phase)
 *   d_envelope [C][n_bands][n_cols]  float32    sqrt(fmaf(y, y, x * x))
 *   d_power [C][n_bands][n_cols]     float32    p
 * The chain of a cell depends on its band's rows alone: a cell has the same bits asked for alone, among any other bands
 * in any position of the list, for any column count, and on a second call.  Zero columns (the gaps between epochs) give
 * exact zeros.  Rounding, with u = 2^-24 and T = sum |g_r| |w_r|: |analytic - exact| <= sqrt(2) R u T; envelope that plus
 * 2 u |analytic|; power (2 + R) u relative.  Any output may be NULL, but not all; their rows are out_pitch (>= n_cols)
 * elements apart.  g may be NULL if neither analytic nor envelope is asked for, h if power is not.  A band narrower than
 * the wavelet's own response reads low, and the phase of analytic carries each row's sub-sample delay where the rows
 * do: properties of the rows, not of the sum.  Plan-independent; the device is the one that holds d_rows.  Arguments --
 * every band and weight among them -- are checked before any device call (GCWT_ERR_INVALID; the message names the
 * first offending band's index). */
int gcwt_bandpass(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                  const int32_t* bands, int32_t n_bands, const float* g, const float* h,
                  float* d_analytic, float* d_envelope, float* d_power, int64_t out_pitch);
/* The spectral ridge of each band of a device-resident complex result and the instantaneous frequency on it, on the
 * device that holds the rows (csrc/ridge.hip): per column the row of largest weighted modulus in the band, and the rate
 * of phase advance on that row.  d_rows, pitch and n_cols are those of gcwt_coherence.  bands: n_bands (first, count)
 * pairs in HOST memory as for gcwt_bandpass; bands may overlap and repeat.  e: n_scales float32 weights in HOST memory,
 * finite and > 0, which make rows comparable (ghost_amd.engine.ridge_weights makes them so that a sinusoid of amplitude
 * A on a row's frequency reads amplitude = A there).  nu: n_scales float32 in HOST memory, finite and >= 0: the phase
 * advance row r expects per column, 2 pi f_r K / fs with the output stride K.  hz_per_cycle: fs / K, finite and > 0.
 * segments: n_segments (start, stop) pairs in HOST memory, ascending, each holding a column and starting where the one
 * before stops, the first at 0 and the last ending at n_cols (ghost_amd.engine.segments_of): the stretches of columns
 * that belong together on the clock.  The entry copies the tables to the device and frees the copy.  For every channel
 * c, band b (rows first .. first + R - 1) and column t, every operation a single correctly rounded float32 one and no
 * product contracted into a sum that is not written as fmaf:
 *   q_r = e[r] * fmaf(w.im, w.im, w.re * w.re), w = W[c][r][t], the rows walked in ascending r.  The winner is the first
 *     row whose q is larger than every earlier one and than 0: the lowest index among equal maxima.  Where every q_r
 *     is 0 (a gap between epochs) there is no winner.
 *   d_row [C][n_bands][n_cols]        int32    the winner's row index in [0, n_scales), or -1
 *   d_amplitude [C][n_bands][n_cols]  float32  sqrt(q_win); 0 with no winner
 *   d_offset [C][n_bands][n_cols]     float32  the parabolic sub-row position of the maximum of q, in rows: with qm, qp
 *     the q of rows row - 1 and row + 1,  d1 = qm - qp;  s = qm + qp;  d2 = s - 2 * q_win;  offset = (0.5f * d1) / d2.
 *     Exactly 0 where the winner is the band's first or last row, where d2 == 0, and with no winner; otherwise inside
 *     [-0.5, 0.5] up to the rounding of d1 and d2 (q_win >= qm, qp)
 *   d_frequency [C][n_bands][n_cols]  float32  Hz: with [start, stop) the segment that holds t, tm = max(t - 1, start), tp
 *     = min(t + 1, stop - 1), span = tp - tm (0, 1 or 2), a = W[c][row][tp], b = W[c][row][tm], T = float32(2 pi):
 *       re = fmaf(a.re, b.re, a.im * b.im)    im = fmaf(a.im, b.re, -(a.re * b.im))    dphi = atan2f(im, re)
 *       k = rintf(((float)span * nu[row] - dphi) / T)      num = dphi + T * k
 *       scale = hz_per_cycle / (T * (float)span)           frequency = num * scale
 *     k unwraps the advance against the row's own frequency, so an output stride does not alias the result.  NaN where
 *     row == -1, where span == 0 (a segment of one column), and where re and im are both 0.  The arctangent is the
 *     device library's (within 2e-6 rad, measured: profiles/ridge.md); everything else is counted:
 *     tests/ridge_model.py has the bound.
 * A cell depends on nothing but its own band's rows at the columns tm, t and tp: a band gives the same bits alone and
 * among any others, in any order, at any column count or pitch and whichever outputs are asked for, and two runs agree
 * in bits.  There is no chaining of the ridge across columns and one maximum per band: two rhythms in one band need two
 * bands; where the two largest rows are nearly equal the row flickers between them while frequency does not.  Any
 * output may be NULL, but not all; their rows are out_pitch (>= n_cols) elements apart.  Without d_frequency neither
 * the neighbours are fetched nor the arctangent made.  A workgroup takes GCWT_RIDGE_TILE_COLS columns, counted from
 * column 0, of GCWT_RIDGE_GROUP_BANDS consecutive bands of the list.  Plan-independent; the device is the one that
 * holds d_rows.  Arguments -- every band, weight, nu entry and segment among them -- are checked before any device call
 * (GCWT_ERR_INVALID; the message names the first offending index). */
enum { GCWT_RIDGE_TILE_COLS = 512, GCWT_RIDGE_GROUP_BANDS = 4 };
int gcwt_ridge(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
               const int32_t* bands, int32_t n_bands, const float* e, const float* nu, float hz_per_cycle,
               const int64_t* segments, int64_t n_segments,
               int32_t* d_row, float* d_amplitude, float* d_offset, float* d_frequency, int64_t out_pitch);
/* The synchrosqueezed transform of a run of rows of a device-resident complex result, on the device that holds the rows
 * (csrc/squeeze.hip): every coefficient is moved to the frequency cell that its own phase advance names, and what lands
 * in a cell is added.  d_rows, pitch and n_cols are those of gcwt_coherence.  The input rows are row_first .. row_first +
 * n_rows - 1 = R rows inside [0, n_scales).  g, floor2, nu: n_scales float32 each in HOST memory: g any finite weight
 * (ghost_amd.engine.band_weights' g makes the sum over the cells of a column the band's analytic signal), floor2 finite
 * and >= 0, a threshold on |w|^2, nu finite and >= 0 as for gcwt_ridge.  hz_per_cycle, segments and n_segments are
 * exactly gcwt_ridge's.  edges: n_cells + 1 float32 in HOST memory, finite, > 0 and strictly ascending, 1 <= n_cells = L <=
 * GCWT_SQUEEZE_MAX_CELLS: cell l holds the frequencies edges[l] <= f < edges[l + 1] (ghost_amd.engine.squeeze_edges makes
 * them from centre frequencies).  The entry copies the tables to the device and frees the copy.  For every channel c,
 * input row r and column t, with w = W[c][r][t], every operation a single correctly rounded float32 one and no product
 * contracted into a sum that is not written as fmaf:
 *   d_frequency [C][R][n_cols]      float32    Hz: gcwt_ridge's frequency with row = r -- tm, tp, span, a = W[c][r][tp], b =
 *     W[c][r][tm], re, im, dphi, k, num, scale, frequency = num * scale, operation for operation.  NaN where span == 0 and
 *     where re and im are both 0.  It does not depend on floor2.
 *   cell: the largest l with edges[l] <= frequency, found by binary search on the float32 values.  The entry is out where
 *     !(fmaf(w.im, w.im, w.re * w.re) > floor2[r]), where frequency is NaN, where frequency < edges[0] and where frequency
 *     >= edges[L].
 *   d_index [C][R][n_cols]          int32      the output row the entry was added to: l, or L - 1 - l with descending != 0;
 *     -1 where the entry is out
 *   d_coefficients [C][L][n_cols]   complex64  (x, y): from (0, 0), the input rows walked in ascending r, every entry
 *     that is not out does on its output row   x = fmaf(g[r], w.re, x)   y = fmaf(g[r], w.im, y)   -- one chain per cell
 *     and column: gcwt_bandpass's arithmetic, and with one cell that holds every entry its analytic
 *   d_power [C][L][n_cols]          float32    fmaf(y, y, x * x)
 * Columns in a gap between epochs (exact zeros) give exact zeros, index -1 and frequency NaN.  Nothing depends on the
 * column count, the pitch, the tiling, the grouping of the cells or which outputs are asked for, and two runs agree in
 * bits; there are no atomics.  The sum over the cells of a column is the sum of g[r] w over the entries that are not out:
 * the result stays invertible.  There is no second-order (chirp-rate) correction; an entry below the noise carries a
 * noise phase and goes where that says: floor2 is what keeps it out.  Any output may be NULL, but not all; their rows
 * are out_pitch (>= n_cols) elements apart.  Without d_coefficients and d_power nothing is summed.  A workgroup takes
 * GCWT_SQUEEZE_TILE_COLS columns, counted from column 0, of GCWT_SQUEEZE_GROUP_CELLS consecutive output rows, counted
 * from row 0, and walks all R input rows: more cells than one group holds cost another walk.  Plan-independent; the
 * device is the one that holds d_rows.  Arguments -- every table entry, edge and segment among them -- are checked before
 * any device call (GCWT_ERR_INVALID; the message names the first offending index). */
enum { GCWT_SQUEEZE_TILE_COLS = 512, GCWT_SQUEEZE_GROUP_CELLS = 16, GCWT_SQUEEZE_MAX_CELLS = 4096 };
int gcwt_squeeze(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                 int32_t row_first, int32_t n_rows, const float* g, const float* floor2, const float* nu, float hz_per_cycle,
                 const int64_t* segments, int64_t n_segments, const float* edges, int32_t n_cells, int32_t descending,
                 float* d_coefficients, float* d_power, float* d_frequency, int32_t* d_index, int64_t out_pitch);
/* The steps of threshold-crossing detection on float32 traces that lie on a device (csrc/detect_runs.hip): n_traces
 * rows of n_cols (1 .. 2^40 - 1) live columns, pitch (>= n_cols) elements apart -- what gcwt_bandpass leaves in
 * d_envelope / d_power with n_traces = C * n_bands, or any row of an amplitude result.  All are plan-independent and
 * know nothing of bands; the device is the one that holds d_trace; arguments are checked before any device call
 * (GCWT_ERR_INVALID).  Whatever lies between n_cols and pitch may be read and is never used.
 *
 * gcwt_trace_stats: per trace, over its columns that are not exactly 0 (the gaps between epochs are exact zeros in
 * every operator here and must not drag the mean down): n[i] the number of such columns and, with s1 = sum v and s2 =
 * sum v * v in float64 (the product is exact),
 *   mean[i] = s1 / n      sd[i] = sqrt(max(s2 / n - mean^2, 0)), the population sd      both 0 where n == 0
 * n, mean, sd: n_traces entries each in HOST memory.  The sums are made in two steps in a fixed order
 * (csrc/detect_runs.h spells it out): float64 partial sums of every tile of 1024 columns counted from column 0 go to a
 * work array -- a lane adds its 4 adjacent columns in ascending order, a butterfly adds the 64 lanes, the 4 waves are
 * added in ascending order --, then one wave per trace adds the tiles: lane l the tiles l, l + 64, ... in ascending
 * order, and the same butterfly.  No atomics: a trace gives the same bits alone, among other traces and on a second
 * call.  For any order |s1 - exact| <= gamma_n sum |v| and |s2 - exact| <= gamma_n sum v^2, gamma_n = n u / (1 - n u),
 * u = 2^-53.  A NaN or inf column is a column like any other: it is counted and makes mean and sd NaN or inf.  Three
 * numbers per trace cross to the host.
 *
 * gcwt_trace_runs: the maximal runs of columns above a threshold, with their peaks.  lo: n_traces finite thresholds in
 * HOST memory.  Column t of trace i is above iff v[t] > lo[i] -- strictly, so a NaN is not above --; columns -1 and
 * n_cols are not above.  A run is a maximal range [start, stop) of above columns; its peak is the largest value in it
 * and peak_col the smallest column that holds that value.  counts[i] (HOST memory, n_traces entries) is the number of
 * runs of trace i.  If sum counts <= capacity the records of all runs, ordered by trace and then by ascending start,
 * are written to the DEVICE arrays d_start, d_stop, d_peak_col (int64) and d_peak (float32) of capacity entries each;
 * otherwise nothing is written to them and the return is still GCWT_OK: the caller sizes with capacity = 0 (the four
 * arrays may then be NULL) and calls again.  Everything returned is an integer or an exact copy of an input value, so
 * the result is defined bit for bit and does not depend on tiling, wave shape or reduction order.  A run that covers
 * millions of columns has its peak searched by one wave.
 *
 * gcwt_trace_order: exact order statistics of every trace (csrc/trace_order.hip), the bits a sort would give.
 *   Included columns of trace i: t < n_cols with v[t] != 0 under the IEEE comparison -- both zeros are excluded, a NaN
 *     is included: gcwt_trace_stats's rule, so the exact zeros of a gap between epochs never count.  n[i] is their
 *     number.
 *   Key of an included column: with center == NULL, v[t]; otherwise fabsf(v[t] - center[i]), the difference one float32
 *     subtraction rounded to nearest even, subnormals kept, contracted with nothing.  Inclusion is decided on v, not on
 *     the key: a column equal to the centre is included with key +0.
 *   Order: the unsigned order of ord(k) = bits(k) ^ (bits(k) >> 31 ? 0xffffffff : 0x80000000), which is the numeric
 *     order wherever that exists and is made total by -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN, NaNs ordered by
 *     payload.
 *   Output: out[i * n_ranks + j] is the key of rank ranks[i * n_ranks + j] (0-based) among the included columns of
 *     trace i, copied bit for bit; where the rank is >= n[i] -- also when n[i] == 0 -- the bit pattern 0x7fc00000: the
 *     caller compares with n.
 * center (n_traces finite entries, or NULL), ranks (n_traces x n_ranks, each >= 0; n_ranks 1 .. 4), n (n_traces) and out
 * (n_traces x n_ranks) are HOST memory.  Everything returned is an integer, a copy of an input value or of the one
 * prescribed subtraction, so the result is defined bit for bit and does not depend on tiling, digit width, wave shape
 * or the order in which counts are added (integer counts are exact in any order): a trace gives the same bits alone,
 * among other traces and on a second call.  A radix select from the most significant digit down, 11 / 11 / 10 bits:
 * per pass one kernel counts digits and one picks each rank's bin; prefixes and remaining ranks stay on the device, six
 * launches whatever the data, and n_traces x (8 + 4 n_ranks) bytes cross to the host.  NULL pointers, n_ranks outside
 * 1 .. 4, a negative rank and a centre that is not finite are refused with the index of the first offender.
 *
 * gcwt_trace_smooth: a symmetric FIR along every trace, inside segments, optionally after a mean over traces
 * (csrc/trace_smooth.hip) -- the Gaussian smoothing and the consensus trace of a ripple detector.  Every operation is
 * one correctly rounded float32 one, contracted with nothing.
 *   Combine (members given, M = n_members): s = v[m_0], then s = s + v[m_i] in the order of the list (a trace may be
 *     named twice), then s * (float)(1.0 / M): ONE trace, the input of the next step and the only output row.  Without
 *     members every trace is smoothed on its own into output row i.
 *   Smooth: taps w_0 .. w_half are the centre and one side of the window.  Column c of a segment [a, b):
 *       acc = w_0 * v[c];   acc = fmaf(w_k, v[c - k] + v[c + k], acc) for k = 1 .. half in ascending order
 *     where a term whose column lies outside [a, b) is an exact 0.f, whatever the trace holds there (a NaN included):
 *     zero extension at both ends, and a segment never sees its neighbour.  A column in no segment is an exact 0.
 *     half = 0 with w_0 = 1 copies the segments: the consensus trace without smoothing.
 *   Reproducibility: a column's bits depend on its own segment's columns and on the taps alone -- not on the tile,
 *     n_cols, the pitch, the alignment, the other traces or the other segments.  No atomics, no cross-lane sums.
 *   Rounding: with u = 2^-24 and gamma_m = m u / (1 - m u), |out - exact| <= gamma_(half + 1) sum_k |w_k| (|v[c - k]| +
 *     |v[c + k]|) (k = 0 once): each product enters at most half + 1 roundings -- the addition of its pair, its own and
 *     the additions after it; a member mean adds its own M roundings to v before that.
 * taps (half + 1 finite entries; half 0 .. GCWT_SMOOTH_MAX_HALF -- the window counts in columns, so an output stride
 * shortens it), segments (n_segments (start, stop) pairs, ascending, disjoint, each holding a column, inside [0,
 * n_cols); NULL and 0: one segment, every column) and members (n_members trace indices; NULL and 0: none) are HOST
 * memory.  d_out: 1 row (members) or n_traces rows on the device, out_pitch (>= n_cols) elements apart, not overlapping
 * d_trace; nothing is written between n_cols and out_pitch.  The tile and its halo are staged in LDS, (1024 + 2 half) x 4
 * bytes, 36 KB at the limit.  The message of a refusal names the first offending tap, segment or member. */
enum { GCWT_SMOOTH_MAX_HALF = 4096 };
int gcwt_trace_stats(const float* d_trace, int64_t pitch, int64_t n_traces, int64_t n_cols,
                     int64_t* n, double* mean, double* sd);
int gcwt_trace_runs(const float* d_trace, int64_t pitch, int64_t n_traces, int64_t n_cols,
                    const float* lo, int64_t capacity,
                    int64_t* d_start, int64_t* d_stop, int64_t* d_peak_col, float* d_peak, int64_t* counts);
int gcwt_trace_order(const float* d_trace, int64_t pitch, int64_t n_traces, int64_t n_cols,
                     const float* center,                   /* HOST, n_traces entries, or NULL */
                     const int64_t* ranks, int32_t n_ranks, /* HOST, n_traces x n_ranks, 0-based; n_ranks 1 .. 4 */
                     int64_t* n, float* out);               /* HOST: n_traces, n_traces x n_ranks */
int gcwt_trace_smooth(const float* d_trace, int64_t pitch, int64_t n_traces, int64_t n_cols,
                      const float* taps, int32_t half,              /* HOST: w_0 .. w_half */
                      const int64_t* segments, int64_t n_segments,  /* HOST: (start, stop) pairs, or NULL and 0 */
                      const int32_t* members, int32_t n_members,    /* HOST: traces averaged into ONE output trace, or NULL and 0 */
                      float* d_out, int64_t out_pitch);

/* Planning: host only, touches no device.  Replaces the per-call setup of
 * transforms.py:179-185 (wavelet lengths, output allocation) and decides, per
 * scale, the decimation factor and block layout. */
int gcwt_plan_create(gcwt_plan** out, const gcwt_params* params);
void gcwt_plan_destroy(gcwt_plan* plan);
int gcwt_plan_get_info(const gcwt_plan* plan, gcwt_plan_info* info);
/* Per-scale arrays of length S; any pointer may be NULL.  length[] is the
 * reference kernel length L of morse.py:108-122. */
int gcwt_plan_scale_info(const gcwt_plan* plan, int32_t* method, int32_t* decimation,
                         int32_t* halo, int32_t* hop, int64_t* length);
/* What the planner measured on each scale's exact response (arrays of length S, any may
 * be NULL): theta_hi, the radian frequency above which (through the negative
 * frequencies, up to 2 pi) the response stays below band_eps of its peak; support, the
 * distance in samples from the kernel's centre that a block halo must cover; n_bins, the
 * spectrum samples of morseutils.py:130-131 the kernel is built from. */
int gcwt_plan_scale_support(const gcwt_plan* plan, double* theta_hi, double* support,
                            int32_t* n_bins);
/* Stage timings (gcwt_get_timings; the reference's `verbose` print, transforms.py:226-229).  enabled = 1: every stage of
 * an execute lies between two HIP events on its stream; 2: only the synthesis kernels do (synth_ms, interp_ms and
 * synth_launches are filled, total_ms is their span, the other stages read 0) -- the events themselves cost a step of the
 * headline shape 0.19 ms of 13.5, so a loop that is itself being timed asks for level 2; 0: none. */
int gcwt_plan_set_profiling(gcwt_plan* plan, int enabled);
/* After an execute of a plan with precision DEFAULT / AUTO / HIGH: predicted[s] (S floats, may be NULL) is the
 * predicted loss of scale s to the float32 stages of its decimation level, relative to its own output (0 for
 * scales on the exact paths), *worst the largest of them, *n_rerouted how many scales that execute made again by
 * the exact paths (AUTO; 0 for HIGH).  Negative: that many scales were over the threshold and some of them could NOT
 * be made again -- no device memory for the exact sub-plan (gcwt_last_error tells) -- so their rows are the fast
 * path's, what HIGH returns; the execute itself succeeded.  The reference needs no such thing: it is float64 end
 * to end (transforms.py:142-143). */
int gcwt_plan_precision_report(const gcwt_plan* plan, float* predicted, float* worst, int32_t* n_rerouted);
/* Row pitch, in samples, of DEVICE output buffers (0 = dense rows of N, or of the block
 * length).  Rows whose byte offset is not a multiple of 128 make every store straddle
 * cache lines; pad rows to a multiple of 32 samples for full speed when N is not one.
 * Host output buffers are always dense (the library pads internally). */
int gcwt_plan_set_row_pitch(gcwt_plan* plan, int64_t pitch_samples);
/* Output stride K >= 1 (1 = every sample, the default): output column j of a row holds the coefficient at sample
 * n = K j of the recording's own grid (not per epoch), the full-rate result's [..., ::K] -- point sampling, no
 * averaging.  Rows have ceil(N / K) columns: gcwt_plan_info.out_bytes, gcwt_execute's out and the row pitch of
 * gcwt_plan_set_row_pitch count columns, and gcwt_execute_block(start, length) writes the kept samples of
 * [start, start + length), the multiples of K there (any start), as that many columns.  Only the kept samples are
 * stored.  Of the work: the interpolating synthesis (R >= 16) evaluates its FIR and |.| at the kept samples only; the
 * 256-point synthesis skips the block phases that hold no kept sample when 4 divides K (one phase of R left when R
 * divides K) and computes every phase otherwise; the other paths compute every sample and store the kept ones.
 * Allowed from plan creation up to the first upload or execute; GCWT_ERR_INVALID after that or for K < 1;
 * GCWT_ERR_UNSUPPORTED for K > 1 on recordings of 2^31 samples or more. */
int gcwt_plan_set_output_stride(gcwt_plan* plan, int64_t stride);

/* Device side ------------------------------------------------------------ */
/* Allocate workspace, build the Morse filter bank and FFT tables on the
 * device.  Called implicitly by the first gcwt_execute.  Replaces the kernel
 * construction of morse.py:84-91 / morseutils.py:93-198 for every scale. */
int gcwt_plan_upload(gcwt_plan* plan);

/* The transform: transforms.py:142-143 (global mean), :187-204 (per scale, per
 * epoch convolution + abs) for every channel.  x: float32 [C][N] row-major.
 * out: per out_mode, [C][S][N] row-major, scales in the order of freqs_hz.
 * Samples outside every epoch are written as 0 (transforms.py:185). */
int gcwt_execute(gcwt_plan* plan, const void* x, void* out, int flags);

/* Streaming form of the same transform for recordings whose output does not fit
 * in memory: computes samples [start, start+length) of every channel and scale.
 * x is the WHOLE recording, float32 [C][N] (the global mean and the kernels'
 * support around the range are taken from it); out is [C][S][length].  Cheapest
 * when ranges coincide with the plan's time blocks (gcwt_plan_segment_info).
 * This is the overlap-save front end the reference sketches in
 * ghost/wave/transforms.py:529-597 (_cwtft: chunks with both edges discarded). */
int gcwt_execute_block(gcwt_plan* plan, const void* x, void* out, int64_t start, int64_t length,
                       int flags);
/* Time blocks the plan cuts the epochs into: output range [core_start, core_stop). */
int gcwt_plan_segment_count(const gcwt_plan* plan);
int gcwt_plan_segment_info(const gcwt_plan* plan, int segment, int64_t* core_start,
                           int64_t* core_stop, int64_t* fft_length);

/* Filter bank as held on the device, for parity tests of the bank builder:
 * bank: float32 (re,im) [S][B], H_s(2 pi k / (B R_s)), zero rows for direct
 * scales.  Compare with the spectrum of morseutils.py:130-131. */
int gcwt_filter_bank(gcwt_plan* plan, float* bank);
/* Literal kernel of a direct scale: float32 (re,im) [L].  Compare with psi of
 * morseutils.py:149. */
int gcwt_direct_kernel(gcwt_plan* plan, int scale, float* psi);

int gcwt_get_timings(const gcwt_plan* plan, gcwt_timings* t);

/* The operator layer under the transform: FFT convolution of real signals with one kernel,
 * ghost/sigtools/convolution.py:16-87 (fastconv_scipy) / :89-216 (fastconv_fftw) for a
 * kernel in the time domain, :218-402 (fastconv_freq_scipy / _fftw) for a kernel given by
 * its DFT.  A plan is made once per (signal length n, kernel length m, channel count) and
 * reused: it owns its stream, FFT tables, the kernel's spectrum and the workspace.  Signals
 * longer than one FFT run as overlap-save chunks (the reference's chunked overlap-add,
 * convolution.py:68-77); chunks and channels are batched.  fft_log2: 0 = the smallest
 * 2^k >= n + 2 (m - 1) -- one overlap-save chunk (m - 1 samples of history, then the signal and
 * its tail) holds the whole convolution -- at most 2^22; or 12..22 to fix the FFT length F = 2^fft_log2 (the
 * reference's fft_length: chunks of F - m + 1 samples, convolution.py:70). */
typedef struct gcwt_conv_plan gcwt_conv_plan;
int gcwt_conv_plan_create(gcwt_conv_plan** out, int64_t n, int64_t m, int32_t n_channels,
                          int32_t fft_log2, int32_t device);
void gcwt_conv_plan_destroy(gcwt_conv_plan* plan);
int gcwt_conv_plan_info(const gcwt_conv_plan* plan, int64_t* fft_length, int64_t* chunk,
                        int64_t* n_chunks);
/* kernel: float32 [m] real, or (re,im) pairs [m] when is_complex; host or device memory. */
int gcwt_conv_plan_set_kernel(gcwt_conv_plan* plan, const float* kernel, int is_complex,
                              int on_device);
/* kernel_fd: (re,im) pairs, the DFT of the (zero-padded) kernel on the plan's own
 * fft_length-point grid, natural bin order (the kernel_fd argument of
 * convolution.py:218-219 when its length is a power of two the plan can take). */
int gcwt_conv_plan_set_kernel_fd(gcwt_conv_plan* plan, const float* kernel_fd, int on_device);
/* signal: float32 [C][n]; out: (re,im) pairs [C][count], count = n+m-1 ('full', mode 0),
 * n ('same', mode 1, centred as convolution.py:85) or n-m+1 ('valid', mode 2).
 * flags: GCWT_X_ON_DEVICE, GCWT_OUT_ON_DEVICE. */
int gcwt_conv_plan_execute(gcwt_conv_plan* plan, const float* signal, int mode, float* out,
                           int flags);
/* One-shot form: one signal, one kernel, host memory (a plan made and destroyed inside). */
int gcwt_fastconv(const float* signal, int64_t n, const float* kernel, int64_t m,
                  int kernel_is_complex, int mode, float* out, int device);

/* DFT of arbitrary length n (not only powers of two) by the chirp-z identity, the operator
 * of ghost/sigtools/fourier.py:9-52 (chirpz_dft).  x: float32 [n] real, or (re,im) pairs
 * when is_complex; inverse != 0 gives the normalised inverse DFT.  out: (re,im) pairs [n]
 * (host).  n <= 2^21. */
int gcwt_dft(const float* x, int64_t n, int is_complex, int inverse, float* out, int device);

/* Analytic signal x + i*Hilbert(x) of a real signal through an fft_length-point DFT
 * (0 = n, the reference's default: no padding), as ghost/sigtools/analytic.py:22-112
 * (analytic_signal_fftw; the same numbers as scipy.signal.hilbert(x, N=fft_length)[:n]).
 * signal: float32 [n] (host); out: (re,im) pairs [n] (host).  fft_length <= 2^21, any
 * length (the DFTs run as chirp-z transforms on power-of-two FFTs). */
int gcwt_analytic_signal(const float* signal, int64_t n, int64_t fft_length, float* out,
                         int device);

/* The same operators in float64, the reference's own arithmetic and result dtype (complex128 from float64 FFTs:
 * ghost/sigtools/convolution.py:68-87, fourier.py:9-52, analytic.py:22-112) -- for callers that compare element by
 * element, down to a result's zero crossings.  Host memory in and out; out: (re, im) pairs of doubles.
 * gcwt_dft_f64: any n <= 2^23 (powers of two directly, other lengths by the chirp-z identity, phases reduced in
 * integers).  gcwt_fastconv_f64: signal and kernel real or complex; mode 0 'full', 1 'same' (centred as
 * convolution.py:85), 2 'valid'; results beyond 2^24 samples are made by overlap-add over chunks of the signal like
 * convolution.py:70-77's (kernels up to 2^23 taps then).  The analytic signal is two gcwt_dft_f64 calls around the
 * one-sided mask (ghost_amd.sigtools.analytic_signal_hip(precision='high')). */
int gcwt_dft_f64(const double* x, int64_t n, int is_complex, int inverse, double* out, int device);
int gcwt_fastconv_f64(const double* signal, int64_t n, int signal_is_complex, const double* kernel, int64_t m,
                      int kernel_is_complex, int mode, double* out, int device);

/* Multi-GPU control plane (one process per GPU; RCCL over xGMI).  The data path
 * has no collective: channels are sharded.  The filter bank is broadcast once
 * from rank 0 as BASELINE.json asks; barrier/all-reduce exist for bench timing. */
typedef struct gcwt_comm gcwt_comm;
#define GCWT_COMM_ID_BYTES 128
int gcwt_comm_unique_id(void* id128);
int gcwt_comm_create(gcwt_comm** out, int rank, int n_ranks, const void* id128);
void gcwt_comm_destroy(gcwt_comm* comm);
/* Tears a communicator down after a failed collective without waiting for anything in flight
 * (ncclCommAbort; its stream and scratch are left to process exit).  gcwt_comm_destroy is for
 * communicators whose operations have all completed. */
void gcwt_comm_abort(gcwt_comm* comm);
int gcwt_comm_barrier(gcwt_comm* comm);
int gcwt_comm_allreduce_max(gcwt_comm* comm, double* value);
int gcwt_comm_broadcast_bank(gcwt_comm* comm, gcwt_plan* plan, int root);

#ifdef __cplusplus
}
#endif
#endif /* GHOSTCWT_H */
