/* ghostcwt_debug.h -- test-only hooks of libghostcwt.so: read back the
 * intermediate buffers of the last gcwt_execute so each stage can be checked
 * against the NumPy model in tests/decimated_model.py.  Not part of the drop-in
 * surface. */
#ifndef GHOSTCWT_DEBUG_H
#define GHOSTCWT_DEBUG_H
#include "ghostcwt.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  GCWT_DEBUG_SPECTRUM = 0,      /* X~[k1][k2] = X[k1 + P1 k2], P complex values; only
                                   k2 < 2048 (positive frequencies) is filled            */
  GCWT_DEBUG_DECIMATED = 1,     /* x_R of one level, M = P/R complex values (times P)    */
  GCWT_DEBUG_BLOCK_SPECTRA = 2  /* XB[blk][k] of one level, nblk*B complex values        */
};

/* Named switches read when a plan is created (csrc/options.h): which kernel instantiation or planning
 * layout is used -- "synth16", "synth_cols", "fuse_blocks", "slow_fft", "level_streams", "interp",
 * "interp_grid", "interp_lgnb", "synth_streams", "merge_levels", "split_levels", "early_interp",
 * "interp_split_r", "bc_chunk_blocks" (all compute the same rows; the tests compare them) and the budgets "batch_bytes", "stage_floats".  Options that change
 * accuracy or exist for measurements ("halo_margin", "interp_q", "interp_min_r", "prune_inputs",
 * "clock_phases", "synth_kernel", "synth_drop_stores", "clock_probe", "synthi_pad_kb") are refused with
 * GCWT_ERR_UNSUPPORTED by the product library: libghostcwt_measure.so takes them.  clear != 0 returns
 * the option to its default.  Process-wide; not part of the drop-in surface. */
int gcwt_debug_set_option(const char* name, int64_t value, int clear);
int gcwt_debug_level_count(const gcwt_plan* plan);
int gcwt_debug_level_info(const gcwt_plan* plan, int epoch, int level, int32_t* decimation,
                          int32_t* halo, int32_t* hop, int32_t* nblk, int64_t* m);
/* Bins of a level's 256-point grid that lie below zero frequency (heavy-tailed wavelets: the level's
 * band is [-shift, 256 - shift) * 2 pi / (256 R); 0 for the default wavelet). */
int gcwt_debug_level_band_shift(const gcwt_plan* plan, int level, int32_t* shift);
/* precision = high: x_R of the level's decimation is made from a slice of the spectrum that is zero
 * below theta_cut / 2 and raised (half a cosine) to one at theta_cut radians per sample -- below the band
 * of every scale that reads it (planner.h: LevelPlan::taper_hi); 0: no cut.  Per scale: theta_lo, up to
 * which its exact response stays under 2e-8 of its peak. */
int gcwt_debug_level_low_cut(const gcwt_plan* plan, int level, double* theta_cut);
int gcwt_debug_scale_theta_lo(const gcwt_plan* plan, double* theta_lo);
/* Small device-resident executes replay a HIP graph from the third call with the same arguments on: 1 = a graph is
 * instantiated, 0 = none (yet), -1 = capture failed once and the plan runs eagerly. */
int gcwt_debug_graph_state(const gcwt_plan* plan);
/* 1 when the plan's last run took the channel sums inside the forward column pass and the mean's transform out of the
 * row pass's input (one segment that is the whole recording, FFTs up to 2^22 points, every scale spectral; option
 * fold_mean = 0 turns it off), 0 when a pass of its own over x made them (transforms.py:142-143 either way). */
int gcwt_debug_mean_folded(const gcwt_plan* plan);
/* precision = auto / high: the two terms of the last execute's prediction for workspace slot 0 of its last batch
 * (S floats each: float32 rounding of the level's stages; what the level's slice of the spectrum leaves out), the
 * energy each level's x_R held (one float per level; may be NULL) and the band energies they come from (384 floats,
 * may be NULL: sum of |X[k]|^2 over the bins 0 < k < P / 2 of band (bits of (float) k >> 19) - 127 * 16, sixteen
 * bands per octave -- summed by the forward row pass, csrc/fwd64.hip: row_band_sums).  Scales off the decimated path
 * and levels without a scale read as zero. */
int gcwt_debug_precision_terms(gcwt_plan* plan, float* rounding, float* left_out, float* level_energy,
                               float* band_energy);
/* Block convolution (GCWT_SCALE_BLOCKCONV): the scales in order of kernel length (`order`: n_blockconv entries, at
 * most max_order are written) and the groups of consecutive entries that share the spectra of their blocks (at
 * most max_groups are written): blocks of `hop` output samples from the 4096 recording samples that start `back`
 * before them.  Returns the number of groups. */
int gcwt_debug_blockconv_groups(const gcwt_plan* plan, int32_t* first, int32_t* count, int32_t* hop,
                                int32_t* back, int32_t* order, int max_groups, int max_order);
/* Segments of equal FFT length are launched together: first segment and size of the batch
 * that `segment` belongs to. */
int gcwt_debug_batch_of(const gcwt_plan* plan, int segment, int32_t* first, int32_t* count);
int gcwt_debug_fetch(gcwt_plan* plan, int what, int channel, int epoch, int level, float* dst,
                     int64_t max_complex);
/* The lists the synthesis kernels walk, one per level and one after the other: entry i is scale row[i], and for
 * level l the entries level_first[l] .. level_first[l + 1] - 1 (level_first: n_levels + 1 values), of which the
 * first level_plain[l] are the kernels of odd length (every scale of a Morlet plan) and the rest carry the level's
 * half-sample ramp (Synth7Level::n_plain).  j_hi[i]: how many of the sixteen first-layer inputs k_synth7 computes
 * for the entry (9 .. 16; csrc/kernels.hip: k_scale_windows), read back from the device list's top byte -- 0 as
 * long as the plan's tables are not on the device (before gcwt_plan_upload or the first execute).  Any pointer may
 * be NULL.  Returns the number of entries; row and j_hi are filled only when max_entries holds them. */
int gcwt_debug_scale_lists(gcwt_plan* plan, int32_t* level_first, int32_t* level_plain, int32_t* row,
                           int32_t* j_hi, int32_t max_entries);
/* The workgroup items of one synthesis kernel for launch batch `batch` (0 .. in the order of gcwt_debug_batch_of),
 * exactly as gcwt_plan_upload sends them and in that order (csrc/work_items.h), as flat int32 records:
 *   SYNTH16                  level, scale, blk0, nblk
 *   SYNTH7, _WIDE, _NARROW   level, blk0, rtile, 0        (k_synth7, its wide-halo and its 16-column list)
 *   INTERP                   one value first, the number of items of the first launch (the levels below option
 *                            interp_split_r); then level, blk0, pass0, n_pass, wt_lo, wt_hi
 *   PIPELINED                one value first, the number of items of the first launch (I > 4; the second: I = 4);
 *                            then level, blk0, round0, n_rounds
 * Needs no device and no upload.  Returns the number of int32 values (out is filled only when max_ints holds them;
 * out may be NULL), or a negative error. */
enum gcwt_debug_items {
  GCWT_DEBUG_ITEMS_SYNTH16 = 0,
  GCWT_DEBUG_ITEMS_SYNTH7 = 1,
  GCWT_DEBUG_ITEMS_SYNTH7_WIDE = 2,
  GCWT_DEBUG_ITEMS_SYNTH7_NARROW = 3,
  GCWT_DEBUG_ITEMS_INTERP = 4,
  GCWT_DEBUG_ITEMS_PIPELINED = 5
};
int gcwt_debug_work_items(const gcwt_plan* plan, int kernel, int batch, int32_t* out, int32_t max_ints);
/* The exact (real) response G of one scale's reference kernel at theta = 2 pi a[i] / b,
 * i < n, evaluated on the HOST by the same code the device bank builder runs
 * (csrc/morse_exact.h).  Needs no GPU. */
int gcwt_debug_exact_gain(const gcwt_plan* plan, int scale, const int64_t* a, int64_t b, int64_t n,
                          double* gain);
/* Interpolating synthesis (csrc/synthi.hip) of one level: phases q of the block transform per
 * (block, scale) -- 0 when the level is made by the FFT-per-sample kernels -- the interpolation
 * factor I = R / q, the design band (fraction of the oversampled Nyquist) and the planner's bound
 * on the error the interpolation adds, relative to a scale's peak gain.  coef (may be NULL):
 * [2][I][8] floats, the 8-tap interpolators of the I sub-sample positions for kernels of odd and
 * of even length.  demod (may be NULL): per SCALE of the plan, the bin of its level's 256-point
 * grid its oversampled output is demodulated by.  Host only. */
int gcwt_debug_interp_level(const gcwt_plan* plan, int level, int32_t* q, int32_t* factor,
                            double* alpha, double* err_bound, float* coef, int64_t max_floats);
int gcwt_debug_scale_demod(const gcwt_plan* plan, int32_t* demod);
/* Per scale: how far below zero frequency (radians per sample) the response of its kernel still
 * exceeds band_eps of the peak (planner.h: ScalePlan::theta_neg; 0 for the default wavelet). */
int gcwt_debug_scale_theta_neg(const gcwt_plan* plan, double* theta_neg);
/* 1 in libghostcwt_measure.so (`make -C ghost_amd/csrc measure`: -DGCWT_MEASURE), the build that
 * carries the measurement hooks -- stores dropped / barriers removed (GHOSTCWT_SYNTH_DROP_STORES,
 * results WRONG), the in-kernel clock probe, the slower k_synth8 (GHOSTCWT_SYNTH_KERNEL=8);
 * 0 in the product library, which has none of those paths. */
int gcwt_debug_measure_build(void);
/* Measure build only, plans created with GHOSTCWT_CLOCK_PROBE=1 in the environment: the shader
 * clock the synthesis workgroups ran at since the last call (sum of s_memtime deltas over
 * sum of s_memrealtime deltas, one pair per workgroup: MI355X_MICROARCH.md "DVFS
 * give-back" item 6) and the summed workgroup lifetimes. */
int gcwt_debug_clock(gcwt_plan* plan, double* ghz, double* workgroup_seconds);
/* Measurement only: GB/s this device reaches on `bytes` (>= 64 MiB) of HBM with a plain
 * 16-byte fill, a 16-byte copy (read + write counted), or the store pattern of the
 * synthesis kernel (128-byte runs into 100 rows a megasample apart).  Best of three. */
enum { GCWT_BW_FILL = 0, GCWT_BW_COPY = 1, GCWT_BW_SYNTH_STORES = 2,
       GCWT_BW_SYNTHI_STORES = 3 /* k_synthi's: 1 KB runs per wave, 53 KB visits, four rows per pass, three
                                    256-thread workgroups per CU (profiles/r04_store_study.md) */ };
int gcwt_debug_bandwidth(int pattern, size_t bytes, double* gb_per_s);

/* Whole-result properties of a device-resident result of rows_per_channel x n_channels rows (at most 65535) of
 * n_valid_floats floats, row_pitch_floats apart: how many values are Inf / NaN, and how many values of a
 * channel c >= distinct differ in any bit from the same row of channel c % distinct (a caller that tiled
 * `distinct` recordings over its channels expects 0: bench.py). */
int gcwt_debug_check_output(const void* out_device, int64_t row_pitch_floats, int64_t n_valid_floats,
                            int32_t rows_per_channel, int32_t n_channels, int32_t distinct,
                            int64_t* n_nonfinite, int64_t* n_mismatched);


/* Host only: the tasks gcwt_coherence cuts a pair list into.  Channels form tiles of GCWT_COHERENCE_TILE; a task is
 * one (tile_a <= tile_b) -- times every scale and run of bins -- and accumulates the cells (i, j) = channel i of tile
 * a with channel j of tile b that its entries name.  entries: n_pairs x 3 = (cell i * GCWT_COHERENCE_TILE + j,
 * conjugate, output row = index into pairs); entry_first [n_tasks + 1]: task t owns entries [entry_first[t],
 * entry_first[t + 1]).  conjugate = 1: the pair was asked for as (channel of the cell's j, channel of its i).  flags:
 * bit 0 / 1 -- the task writes the power rows of tile a's / tile b's channels; every tile is written by exactly one
 * task, and tiles that no pair touches get a task of their own without entries, after all others.  Returns the
 * number of tasks (arrays, any of which may be NULL, are filled when max_tasks holds them) or an error code < 0. */
enum { GCWT_COHERENCE_TILE = 8 };
int gcwt_debug_coherence_tasks(int32_t n_channels, const int32_t* pairs, int32_t n_pairs, int32_t* tile_a,
                               int32_t* tile_b, int32_t* flags, int32_t* entry_first, int32_t* entries,
                               int32_t max_tasks);

/* Host only: the grid gcwt_coupling launches.  The phase rows form tiles of GCWT_COUPLING_TILE_PHASE and the amplitude
 * rows tiles of GCWT_COUPLING_TILE_AMP, counted from the first row of each range (the last tile of either may be
 * ragged); a workgroup takes one (channel, run of run_bins bins, phase tile, amplitude tile).  n_blocks counts the
 * workgroups: every tile of every (channel, run), the (channel, run)s padded to a multiple of 8 so that the tiles of
 * one of them lie 8 workgroups apart.  Any pointer may be NULL.  Returns GCWT_OK or an error code < 0. */
enum { GCWT_COUPLING_TILE_PHASE = 4, GCWT_COUPLING_TILE_AMP = 8 };
int gcwt_debug_coupling_grid(int32_t n_channels, int64_t n_cols, int32_t n_phase, int32_t n_amp, int64_t window,
                             int32_t* n_phase_tiles, int32_t* n_amp_tiles, int64_t* run_bins, int64_t* n_runs,
                             int64_t* n_blocks);

/* Host only: the grid gcwt_coupling_surrogates launches.  The tiles are formed as gcwt_coupling's, of
 * GCWT_COUPLING_SURROGATES_TILE_PHASE x GCWT_COUPLING_SURROGATES_TILE_AMP rows; a workgroup of
 * GCWT_COUPLING_SURROGATES_WAVES waves takes one (channel, bin, phase tile, amplitude tile) and every shift.  n_blocks
 * counts the workgroups: every tile of every (channel, bin), the (channel, bin)s padded to a multiple of 8 so that the
 * tiles of one of them lie 8 workgroups apart.  lds_bytes: the LDS a workgroup asks for at this window (64 bytes per
 * column, the planes padded to 4 columns, plus the waves' sums).  Any pointer may be NULL.  Returns GCWT_OK or an error
 * code < 0 (a window above GCWT_COUPLING_SURROGATES_MAX_WINDOW and a grid of more than 2^31 - 1 workgroups among them). */
enum { GCWT_COUPLING_SURROGATES_TILE_PHASE = 4, GCWT_COUPLING_SURROGATES_TILE_AMP = 8, GCWT_COUPLING_SURROGATES_WAVES = 8 };
int gcwt_debug_coupling_surrogates_grid(int32_t n_channels, int64_t n_cols, int32_t n_phase, int32_t n_amp, int64_t window,
                                        int32_t* n_phase_tiles, int32_t* n_amp_tiles, int64_t* n_blocks, int64_t* lds_bytes);

/* Host only: the grid gcwt_triggered launches for n_rows rows and before + after + 1 lags.  The rows form tiles of
 * GCWT_TRIGGERED_TILE_ROWS, counted from the first row asked for, and the lags tiles of GCWT_TRIGGERED_TILE_LAGS,
 * counted from lag 0 (the last tile of either may be ragged); a workgroup takes one (channel, lag tile, row tile) and
 * every event.  n_blocks counts the workgroups: every row tile of every (channel, lag tile), the (channel, lag tile)s
 * padded to a multiple of 8 so that the row tiles of one of them lie 8 workgroups apart.  Any pointer may be NULL.
 * Returns GCWT_OK or an error code < 0 (a grid of more than 2^31 - 1 workgroups among them). */
enum { GCWT_TRIGGERED_TILE_ROWS = 4, GCWT_TRIGGERED_TILE_LAGS = 64 };
int gcwt_debug_triggered_grid(int32_t n_channels, int32_t n_rows, int64_t before, int64_t after, int32_t* n_row_tiles,
                              int64_t* n_lag_tiles, int64_t* n_blocks);

/* Host only: the grid gcwt_bandpass launches for n_cols columns and n_bands bands.  The columns form tiles of
 * GCWT_BANDPASS_TILE_COLS, counted from column 0, and the bands groups of GCWT_BANDPASS_GROUP_BANDS consecutive entries
 * of the list (the last tile and the last group may be ragged); a workgroup takes one (channel, column tile, band
 * group) and every row the group's bands hold.  n_blocks counts the workgroups: every band group of every (channel,
 * column tile), the (channel, column tile)s padded to a multiple of 8 so that the band groups of one of them lie 8
 * workgroups apart.  Any pointer may be NULL.  Returns GCWT_OK or an error code < 0 (a grid of more than 2^31 - 1
 * workgroups among them). */
enum { GCWT_BANDPASS_TILE_COLS = 512, GCWT_BANDPASS_GROUP_BANDS = 4 };
int gcwt_debug_bandpass_grid(int32_t n_channels, int64_t n_cols, int32_t n_bands, int64_t* n_col_tiles,
                             int32_t* n_band_groups, int64_t* n_blocks);

/* The column tile of gcwt_trace_stats and gcwt_trace_runs: GCWT_RUNS_TILE_COLS columns counted from column 0 (the
 * last tile of a trace may be ragged); a workgroup takes one (trace, tile).  Nothing returned depends on it for the
 * runs; for the statistics it is part of the prescribed order of the sums. */
enum { GCWT_RUNS_TILE_COLS = 1024 };

/* The chunk of gcwt_trace_order: a workgroup counts GCWT_ORDER_CHUNK_COLS columns of one trace, counted from column 0
 * (the last chunk of a trace may be ragged), in tiles of GCWT_RUNS_TILE_COLS.  Nothing returned depends on it. */
enum { GCWT_ORDER_CHUNK_COLS = 8192 };

/* The column tile of gcwt_trace_smooth: GCWT_SMOOTH_TILE_COLS columns counted from column 0 (the last tile of a trace
 * may be ragged); a workgroup takes one (output trace, tile) and stages it with its halo.  Nothing returned depends on
 * it. */
enum { GCWT_SMOOTH_TILE_COLS = 1024 };

#ifdef __cplusplus
}
#endif
#endif
