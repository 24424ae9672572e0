// plan_state.h -- what a plan holds (private to the library: the C ABI sees an opaque gcwt_plan) and the small helpers
// every file that works on one shares: error returns, events, device allocation.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ghostcwt.h"
#include "host_out.h"
#include "kernels.h"
#include "planner.h"

namespace gcwt {

// the thread's last error (gcwt_last_error): api.cpp
int set_err(int code, const std::string& msg);
int hip_err(hipError_t e, const char* what);

#define HIP_TRY(call)                                        \
  do {                                                       \
    hipError_t e_ = (call);                                  \
    if (e_ != hipSuccess) return gcwt::hip_err(e_, #call);   \
  } while (0)

struct EpochDev {
  SynthItemDev* items = nullptr;     // 16-column kernel: levels the production kernel does not take
  int n_items = 0;
  SynthLevelDev* levels = nullptr;
  Synth7Item* items7 = nullptr;      // production kernel
  Synth7Level* levels7 = nullptr;
  int n_items7 = 0;
  Synth7Item* items7w = nullptr;     // ... its wide-halo instantiation (shifted-band levels with halo > 48)
  int n_items7w = 0;
  Synth7Item* items7n = nullptr;     // ... its 16-column instantiation (R = 2: gcwt_plan::synth7_narrow_r)
  int n_items7n = 0;
  SynthiItem* items_i = nullptr;     // interpolating kernel (synthi.hip)
  SynthiLevel* levels_i = nullptr;
  int n_items_i = 0;
  int split_i = 0;                   // items_i[0 .. split_i): the levels below gcwt_plan::interp_split_r, launched first (pipeline.cpp: interp_launches)
  SynthpItem* items_p[2] = {nullptr, nullptr};   // pipelined interpolating kernel (synthp.hip); [1]: levels with I = 4
  SynthpLevel* levels_p = nullptr;
  int n_items_p[2] = {0, 0};
  PredLevel* pred_levels = nullptr;              // precision = auto / high: what each level's x_R holds (detect.hip)
};

enum Stage { ST_MEAN = 0, ST_FWD, ST_DECIM, ST_BLOCK, ST_SYNTH, ST_DIRECT, ST_FULLBAND, ST_INTERP, ST_BLOCKCONV, ST_COUNT };

}  // namespace gcwt

struct gcwt_plan {
  gcwt::HostPlan hp;
  bool uploaded = false;
  int profiling = 0;          // gcwt_plan_set_profiling: 0 off, 1 every stage between events, 2 the synthesis kernels only
  int synth_cols = 32;        // columns per workgroup of k_synth7 (GHOSTCWT_SYNTH_COLS=16|32)
  int synth7_narrow_r = 2;    // option synth7_narrow_r: levels of decimation <= this take the 16-column instantiation whatever
                              // synth_cols says (0: none).  R = 2 has seven scales on the headline grid, so a workgroup's prologue
                              // (its blocks' samples, their transforms) is a quarter of its life; 256-thread workgroups are three
                              // to a CU instead of two and hide it better: 1.17 against 1.26 ms for the level, while R = 4 and 8
                              // (fifteen scales) lose 8 % that way (profiles/r06_bound.md 5)
  bool fuse_blocks = true;    // k_synth7 makes its own block spectra from x_R (GHOSTCWT_FUSE_BLOCKS=0: separate pass)
  int synth_kernel = 7;       // 7: k_synth7; 8 (measure build only): producer/consumer waves (synth8.hip,
                              // measured slower: DESIGN.md 5) -- GHOSTCWT_SYNTH_KERNEL
  // Every GHOSTCWT_* knob is read ONCE, when the plan is created; an execute never looks at the
  // environment.
  bool prune_inputs = true;   // first-pass inputs above a scale's band skipped (kernels.hip: k_scale_windows);
                              // GHOSTCWT_PRUNE_INPUTS=0 computes them all (A/B runs)
  bool fast_fft = true;       // GHOSTCWT_SLOW_FFT=1: the generic radix-2 passes (A/B runs, tests)
  int drop_stores = 0;        // measure build only: GHOSTCWT_SYNTH_DROP_STORES (kernels.h)
  bool clock_probe = false;   // measure build only: GHOSTCWT_CLOCK_PROBE
  bool use_synth16 = false;   // GHOSTCWT_SYNTH16=1: 16-column kernel for every output mode (A/B tests)
  int device = -1;
  hipStream_t stream = nullptr;
  hipStream_t aux[2] = {nullptr, nullptr};   // the level passes of a batch run beside each other (pipeline.cpp: level_passes)
  bool level_streams = true;  // GHOSTCWT_LEVEL_STREAMS=0: everything on `stream`
  bool use_synthp = false;    // option synthp = 1: q = 2 levels with I <= 256 go to the pipelined kernel (synthp.hip); it
                              // ties with k_synthi on the headline and loses at R = 8 (profiles/r05_synth_study.md): off
  bool use_graphs = true;     // option graphs: small device-resident executes are replayed as a HIP graph
  bool fullband4 = true;      // option fullband4 = 0: 16 384-point segments by the two-pass kernels (A/B, tests)
  int fullband_group = 0;     // option fullband_group: rows per group of the fused full-band row pass (0: the kernel's default)
  int64_t fullband_cache_cap = 0;   // bytes of full-band responses kept across executes (set at upload: option
                                    // fullband_cache_mb, else a quarter of the memory free then, at most 16 GiB)
  bool hfull_cache_full = false;    // a response could not be allocated: the cache stays as it is
  int synth7_order = 0;       // option synth7_order: order of the k_synth7 work items (A/B runs)
  int synthp_help = -1;       // option synthp_help: share (of 128) of a round's tasks the producer waves take (A/B runs; default: by level)
  int synthp_lgnb = -1;       // option synthp_lgnb: blocks per k_synthp workgroup forced (A/B runs)
  int interp_lgnb = -1;       // option interp_lgnb: blocks per k_synthi workgroup forced (A/B runs)
  int interp_grid = -1;       // GHOSTCWT_INTERP_GRID=0|1: k_synthi's grid order forced (default: by the number of channel slots)
  bool last_fold = false;     // the last run took the channel sums inside the forward column pass
  bool fold_mean = true;      // option fold_mean = 0: the channel sums by a pass of their own over x even where the forward column pass could take them (run_pipeline)
  bool synth_streams = false; // GHOSTCWT_SYNTH_STREAMS=1: the interpolating kernel runs beside k_synth7 on aux[0] (its store-bound
                              // workgroups share the CUs with the arithmetic-bound ones: measured equal on the headline,
                              // profiles/r03_synth_study.md); default: one after the other, so that per-kernel times add up
  int interp_split_r = 64;    // option interp_split_r: k_synthi's items of the levels below this decimation are a launch of their
                              // own, made first: the cycle-bound levels (R = 16, 32: profiles/r06_bound.md 3) apart from the
                              // store-bound ones.  In one launch workgroups of both kinds share the CUs and k_synthi takes
                              // 0.23 ms of 6.4 longer (profiles/early_interp.md); 0: one launch
  bool early_interp = false;  // option early_interp = 1: the level passes k_synthi reads run on the plan's stream with k_synthi right
                              // behind them, the others on aux[] beside it, joined in front of the first kernel that reads them
                              // (pipeline.cpp: run_batch).  Measured: the passes leave the critical path and k_synthi grows by as much; off
  hipStream_t cur = nullptr;  // the stream the stage in hand is launched on (profiling spans follow it)
  // workspace
  bool high_precision = true; // gcwt_params.precision: float64 forward transform (fwd64.hip) + per-level low cut
  double2* d_y = nullptr;     // [slots][rows][4096] float64 intermediate of the forward transform
  int64_t y_stride = 0;
  double2* d_tw64 = nullptr;  // float64 twiddle tables (fwd64_fill_tables)
  float2* d_x = nullptr;      // [C][max_p]   spectrum (k1-major)
  float2* d_xr = nullptr;     // [C][max_xr]  decimated analytic signals, all levels
  float2* d_xb = nullptr;     // [C][max_xb]  block spectra, all levels
  float2* d_bank = nullptr;   // [S][B]
  float* d_gain = nullptr;    // [S][B] |H|
  float* d_gain_lv = nullptr; // the same rows in level-list order, transposed for k_synth7 (+8 zero rows)
  float2* d_half_tw = nullptr; // [levels][256] exp(-i pi k/(256 R))
  float2* d_psi = nullptr;    // direct kernels: running sums of the taps (kernels.hip: k_build_direct)
  float2* d_psi_tail = nullptr; // [n_direct] sum of all taps of each
  float2* d_psi_lit = nullptr;  // the literal taps, d_psi's layout (gcwt_direct_kernel)
  unsigned long long* d_probe = nullptr;   // GHOSTCWT_CLOCK_PROBE=1: [cycles, 100 MHz ticks] of the synthesis workgroups
  double* d_amps = nullptr;   // kept spectrum samples A_j of every scale (planner.h: amps)
  float2* d_xs = nullptr;     // [C][xs_stride] shifted slice of the spectrum of the level in hand (levels with a
  int64_t xs_stride = 0;      //   band shift: heavy-tailed wavelets); xs_stride = the largest such level's M
  float2* d_z = nullptr;      // [z_sets][slots][max_p]  full-band scales, up to four at a time: row-transformed spectrum * response
  int64_t z_half = 0;         //              elements between two of the set
  int z_sets = 1;
  float2* d_hfull = nullptr;  // [z_sets][max_p]  full-band responses of the scales in hand (when the cache below is full)
  // Full-band responses are an O(n_bins P) fp64 evaluation each: computed once per (scale, FFT
  // length) and kept on the device while they fit 16 GiB, reused by every later batch and execute.
  std::map<std::pair<int, int>, float2*> hfull_cache;
  int64_t hfull_cache_bytes = 0;
  float2* d_tw4096 = nullptr; // exp(-2 pi i j/4096), j < 2048
  float2* d_tw256 = nullptr;  // exp(+2 pi i q/256)
  float2* d_level_tw = nullptr;
  double* d_sums = nullptr;   // [C] sums (+ the partial sums and counters of k_channel_sum)
  int32_t* d_scale_list = nullptr;
  int n_listed = 0;           // entries of d_scale_list (all levels)
  int32_t* d_scale_aux = nullptr;   // per list entry: demodulation bin | (even kernel length) << 16 (synthi.hip)
  float* d_interp_coef = nullptr;   // interpolator coefficients of the interpolated levels
  gcwt::BankScale* d_bank_sc = nullptr;
  gcwt::DirectScale* d_direct_sc = nullptr;
  float2* d_bc_h = nullptr;       // [n_blockconv][4096]  block convolution: responses, in HostPlan::bc_order
  int32_t* d_bc_rows = nullptr;   // [n_blockconv]        their output rows
  float2* d_bc_x = nullptr;       // [bc_chunk_blocks][C][4096]  spectra of the blocks in hand
  float2* d_bc_tw = nullptr;      // [4096]               the middle twiddles in k_bc_scales' order
  std::vector<gcwt::EpochDev> ep_dev;
  int64_t max_direct_len = 0;
  // staging for host-side callers
  float* d_in = nullptr;
  size_t d_in_bytes = 0;
  void* d_out = nullptr;
  size_t d_out_bytes = 0;
  gcwt::HostOut host_out;    // pinned staging ring for host results
  // profiling
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  struct Span { int stage; hipEvent_t a, b; };
  std::vector<Span> spans;
  gcwt_timings last{};
  bool have_timings = false;
  bool have_means = false;
  // precision = auto / high: the detector (detect.hip).  d_hist: band energies of the spectrum per slot, filled by the
  // forward row pass; d_pred: per scale, the largest predicted loss over the slots of an execute.
  bool detect = false;               // the plan predicts (float64 forward transform, no long mode, some spectral scale)
  float* d_hist = nullptr;
  float* d_bands = nullptr;          // [slots][kSpecBands]: the rows of d_hist added up (detect.hip: k_band_sums)
  float* d_pred = nullptr;
  hipStream_t det_stream = nullptr;  // the predictions are made beside the level passes and the synthesis, not behind them
  int32_t* d_scale_level = nullptr;
  int32_t* d_scale_length = nullptr;   // the reference kernel's L per scale (capped at 2^30)
  std::vector<float> last_pred;      // the last execute's predictions (host)
  float* h_pred = nullptr;           // ... as they arrive: page-locked, so that the 4 S bytes do not go through a staging copy
  float last_worst = 0.f;
  int last_rerouted = 0;
  float auto_threshold = 1.5e-6f;    // option auto_threshold_ppb.  The prediction is an r.m.s. figure calibrated on noise-like rows
                                     // (1.6e-7 D); a row that is nearly a sinusoid (narrow wavelets, gamma = 6) has a crest
                                     // factor three times smaller, so its gate metric reads three times the prediction: the
                                     // threshold leaves a factor 6.7 to the 1e-5 gate (benign recordings predict 2 - 4e-7)
  float kappa_eps = 1.6e-7f;         // predicted loss = kappa_eps sqrt(E_level W_s / E_s); option auto_kappa_ppb
  float oob_tol = 2.5e-8f;            // ... or oob_tol sqrt(E_out / E_s), what the level leaves out; option auto_oob_ppt (1e-12)
  int last_batch_slots = 0;          // slots of the last batch that ran (gcwt_debug_precision_terms)
  int last_batch = 0, last_rows = 0;
  double last_pt = 0;
  // scales made again by the exact paths: a sub-plan with precision = exact over ALL the scales, for every channel [0] or
  // for one [1], made on first need; a run of it is masked to the scales wanted and writes straight into this plan's rows
  gcwt_plan* sub_plan[2] = {nullptr, nullptr};
  bool is_sub_plan = false;          // this plan IS such a sub-plan (its response cache takes half the share)
  // a masked run (this plan IS such a sub-plan): run_mask[scale] != 0 -> make the row; nothing else is touched
  const unsigned char* run_mask = nullptr;
  unsigned char* d_run_mask = nullptr;
  // Small device-resident executes are launch-bound (config 1: fifteen kernels of a few microseconds each): the
  // second execute with the same arguments is captured into a graph, later ones replay it
  struct GraphKey {
    const void* x = nullptr; const void* out = nullptr;
    int64_t r0 = 0, r1 = 0, row_len = 0; bool reuse = false;
    bool operator==(const GraphKey& o) const {
      return x == o.x && out == o.out && r0 == o.r0 && r1 == o.r1 && row_len == o.row_len && reuse == o.reuse;
    }
  };
  GraphKey graph_key, graph_seen;
  hipGraphExec_t graph_exec = nullptr;
  bool graph_seen_valid = false, graph_failed = false;
  int64_t row_pitch = 0;     // device output rows, samples; 0 = dense
  int64_t out_stride = 1;    // K: output column j holds recording sample K j (gcwt_plan_set_output_stride)
};

namespace gcwt {

// output columns of the samples [a, b) of the recording: the multiples of K among them
inline int64_t stride_cols(int64_t a, int64_t b, int64_t k) { return b <= a ? 0 : (b + k - 1) / k - (a + k - 1) / k; }

template <typename T>
int dev_alloc(T** p, size_t count) {
  if (count == 0) count = 1;
  HIP_TRY(hipMalloc((void**)p, count * sizeof(T)));
  return GCWT_OK;
}

template <typename T>
int upload_vec(T** p, const std::vector<T>& v, hipStream_t st) {
  int rc = dev_alloc(p, v.size());
  if (rc) return rc;
  if (!v.empty()) HIP_TRY(hipMemcpyAsync(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
  return GCWT_OK;
}

inline int get_event(gcwt_plan* p, hipEvent_t* e) {
  if (p->ev_used == p->ev_pool.size()) {
    hipEvent_t n;
    HIP_TRY(hipEventCreate(&n));
    p->ev_pool.push_back(n);
  }
  *e = p->ev_pool[p->ev_used++];
  return GCWT_OK;
}

// RAII-less span helper: begin/end record events on the stage's stream when profiling
struct SpanGuard {
  gcwt_plan* p;
  int stage;
  hipEvent_t a = nullptr;
  int rc = GCWT_OK;
  bool on = false;
  SpanGuard(gcwt_plan* p_, int st) : p(p_), stage(st) {
    // (level 2: the events around the other stages cost the step they measure 0.19 ms of 13.5 -- tools/step_gap.py)
    on = p->profiling == 1 || (p->profiling == 2 && (st == ST_SYNTH || st == ST_INTERP));
    if (!on) return;
    rc = get_event(p, &a);
    if (rc == GCWT_OK && hipEventRecord(a, p->cur ? p->cur : p->stream) != hipSuccess) rc = GCWT_ERR_HIP;
  }
  int end() {
    if (!on || rc) return rc;
    hipEvent_t b;
    rc = get_event(p, &b);
    if (rc) return rc;
    if (hipEventRecord(b, p->cur ? p->cur : p->stream) != hipSuccess) return GCWT_ERR_HIP;
    p->spans.push_back({stage, a, b});
    return GCWT_OK;
  }
};

// Computes samples [r0, r1) of every (channel, scale) row into rows of row_len samples
// (column = sample - r0).  The full transform is r0 = 0, r1 = N, row_len = N.  (pipeline.cpp)
int run_pipeline(gcwt_plan* p, const float* dx, float* dout, int64_t r0, int64_t r1, int64_t row_len, bool reuse_means);

}  // namespace gcwt

// the tables derived from the bank, made again after a (broadcast) bank has arrived (api.cpp; comm.cpp calls it)
int gcwt_internal_refresh_bank(gcwt_plan* p);
