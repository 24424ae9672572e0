// pipeline.cpp -- the launches of one transform: run_pipeline (plan_state.h) as a list of stages.
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "interp.h"
#include "kernels.h"
#include "plan_state.h"
#include "work_items.h"

namespace gcwt {
namespace {

// what is fixed for one call of run_pipeline
struct Call {
  gcwt_plan* p;
  const float* dx;
  float* dout;
  int64_t r0, r1, row_len;
  int mode, elem;
  double inv_n;
  OutStride os;                   // output stride K: sample n of the recording is column n / K - ceil(r0 / K) of a row, kept when K divides it
  const unsigned char* hmask;     // a masked run (gcwt_plan::run_mask) and its copy on the device
  const unsigned char* dmask;
  bool fold;                      // the channel sums are taken inside the forward column pass
};

// what is fixed for one batch: segments that share the FFT length and the level grids; those with something to write
// in [r0, r1) become extra sets of "channels"
struct Batch {
  const EpochPlan* ep;
  const EpochDev* dev;
  SegIn sin{};
  SegOut sout{};
  PredSegs psegs{};
  int nb = 0, slots = 0;
  // P, P1: the STORED spectrum (rows of 4096 bins); Pt: the segment's true FFT length.  They differ in long mode
  // only (planner.h, EpochPlan::long_a: Pt = A P, the spectrum's low half combined from A interleaved transforms)
  int64_t P = 0, Pt = 0;
  int P1 = 0, A = 1;
  // The input is real, so rows k1 and P1 - k1 of the k1-major spectrum mirror each other:
  // the fast path builds rows 0 .. P1/2 only and writes the rest as their reflections.
  // Full-band scales read every bin, so a plan that has any builds the whole spectrum.
  bool hermitian = false;
  int rows_a = 0;
  float xb_scale = 0.f;           // 1 / (block Pt): what the block spectra carry
  // what the stages leave for the ones behind them
  bool early = false;             // option early_interp is in force for this batch (level_passes)
  bool forked[2] = {false, false};   // aux[k] runs level passes the plan's stream has not waited for yet
  hipStream_t si = nullptr;       // the stream of the interpolating kernels (interp_launches)
};

#define RUN(stage_id, call)                                 \
  do {                                                      \
    SpanGuard sg_(p, stage_id);                             \
    if (sg_.rc) return sg_.rc;                              \
    const hipError_t he_ = (call);                          \
    if (he_ != hipSuccess) return hip_err(he_, #call);      \
    int rc_ = sg_.end();                                    \
    if (rc_) return rc_;                                    \
  } while (0)

// an event that stands for what `on` has been given so far
int mark(gcwt_plan* p, hipStream_t on, hipEvent_t* ev, const char* what) {
  int rc = get_event(p, ev);
  if (rc) return rc;
  const hipError_t he = hipEventRecord(*ev, on);
  return he == hipSuccess ? GCWT_OK : hip_err(he, what);
}

// `waiter` waits for what `on` has been given so far
int wait_for(gcwt_plan* p, hipStream_t waiter, hipStream_t on, const char* what) {
  hipEvent_t ev;
  int rc = mark(p, on, &ev, what);
  if (rc) return rc;
  const hipError_t he = hipStreamWaitEvent(waiter, ev, 0);
  return he == hipSuccess ? GCWT_OK : hip_err(he, what);
}

// does the run make a scale of a method `is` names?  (a masked run: a marked one)
template <typename Is>
bool any_scale(const Call& c, Is is) {
  const HostPlan& hp = c.p->hp;
  for (int i = 0; i < hp.prm.n_freqs; ++i)
    if ((!c.hmask || c.hmask[i]) && is(hp.scales[i].method)) return true;
  return false;
}

// the plan's epochs, in the caller's order, cut to [r0, r1): fn(start, stop, g_lo, g_hi) for each that keeps a sample;
// a failure ends the walk
template <typename Fn>
int for_clipped_epochs(const Call& c, Fn fn) {
  const std::vector<int64_t>& b = c.p->hp.bounds;
  for (size_t i = 0; i + 1 < b.size(); i += 2) {
    const int64_t g_lo = std::max(b[i], c.r0), g_hi = std::min(b[i + 1], c.r1);
    if (g_hi <= g_lo) continue;
    const int rc = fn(b[i], b[i + 1], g_lo, g_hi);
    if (rc) return rc;
  }
  return GCWT_OK;
}

// samples outside every epoch are zero (transforms.py:185): one launch per gap, or one
// fill of the whole result when there are many of them (a masked run writes into rows that are finished but for
// the marked scales: their gaps are zero already)
int zero_gaps(const Call& c) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  const int64_t C = hp.prm.n_channels, S = hp.prm.n_freqs, N = hp.prm.n_samples, K = c.os.k;
  if (c.hmask) return GCWT_OK;
  std::vector<std::pair<int64_t, int64_t>> eps, gaps;
  for (size_t i = 0; i + 1 < hp.bounds.size(); i += 2) eps.push_back({hp.bounds[i], hp.bounds[i + 1]});
  std::sort(eps.begin(), eps.end());
  int64_t cursor = c.r0;
  for (size_t i = 0; i <= eps.size(); ++i) {
    const int64_t gap_end = std::min(c.r1, i < eps.size() ? eps[i].first : N);
    if (gap_end > cursor) gaps.push_back({cursor, gap_end});
    if (i < eps.size()) cursor = std::max(cursor, std::min(c.r1, eps[i].second));
  }
  if (gaps.size() > 8) {
    const hipError_t he = hipMemsetAsync(c.dout, 0, sizeof(float) * (size_t)c.elem * (size_t)c.row_len * (size_t)C * (size_t)S, p->stream);
    if (he != hipSuccess) return hip_err(he, "zero fill");
    return GCWT_OK;
  }
  for (const auto& g : gaps) {     // (K > 1: the gap's columns, the multiples of K inside it)
    const hipError_t he = launch_zero_range(c.dout, c.row_len * c.elem, C * S, stride_cols(c.r0, g.first, K) * c.elem,
                                            stride_cols(g.first, g.second, K) * c.elem, p->stream);
    if (he != hipSuccess) return hip_err(he, "zero_range");
  }
  return GCWT_OK;
}

// the segments e0 .. e0 + count - 1 of a batch that have something to write in [r0, r1), and the batch's shapes
Batch gather_batch(const Call& c, size_t e0, size_t count) {
  const gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  const int C = hp.prm.n_channels;
  Batch b;
  b.ep = &hp.epochs[e0];
  b.dev = &p->ep_dev[b.ep->batch_first];
  for (size_t i = 0; i < count; ++i) {
    const EpochPlan& m = hp.epochs[e0 + i];
    // output window of the segment, segment-local: its core, cut to the range
    const int64_t w_lo = std::max(m.core0, c.r0) - m.start, w_hi = std::min(m.core1, c.r1) - m.start;
    if (w_hi <= w_lo) continue;
    b.psegs.seg[b.nb] = (int32_t)(e0 + i);
    b.sin.x_off[b.nb] = m.start;
    b.sin.n_valid[b.nb] = m.ne;
    b.sin.n_lead[b.nb] = m.lead;
    b.sin.ramp_lo[b.nb] = m.ramp_lo;
    b.sin.ramp_hi[b.nb] = m.ramp_hi;
    b.sout.seg_col[b.nb] = m.start - c.r0;
    b.sout.w_lo[b.nb] = w_lo;
    b.sout.w_hi[b.nb] = w_hi;
    ++b.nb;
  }
  b.sin.n_channels = b.sout.n_channels = b.psegs.n_channels = C;
  b.sout.os = c.os;
  b.slots = C * b.nb;
  b.P = b.ep->p_store;
  b.Pt = b.ep->p;
  b.P1 = b.ep->p1;
  b.A = b.ep->long_a;
  b.hermitian = p->fast_fft && b.P1 >= 4 && hp.n_fullband == 0;
  b.rows_a = b.hermitian ? b.P1 / 2 + 1 : b.P1;
  b.xb_scale = (float)(1.0 / ((double)hp.block * (double)b.Pt));
  b.si = p->stream;
  return b;
}

// precision = auto / high: the row pass left the band energies of every row of the spectrum (fwd64.hip:
// row_band_sums); on a stream of its own, beside the level passes and the synthesis, they are added up and turned
// into what the float32 stages will cost each scale (detect.hip); joined at the end of the batch
int detector_fork(const Call& c, const Batch& b) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  int rc = wait_for(p, p->det_stream, p->stream, "detector fork");
  if (rc) return rc;
  hipError_t he = launch_band_sums(p->d_hist, b.P1, p->d_bands, b.slots, p->det_stream);
  if (he != hipSuccess) return hip_err(he, "launch_band_sums");
  he = launch_precision_predict(p->d_bands, p->d_gain, p->d_scale_level, p->d_scale_length, b.dev->pred_levels, hp.prm.n_freqs,
                                (int)hp.levels.size(), (double)b.Pt, p->kappa_eps, p->oob_tol, p->d_pred, nullptr, nullptr, b.slots, b.psegs,
                                p->det_stream);
  if (he != hipSuccess) return hip_err(he, "launch_precision_predict");
  p->last_batch_slots = b.slots; p->last_batch = b.ep->batch_first; p->last_pt = (double)b.Pt; p->last_rows = b.P1;
  return GCWT_OK;
}

// forward FFT, pass A: FFT over n1 (stride 4096) of x[4096 n1 + n2], twiddle W_P^{-n2 k1}; pass B: rows over n2
int forward_transform(const Call& c, const Batch& b) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  const int64_t N = hp.prm.n_samples;
  hipStream_t st = p->stream;
  if (p->d_y) {
    // precision = high: both passes in float64, the spectrum rounded to float32 per bin (fwd64.hip)
    for (int a = 0; a < b.A; ++a) {
      RUN(ST_FWD, launch_fwd64_cols(c.dx, p->d_y, b.P1, N, p->y_stride, b.P, p->d_tw64, p->d_sums, c.inv_n, b.sin, b.nb,
                                    b.rows_a, st, b.A, a, c.fold));
      if (c.fold) RUN(ST_MEAN, launch_channel_sum_final(p->d_sums, hp.prm.n_channels, fold_parts(b.P1), st));
      RUN(ST_FWD, launch_fwd64_rows(p->d_y, p->d_x, b.rows_a, p->y_stride, b.P, p->d_tw64, b.slots,
                                    hp.n_fullband > 0 ? kRowLen : kRowLen / 2, b.hermitian ? b.P1 : 0, st, a, b.A, b.Pt,
                                    p->detect ? p->d_hist : nullptr, b.P1, c.fold ? p->d_sums : nullptr, c.inv_n, b.ep->ne, b.P1));
    }
    return p->detect ? detector_fork(c, b) : GCWT_OK;
  }
  if (b.A > 1) return set_err(GCWT_ERR_UNSUPPORTED, "internal: long mode without the float64 forward transform");
  RUN(ST_FWD, launch_fft_cols_batch(c.dx, p->d_x, b.P1, kRowLen, N, b.P, b.P1 > 1 ? b.P : 0, p->d_tw4096,
                                    p->fast_fft ? p->d_tw256 : nullptr, p->d_sums, c.inv_n, b.sin, b.nb, st,
                                    b.rows_a));
  // pass B: rows over n2 -> X~[k1][k2] = X[k1 + P1 k2]; only X[k < P/2] is ever read
  RUN(ST_FWD, launch_fft_rows(-1, p->d_x, p->d_x, kRowLen, b.rows_a, kRowLen, kRowLen, b.P, b.P, 0,
                              p->d_tw4096, p->fast_fft ? p->d_tw256 : nullptr, 1.0f, b.slots, st,
                              hp.n_fullband > 0 ? kRowLen : kRowLen / 2, b.hermitian ? b.P1 : 0));
  return GCWT_OK;
}

// the production synthesis kernel computes its blocks' spectra itself (no XB pass)
bool fused_blocks(const gcwt_plan* p) { return p->fuse_blocks && p->synth_kernel == 7 && !p->use_synth16; }

// Where the level passes of a batch run, and in which order they are launched.
struct LevelOrder {
  bool side = false;              // the passes are shared among the plan's stream and aux[]
  bool early = false;             // option early_interp in force
  std::vector<char> in_h;         // the level's x_R is read by an interpolated level (early: group H)
  std::vector<int> stream_of;     // 0: the plan's stream, k: aux[k - 1]
  std::vector<size_t> order;      // the levels in launch order
};

// The levels are independent once the spectrum is there (rows pass -> column pass per
// level, disjoint x_R); run one after the other they leave 10 us between launches and the
// small ones (R >= 16: grids that do not fill the chip) cost 0.2 ms.  Three streams, the
// plan's own being one of them, share them by estimated time -- two passes over the level's
// P/R samples per slot at the rate such passes reach, plus what two launches cost however
// small they are (config 5's levels are all of the second kind and end up three per stream;
// the headline's R = 2 level is half of all the work and keeps a stream to itself) -- and
// join before the synthesis.
LevelOrder level_order(const gcwt_plan* p, const Batch& b) {
  const HostPlan& hp = p->hp;
  const EpochPlan& ep = *b.ep;
  const EpochDev& dev = *b.dev;
  LevelOrder lo;
  lo.side = p->level_streams && hp.levels.size() > 2;
  // The interpolating kernel reads the x_R of its own levels only (R >= 16: an eighth of the level passes' traffic)
  // and the kernels behind it read the rest.  Option early_interp = 1: group H, the levels whose x_R an interpolated
  // level reads, on the plan's own stream with k_synthi right behind them; group L, the others, on aux[0] and aux[1]
  // beside both, joined in front of the first kernel that reads them.  Off by default: what the front end loses
  // k_synthi gains, and no step is shorter for it (profiles/early_interp.md).  Never with every stage between events
  // (profiling level 1: stages_ms stays what it was), with synth_streams (k_synthi on aux[0]) or without an
  // interpolated level.
  lo.in_h.assign(hp.levels.size(), 0);
  bool any_h = false;
  for (size_t l = 0; l < hp.levels.size(); ++l)
    if (level_kernel(p, hp.levels[l]) == LK_INTERP) {
      lo.in_h[hp.levels[l].xr_owner >= 0 ? (size_t)hp.levels[l].xr_owner : l] = 1;
      any_h = true;
    }
  for (size_t l = 0; l < hp.levels.size(); ++l)              // a level that shares an x_R follows its owner
    if (hp.levels[l].xr_owner >= 0) lo.in_h[l] = lo.in_h[(size_t)hp.levels[l].xr_owner];
  lo.early = lo.side && p->early_interp && p->profiling != 1 && !p->synth_streams && any_h &&
             dev.n_items_i + dev.n_items_p[0] + dev.n_items_p[1] > 0;
  lo.stream_of.assign(hp.levels.size(), 0);
  if (lo.side) {
    double load[3] = {0.0, 0.0, 0.0};
    std::vector<size_t> order;
    for (size_t l = 0; l < hp.levels.size(); ++l)
      if (hp.levels[l].xr_owner == (int)l && !(lo.early && lo.in_h[l])) order.push_back(l);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return ep.lv[x].m > ep.lv[y].m; });
    const int k0 = lo.early ? 1 : 0;        // (early: the plan's own stream is group H's)
    for (size_t l : order) {
      const int k = (int)(std::min_element(load + k0, load + 3) - load);
      lo.stream_of[l] = k;
      load[k] += 40e-6 + 32.0 * (double)ep.lv[l].m * (double)b.slots / 4.5e12;   // seconds
    }
    for (size_t l = 0; l < hp.levels.size(); ++l) lo.stream_of[l] = lo.stream_of[hp.levels[l].xr_owner];
  }
  // (early: group H's passes are launched first, in level order, then group L's)
  for (size_t li = 0; li < (lo.early ? 2 : 1) * hp.levels.size(); ++li) {
    const size_t l = li % hp.levels.size();
    if (lo.early && (lo.in_h[l] != 0) != (li < hp.levels.size())) continue;
    lo.order.push_back(l);
  }
  return lo;
}

// the passes that make one level's x_R from the spectrum (and its block spectra, for the kernels that read XB) on `ls`
int level_pass(const Call& c, const Batch& b, size_t l, int stream_index, hipStream_t ls) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  const LevelPlan& lp = hp.levels[l];
  const EpochLevel& el = b.ep->lv[l];
  const int P1 = b.P1, A = b.A, slots = b.slots;
  const int64_t P = b.P;
  const bool fast_fft = p->fast_fft;
  float2* xr = p->d_xr + el.xr_offset;
  RowTaper taper;                      // precision = high: the slice loses what lies below every scale's band
  if (p->high_precision && lp.taper_hi > 0.0 && lp.band_shift == 0) {
    const double k1 = lp.taper_hi * (double)b.Pt / (2.0 * M_PI), k0 = 0.5 * k1;
    if (k1 - k0 >= 1.0) { taper.p1 = P1; taper.k0 = (float)k0; taper.inv_width = (float)(1.0 / (k1 - k0)); }
  }
  if (lp.xr_owner != (int)l) {
    // x_R of this decimation was made for the level that owns it (an earlier one)
  } else if (lp.decimation / A <= kMaxTwoPassDecimation) {
    const int Q = kRowLen * A / lp.decimation;        // M = P1 Q samples: decimation R / A of the stored spectrum
    const float2* src = p->d_x;
    int64_t src_row = kRowLen, src_cstride = P;
    if (lp.band_shift > 0) {
      // the level's band starts band_shift bins below zero: its M spectrum samples are gathered
      // (negative frequencies as conjugates) into a slice buffer first, one per stream
      const int64_t U = (int64_t)lp.band_shift * el.m / hp.block;     // a multiple of P1 (planner: steps of R / 16 bins)
      if (U % P1 != 0 || U / P1 > Q) return set_err(GCWT_ERR_INVALID, "internal: band shift does not slice the spectrum");
      float2* xs = p->d_xs + (int64_t)stream_index * slots * p->xs_stride;
      RUN(ST_DECIM, launch_shift_gather(p->d_x, xs, P1, Q, (int)(U / P1), kRowLen, P, p->xs_stride, slots, ls));
      src = xs; src_row = Q; src_cstride = p->xs_stride;
    }
    // x_R[Q m1 + m2] = sum_{j1} e^{2 pi i j1 m1/P1} e^{2 pi i j1 m2/M} sum_{j2} X~[j1][j2] e^{2 pi i j2 m2/Q}
    RUN(ST_DECIM, launch_fft_rows(+1, src, xr, Q, P1, src_row, Q, src_cstride, hp.max_xr,
                                  P1 > 1 ? el.m : 0, p->d_tw4096,
                                  fast_fft ? p->d_tw256 : nullptr, 1.0f, slots, ls, 0, 0, taper));
    if (P1 > 1)
      RUN(ST_DECIM, launch_fft_cols(+1, false, xr, xr, P1, Q, hp.max_xr, hp.max_xr, 0,
                                    p->d_tw4096, fast_fft ? p->d_tw256 : nullptr, p->d_sums,
                                    c.inv_n, 0, slots, ls));
  } else {
    // M = P/R <= 8192: rows j1 < n1 of X~, q leading entries each
    const int n1 = (int)std::min<int64_t>(P1, el.m);
    const int q = (int)(el.m / n1);
    RUN(ST_DECIM, launch_level_small(p->d_x, xr, n1, q, kRowLen, P, hp.max_xr, p->d_tw4096, slots, ls, taper));
  }
  const LevelKernel lk = level_kernel(p, lp);
  if (lk == LK_SYNTH16 || (lk == LK_SYNTH7 && !fused_blocks(p)))     // the kernels that read XB
    RUN(ST_BLOCK, launch_block_fft(xr, p->d_xb + el.xb_offset, el.m, lp.hop, lp.halo, el.blk_lo,
                                   el.nblk, hp.max_xr, hp.max_xb, p->d_tw256, b.xb_scale, slots, ls));
  return GCWT_OK;
}

// every level's passes, each on its stream; aux[k] waits for the spectrum in front of its first pass
int level_passes(const Call& c, Batch* b) {
  gcwt_plan* p = c.p;
  hipStream_t st = p->stream;
  const LevelOrder lo = level_order(p, *b);
  b->early = lo.early;
  hipEvent_t spectrum_ready = nullptr;
  if (lo.side) {
    int rc = mark(p, st, &spectrum_ready, "hipEventRecord");
    if (rc) return rc;
  }
  for (size_t l : lo.order) {
    hipStream_t ls = st;
    if (lo.side) {                          // level (and whoever shares its x_R) -> its own stream
      const int k = lo.stream_of[l];
      ls = k == 0 ? st : p->aux[k - 1];
      if (k > 0 && !b->forked[k - 1]) {
        const hipError_t he = hipStreamWaitEvent(ls, spectrum_ready, 0);
        if (he != hipSuccess) return hip_err(he, "hipStreamWaitEvent");
        b->forked[k - 1] = true;
      }
      p->cur = ls;
    }
    int rc = level_pass(c, *b, l, lo.stream_of[l], ls);
    if (rc) return rc;
  }
  if (lo.side) p->cur = nullptr;
  return GCWT_OK;
}

// the plan's stream waits for the level passes on aux[]: before the synthesis, or (early) behind k_synthi's launches
int join_levels(const Call& c, Batch* b) {
  for (int k = 0; k < 2; ++k) {
    if (!b->forked[k]) continue;
    b->forked[k] = false;
    int rc = wait_for(c.p, c.p->stream, c.p->aux[k], "level streams join");
    if (rc) return rc;
  }
  return GCWT_OK;
}

// Which index runs fastest in the grid decides what is in flight together: the same few items
// of every channel, or many items of one channel.  Measured (profiles/r03_synth_study.md 12): with
// 24 channel slots (config 5) channels-fastest is 3 % faster; with 128 it is as fast in most
// processes and 8 % slower in some (the placement of the 51 GB of rows decides), items-fastest
// never is.
int channels_fastest(const gcwt_plan* p, int slots, int n_items) {
  if (n_items > 65535) return 0;       // (grid.y is 16 bits wide)
  return p->interp_grid >= 0 ? p->interp_grid : (slots <= 32 ? 1 : 0);
}

// The interpolating kernel is launched first; with GHOSTCWT_SYNTH_STREAMS=1 on a stream of its own, k_synth7 beside it:
// the two share the CUs (store-bound workgroups next to arithmetic-bound ones) and each
// fills the other's tail.  Both only read what the level passes left and write disjoint rows.
int interp_launches(const Call& c, Batch* b) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  const EpochDev& dev = *b->dev;
  if (dev.n_items_i == 0) return GCWT_OK;
  const bool beside = p->synth_streams && (dev.n_items7 > 0 || dev.n_items7w > 0 || dev.n_items7n > 0 || dev.n_items > 0);
  if (beside) {
    int rc = wait_for(p, p->aux[0], p->stream, "synthesis fork");
    if (rc) return rc;
    b->si = p->aux[0];
  }
  hipStream_t si = b->si;
  SynthiArgs ai{};
  ai.tw256 = p->d_tw256;
  ai.level_tw = p->d_level_tw;
  ai.levels = dev.levels_i;
  ai.scale_list = p->d_scale_list;
  ai.scale_aux = p->d_scale_aux;
  ai.gain = p->d_gain;
  ai.coef = p->d_interp_coef;
  ai.out = c.dout;
  ai.row_len = c.row_len;
  ai.xr = p->d_xr;
  ai.xr_cstride = hp.max_xr;
  ai.xb_scale = b->xb_scale;
  ai.n_scales = hp.prm.n_freqs;
  ai.channels_fastest = channels_fastest(p, b->slots, dev.n_items_i);
  ai.seg = b->sout;
  p->cur = si;
  // two launches, one behind the other: the levels below interp_split_r, then the rest (work_items.cpp: one
  // list in two parts)
  for (int part = 0; part < 2; ++part) {
    const int first = part == 0 ? 0 : dev.split_i, n_part = part == 0 ? dev.split_i : dev.n_items_i - dev.split_i;
    if (n_part == 0) continue;
    ai.items = dev.items_i + first;
    if (c.os.k > 1) RUN(ST_INTERP, launch_synthis(c.mode, ai, n_part, b->slots, si));
    else RUN(ST_INTERP, launch_synthi(c.mode, ai, n_part, b->slots, si));
  }
  p->cur = nullptr;
  return GCWT_OK;
}

// the pipelined interpolating kernel (the measure build's), behind k_synthi on its stream
int pipelined_launches(const Call& c, const Batch& b) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  const EpochDev& dev = *b.dev;
  for (int k = 0; k < 2; ++k) {
    if (dev.n_items_p[k] == 0) continue;
    SynthpArgs ap{};
    ap.tw256 = p->d_tw256;
    ap.level_tw = p->d_level_tw;
    ap.items = dev.items_p[k];
    ap.levels = dev.levels_p;
    ap.scale_list = p->d_scale_list;
    ap.scale_aux = p->d_scale_aux;
    ap.gain_lv = p->d_gain_lv;
    ap.level_half_tw = p->d_half_tw;
    ap.coef = p->d_interp_coef;
    ap.out = c.dout;
    ap.row_len = c.row_len;
    ap.xr = p->d_xr;
    ap.xr_cstride = hp.max_xr;
    ap.xb_scale = b.xb_scale;
    ap.n_scales = hp.prm.n_freqs;
    ap.channels_fastest = channels_fastest(p, b.slots, dev.n_items_p[k]);
    ap.flags = 0;
    ap.seg = b.sout;
    p->cur = b.si;
#ifdef GCWT_MEASURE
    if (c.os.k > 1) return set_err(GCWT_ERR_UNSUPPORTED, "output stride with the pipelined interpolating kernel");
    RUN(ST_INTERP, launch_synthp(c.mode, ap, dev.n_items_p[k], b.slots, k == 1, b.si));
#else
    (void)ap;
    return set_err(GCWT_ERR_INVALID, "internal: a level planned for the measure build's pipelined kernel");
#endif
    p->cur = nullptr;
  }
  return GCWT_OK;
}

// the 16-column kernel: the levels the production kernel does not take
int synth16_launch(const Call& c, const Batch& b) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  const EpochDev& dev = *b.dev;
  if (dev.n_items == 0) return GCWT_OK;
  SynthArgs a{};
  a.xb = p->d_xb;
  a.bank = p->d_bank;
  a.tw256 = p->d_tw256;
  a.level_tw = p->d_level_tw;
  a.items = dev.items;
  a.levels = dev.levels;
  a.out = c.dout;
  a.xb_cstride = hp.max_xb;
  a.row_len = c.row_len;
  a.n_scales = hp.prm.n_freqs;
  a.seg = b.sout;
  RUN(ST_SYNTH, launch_synth(c.mode, a, dev.n_items, b.slots, p->stream));
  return GCWT_OK;
}

// k_synth7: 16 columns (R = 2) first, then the 32-column lists
int synth7_launches(const Call& c, const Batch& b) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  const EpochDev& dev = *b.dev;
  hipStream_t st = p->stream;
  for (int variant = 0; variant < 3; ++variant) {
    const int wide = variant == 2;
    const int cols7 = variant == 0 ? 16 : p->synth_cols;
    const int n7 = variant == 0 ? dev.n_items7n : wide ? dev.n_items7w : dev.n_items7;
    if (n7 == 0) continue;
    Synth7Args a7{};
    a7.xb = p->d_xb;
    a7.bank = p->d_bank;
    a7.tw256 = p->d_tw256;
    a7.level_tw = p->d_level_tw;
    a7.items = variant == 0 ? dev.items7n : wide ? dev.items7w : dev.items7;
    a7.levels = dev.levels7;
    a7.scale_list = p->d_scale_list;
    a7.gain = p->d_gain;
    a7.gain_lv = p->d_gain_lv;
    a7.level_half_tw = p->d_half_tw;
    a7.complex_gains = hp.morlet ? 1 : 0;
    a7.out = c.dout;
    a7.xb_cstride = hp.max_xb;
    a7.row_len = c.row_len;
    a7.n_scales = hp.prm.n_freqs;
    a7.drop_stores = p->drop_stores;
    a7.seg = b.sout;
    a7.clock_probe = p->d_probe;
    if (fused_blocks(p)) {
      a7.xr = p->d_xr;
      a7.xr_cstride = hp.max_xr;
      a7.xb_scale = b.xb_scale;
    }
    if (c.os.k > 1) {                    // every halo width: the strided kernel tests each row's place in the block
      RUN(ST_SYNTH, launch_synth7s(c.mode, cols7, a7, n7, b.slots, st));
      continue;
    }
#ifdef GCWT_MEASURE
    if (p->synth_kernel == 8 && variant == 1)
      RUN(ST_SYNTH, launch_synth8(c.mode, p->synth_cols, a7, n7, b.slots, st));
    else
#endif
      RUN(ST_SYNTH, launch_synth7(c.mode, cols7, wide != 0, a7, n7, b.slots, st));
  }
  return GCWT_OK;
}

// the response of full-band scale i on the batch's FFT grid: from the cache, or computed into the cache while it has
// room, else into scratch row `scratch` of d_hfull
int fullband_response(const Call& c, const Batch& b, int i, int scratch, const float2** h_out) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  const auto cached = p->hfull_cache.find({i, b.P1});
  if (cached != p->hfull_cache.end()) { *h_out = cached->second; return GCWT_OK; }
  float2* dst = p->d_hfull + (int64_t)scratch * hp.max_p;
  float2* keep = nullptr;
  const int64_t bytes = (int64_t)sizeof(float2) * b.P;
  if (!p->hfull_cache_full && p->hfull_cache_bytes + bytes <= p->fullband_cache_cap) {
    if (hipMalloc((void**)&keep, (size_t)bytes) == hipSuccess) dst = keep;
    else {                               // no room: compute into the scratch row as before, and stop asking
      (void)hipGetLastError();
      p->hfull_cache_full = true;
    }
  }
  {   // the response enters the cache only once its launch has been accepted: a failed launch must not
      // leave an unfilled buffer behind for later executes to reuse
    SpanGuard sg_(p, ST_FULLBAND);
    int rc_ = sg_.rc;
    if (!rc_) {
      const hipError_t he = launch_fullband_filter(dst, p->d_bank_sc, i, p->d_amps, b.P1, p->stream);
      if (he != hipSuccess) rc_ = hip_err(he, "launch_fullband_filter");
    }
    if (!rc_) rc_ = sg_.end();
    if (rc_) { if (keep) (void)hipFree(keep); return rc_; }
  }
  if (keep) {
    p->hfull_cache[{i, b.P1}] = keep;
    p->hfull_cache_bytes += bytes;
  }
  *h_out = dst;
  return GCWT_OK;
}

// full-band scales: W = IFFT_P(X H_s) for every slot of the batch, up to four scales per pass over X
int fullband_scales(const Call& c, const Batch& b) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  const int S = hp.prm.n_freqs, P1 = b.P1, slots = b.slots;
  const int64_t P = b.P;
  hipStream_t st = p->stream;
  for (int i = 0; i < S && hp.n_fullband > 0;) {
    int member[kFullbandSet], np = 0;
    for (; i < S && np < p->z_sets; ++i)
      if (hp.scales[i].method == GCWT_SCALE_FULLBAND && (!c.hmask || c.hmask[i])) member[np++] = i;
    if (np == 0) break;
    FullbandSet set{};
    set.n = np;
    for (int k = 0; k < np; ++k) {
      set.z[k] = p->d_z + (int64_t)k * p->z_half;
      const int rc_ = fullband_response(c, b, member[k], k, &set.h[k]);
      if (rc_) return rc_;
    }
    if (P1 == 4 && p->fullband4) {       // time blocks of 16 384 samples: both passes in one kernel, no z
      const float2* hh[kFullbandSet];
      int32_t rows_[kFullbandSet];
      for (int k = 0; k < np; ++k) { hh[k] = set.h[k]; rows_[k] = member[k]; }
      RUN(ST_FULLBAND, launch_fullband4(c.mode, p->d_x, hh, rows_, np, c.dout, P, p->d_bc_tw, p->d_tw256, S, c.row_len, b.sout,
                                        slots, st));
      continue;
    }
    // inverse: rows over k2 of the products X H with the W_P^(k1 n2) twiddle, then columns over k1 ->
    // natural order; the usual FFT lengths store from the column pass's registers (2.9 GB of traffic per
    // scale at the headline shape; product, two passes and a store kernel moved 8)
    RUN(ST_FULLBAND, launch_fullband_rows(p->d_x, set, P1, P, P, p->d_bc_tw, p->d_tw256, slots, st,
                                          p->fullband_group));
    for (int k = 0; k < np; ++k) {
      if (fullband_cols_fused(P1)) {
        RUN(ST_FULLBAND, launch_fullband_cols(c.mode, set.z[k], c.dout, P1, P, p->d_tw4096, p->d_tw256, member[k], S,
                                              c.row_len, b.sout, slots, st));
      } else {
        if (P1 > 1)
          RUN(ST_FULLBAND, launch_fft_cols(+1, false, set.z[k], set.z[k], P1, kRowLen, P, P, 0, p->d_tw4096,
                                           p->d_tw256, p->d_sums, c.inv_n, 0, slots, st));
        RUN(ST_FULLBAND, launch_fullband_store(c.mode, set.z[k], c.dout, P, member[k], S, c.row_len, b.sout, b.nb, st));
      }
    }
  }
  return GCWT_OK;
}

// one batch of segments, from the recording to its rows of every scale that reads the spectrum
int run_batch(const Call& c, Batch* b) {
  gcwt_plan* p = c.p;
  int rc;
  if ((rc = forward_transform(c, *b))) return rc;
  if ((rc = level_passes(c, b))) return rc;
  if (!b->early && (rc = join_levels(c, b))) return rc;
  if ((rc = interp_launches(c, b))) return rc;
  if ((rc = pipelined_launches(c, *b))) return rc;
  // (early) every kernel from here on may read a level of group L; so may the next batch (d_x, d_xr and d_xs are reused)
  if (b->early && (rc = join_levels(c, b))) return rc;
  if ((rc = synth16_launch(c, *b))) return rc;
  if ((rc = synth7_launches(c, *b))) return rc;
  // joins: the batch is done when both synthesis kernels are, and when its predictions are (d_hist is free again)
  if (b->si != p->stream && (rc = wait_for(p, p->stream, b->si, "synthesis join"))) return rc;
  if (p->detect && p->d_y && (rc = wait_for(p, p->stream, p->det_stream, "detector join"))) return rc;
  if (p->profiling && !p->hp.levels.empty()) p->last.synth_launches++;
  return fullband_scales(c, *b);
}

// the time-domain scales, up to kSegBatch epochs per launch
int direct_scales(const Call& c) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  const int C = hp.prm.n_channels;
  DirectEpochs eps{};
  eps.n_channels = C;
  int ne = 0;
  auto flush = [&]() -> int {
    if (ne > 0)
      RUN(ST_DIRECT, launch_direct(c.mode, c.dx, c.dout, p->d_psi, p->d_direct_sc, hp.n_direct, p->d_sums,
                                   c.inv_n, hp.prm.n_samples, hp.prm.n_freqs, eps, ne, c.r0, c.row_len, p->max_direct_len,
                                   p->d_psi_tail, p->stream, c.dmask, c.os));
    ne = 0;
    return GCWT_OK;
  };
  int rc = for_clipped_epochs(c, [&](int64_t e0, int64_t e1, int64_t g_lo, int64_t g_hi) -> int {
    eps.epoch_start[ne] = e0;
    eps.epoch_len[ne] = e1 - e0;
    eps.g_lo[ne] = g_lo;
    eps.g_hi[ne] = g_hi;
    // grid.z = epochs * channels of one launch stays within 65535
    return ++ne == kSegBatch || (int64_t)(ne + 1) * C > 65535 ? flush() : GCWT_OK;
  });
  return rc ? rc : flush();
}

// block convolution: per group of scales, per batch of epochs, per chunk of blocks -- the blocks' spectra,
// then every scale of the group from them
int block_convolution(const Call& c) {
  gcwt_plan* p = c.p;
  const HostPlan& hp = p->hp;
  for (const HostPlan::BcGroup& g : hp.bc_groups) {
    if (c.hmask) {                   // masked run: a group none of whose scales is marked makes no block spectra either
      bool wanted = false;
      for (int k = g.first; k < g.first + g.count; ++k) wanted = wanted || c.hmask[hp.bc_order[(size_t)k]];
      if (!wanted) continue;
    }
    BcBlocks bl{};
    bl.n_channels = hp.prm.n_channels;
    bl.hop = g.hop;
    bl.back = g.back;
    bl.ramp = g.ramp;
    int ne = 0;
    auto flush = [&]() -> int {
      bl.n_epochs = ne;
      const int total = ne > 0 ? bl.blk_first[ne] : 0;
      const int chunk = (int)std::max<int64_t>(2, hp.bc_chunk_blocks & ~(int64_t)1);
      for (int b0 = 0; b0 < total; b0 += chunk) {
        const int nblk = std::min(chunk, total - b0);
        RUN(ST_BLOCKCONV, launch_bc_forward(c.dx, p->d_bc_x, bl, b0, nblk, hp.prm.n_samples, p->d_tw64, p->d_sums, c.inv_n, p->stream));
        RUN(ST_BLOCKCONV, launch_bc_scales(c.mode, p->d_bc_x, c.dout, p->d_bc_h + (int64_t)g.first * kRowLen,
                                           p->d_bc_rows + g.first, g.count, p->d_bc_tw, p->d_tw256, bl, b0, nblk,
                                           hp.prm.n_freqs, c.r0, c.row_len, p->stream, c.dmask, c.os));
      }
      ne = 0;
      return GCWT_OK;
    };
    int rc = for_clipped_epochs(c, [&](int64_t e0, int64_t e1, int64_t g_lo, int64_t g_hi) -> int {
      // whole pairs of blocks, even-aligned in recording time: the forward transform carries two blocks at a
      // time, and which two must not depend on the range asked for (execute_block gives execute's bits)
      const int64_t blocks = (((g_hi - 1) / g.hop) | 1) - ((g_lo / g.hop) & ~(int64_t)1) + 1;
      if (ne > 0 && (int64_t)bl.blk_first[ne] + blocks > (1 << 30)) { int rc_ = flush(); if (rc_) return rc_; }
      if (ne == 0) bl.blk_first[0] = 0;
      bl.epoch_start[ne] = e0;
      bl.epoch_stop[ne] = e1;
      bl.g_lo[ne] = g_lo;
      bl.g_hi[ne] = g_hi;
      bl.blk_first[ne + 1] = bl.blk_first[ne] + (int32_t)blocks;
      return ++ne == kSegBatch ? flush() : GCWT_OK;
    });
    if (rc || (rc = flush())) return rc;
  }
  return GCWT_OK;
}

}  // namespace

int run_pipeline(gcwt_plan* p, const float* dx, float* dout, int64_t r0, int64_t r1, int64_t row_len, bool reuse_means) {
  const HostPlan& hp = p->hp;
  const int C = hp.prm.n_channels, S = hp.prm.n_freqs;
  const int64_t N = hp.prm.n_samples;
  p->cur = nullptr;            // (an earlier call may have failed between a fork and its join)
  Call c{};
  c.p = p;
  c.dx = dx;
  c.dout = dout;
  c.r0 = r0;
  c.r1 = r1;
  c.row_len = row_len;
  c.mode = hp.prm.out_mode;
  c.elem = c.mode == GCWT_OUT_COMPLEX_C64 ? 2 : 1;
  c.inv_n = 1.0 / (double)N;
  c.os = make_out_stride(p->out_stride, r0);
  c.hmask = p->run_mask;
  c.dmask = c.hmask ? p->d_run_mask : nullptr;
  // The channel means (transforms.py:142-143).  When the plan is one segment that is the whole recording (no epochs cut
  // out, no time blocks with faded edges, no interleaved transforms) and every scale reads the spectrum, the forward column
  // pass sums the samples it reads anyway and the row pass takes the mean's transform out of its input (fwd64.hip):
  // the recording is read once.  A block request of such a plan runs the same forward side, so it gives the same bits.
  if (p->fold_mean && p->d_y && hp.epochs.size() == 1 && hp.n_direct == 0 && hp.n_blockconv == 0) {
    const EpochPlan& m = hp.epochs[0];
    c.fold = m.start == 0 && m.ne == N && m.lead == 0 && m.ramp_lo == 0 && m.ramp_hi == 0 && m.long_a == 1 &&
             std::max(1, m.batch_count) == 1;
  }
  p->last_fold = c.fold;
  if (!reuse_means && !c.fold) RUN(ST_MEAN, launch_channel_sum(dx, N, C, p->d_sums, p->stream));
  if (p->detect) {
    const hipError_t he = hipMemsetAsync(p->d_pred, 0, sizeof(float) * (size_t)S * (size_t)C * hp.epochs.size(), p->stream);
    if (he != hipSuccess) return hip_err(he, "predictions reset");
  }
  int rc = zero_gaps(c);
  if (rc) return rc;
  // the scales that read the spectrum (spectral, full-band), batch by batch
  const bool any_fft = any_scale(c, [](int m) { return m != GCWT_SCALE_DIRECT && m != GCWT_SCALE_BLOCKCONV; });
  for (size_t e0 = 0; any_fft && e0 < hp.epochs.size();) {
    const size_t count = (size_t)std::max(1, hp.epochs[e0].batch_count);
    Batch b = gather_batch(c, e0, count);
    e0 += count;
    if (b.nb == 0) continue;
    if ((rc = run_batch(c, &b))) return rc;
  }
  if (any_scale(c, [](int m) { return m == GCWT_SCALE_DIRECT; }) && (rc = direct_scales(c))) return rc;
  if (hp.n_blockconv > 0 && (rc = block_convolution(c))) return rc;
  return GCWT_OK;
}

#undef RUN

}  // namespace gcwt
