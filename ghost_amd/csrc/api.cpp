// api.cpp -- C ABI of libghostcwt.so (include/ghostcwt.h): plan objects, device
// workspace, and the orchestration of one transform.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/ghostcwt.h"
#include "../../include/ghostcwt_debug.h"

#include "errors.h"
#include "host_out.h"
#include "interp.h"
#include "kernels.h"
#include "morse_exact.h"
#include "morlet_exact.h"
#include "options.h"
#include "plan_state.h"
#include "planner.h"
#include "work_items.h"

using namespace gcwt;

namespace {
thread_local std::string g_err;
}  // namespace

int gcwt::set_err(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int gcwt::hip_err(hipError_t e, const char* what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? GCWT_ERR_NOMEM : GCWT_ERR_HIP;
}

namespace {

// full-band responses kept on the device across executes (one P-point row per (scale, FFT length)); counted in
// gcwt_plan_info.workspace_bytes
constexpr int64_t kFullbandCacheBytes = (int64_t)16 << 30;   // 193 responses of 2^22 bins (config 5, precision = exact) are 6.2 GB

void free_dev(gcwt_plan* p) {
  auto fr = [](auto*& q) { if (q) { (void)hipFree((void*)q); q = nullptr; } };
  fr(p->d_y); fr(p->d_tw64); fr(p->d_x); fr(p->d_xr); fr(p->d_xb); fr(p->d_xs); fr(p->d_probe); fr(p->d_amps); fr(p->d_z); fr(p->d_hfull); fr(p->d_bank); fr(p->d_gain); fr(p->d_gain_lv); fr(p->d_half_tw); fr(p->d_psi); fr(p->d_psi_tail); fr(p->d_psi_lit); fr(p->d_tw4096);
  fr(p->d_tw256); fr(p->d_level_tw); fr(p->d_sums); fr(p->d_scale_list); fr(p->d_scale_aux); fr(p->d_interp_coef); fr(p->d_bank_sc); fr(p->d_direct_sc); fr(p->d_bc_h); fr(p->d_bc_rows); fr(p->d_bc_x); fr(p->d_bc_tw);
  fr(p->d_in);
  if (p->d_out) { (void)hipFree(p->d_out); p->d_out = nullptr; }
  if (p->h_pred) { (void)hipHostFree(p->h_pred); p->h_pred = nullptr; }
  fr(p->d_hist); fr(p->d_bands); fr(p->d_pred); fr(p->d_scale_level); fr(p->d_scale_length); fr(p->d_run_mask);
  for (gcwt_plan*& sub : p->sub_plan)
    if (sub) { gcwt_plan_destroy(sub); sub = nullptr; }
  for (auto& kv : p->hfull_cache) (void)hipFree(kv.second);
  p->hfull_cache.clear();
  p->hfull_cache_bytes = 0;
  p->host_out.release();
  for (auto& e : p->ep_dev) { fr(e.items); fr(e.levels); fr(e.items7); fr(e.items7w); fr(e.items7n); fr(e.levels7); fr(e.items_i); fr(e.levels_i); fr(e.items_p[0]); fr(e.items_p[1]); fr(e.levels_p); fr(e.pred_levels); }
  p->ep_dev.clear();
  if (p->graph_exec) { (void)hipGraphExecDestroy(p->graph_exec); p->graph_exec = nullptr; }
  for (auto e : p->ev_pool) (void)hipEventDestroy(e);
  p->ev_pool.clear();
  if (p->stream) { (void)hipStreamDestroy(p->stream); p->stream = nullptr; }
  for (auto& q : p->aux) if (q) { (void)hipStreamDestroy(q); q = nullptr; }
  if (p->det_stream) { (void)hipStreamDestroy(p->det_stream); p->det_stream = nullptr; }
  p->uploaded = false;
}

}  // namespace

extern "C" {

int gcwt_abi_version(void) { return GCWT_ABI_VERSION; }

const char* gcwt_last_error(void) { return g_err.c_str(); }

int gcwt_device_count(int* count) {
  if (!count) return set_err(GCWT_ERR_INVALID, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return set_err(GCWT_ERR_NO_DEVICE, hipGetErrorString(e)); }
  *count = n;
  return GCWT_OK;
}

int gcwt_device_name(int device, char* buf, size_t buflen) {
  if (!buf || buflen == 0) return set_err(GCWT_ERR_INVALID, "buf is NULL");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  // some driver stacks leave prop.name empty: say so rather than print a blank
  snprintf(buf, buflen, "%s (%s, %d CUs, %.0f GiB)", prop.name[0] ? prop.name : "AMD GPU (unnamed by the driver)",
           prop.gcnArchName, prop.multiProcessorCount, (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0));
  return GCWT_OK;
}

int gcwt_device_pci_bus_id(int device, char* buf, size_t buflen) {
  if (!buf || buflen < 16) return set_err(GCWT_ERR_INVALID, "buffer of at least 16 bytes needed");
  HIP_TRY(hipDeviceGetPCIBusId(buf, (int)buflen, device));
  return GCWT_OK;
}

int gcwt_set_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    (void)hipGetLastError();
    return set_err(GCWT_ERR_NO_DEVICE, "no HIP device: libghostcwt needs an AMD GPU (gfx950); there is no CPU path");
  }
  if (device < 0 || device >= n) return set_err(GCWT_ERR_NO_DEVICE, "no such device (gcwt_device_count tells how many there are)");
  HIP_TRY(hipSetDevice(device));
  return GCWT_OK;
}
int gcwt_current_device(int* device) {
  if (!device) return set_err(GCWT_ERR_INVALID, "NULL argument");
  HIP_TRY(hipGetDevice(device));
  return GCWT_OK;
}

int gcwt_device_memory(size_t* free_bytes, size_t* total_bytes) {
  if (!free_bytes || !total_bytes) return set_err(GCWT_ERR_INVALID, "NULL argument");
  HIP_TRY(hipMemGetInfo(free_bytes, total_bytes));
  return GCWT_OK;
}
int gcwt_device_malloc(void** ptr, size_t bytes) { HIP_TRY(hipMalloc(ptr, bytes ? bytes : 1)); return GCWT_OK; }
int gcwt_device_free(void* ptr) { HIP_TRY(hipFree(ptr)); return GCWT_OK; }
int gcwt_memcpy_h2d(void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return GCWT_OK;
}
int gcwt_memcpy_d2h(void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return GCWT_OK;
}
int gcwt_device_memset(void* dst, int value, size_t bytes) {
  HIP_TRY(hipMemset(dst, value, bytes)); return GCWT_OK;
}
int gcwt_device_synchronize(void) { HIP_TRY(hipDeviceSynchronize()); return GCWT_OK; }
int gcwt_host_alloc(void** ptr, size_t bytes) {
  if (!ptr) return set_err(GCWT_ERR_INVALID, "NULL argument");
  HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
  return GCWT_OK;
}
int gcwt_host_free(void* ptr) { HIP_TRY(hipHostFree(ptr)); return GCWT_OK; }
int gcwt_rows_to_host(const float* d_src, int64_t src_pitch, int64_t n_rows, int64_t row_elems, void* dst,
                      int64_t dst_pitch, int flags) {
  return guarded([&] {
    if (!d_src || !dst) return set_err(GCWT_ERR_INVALID, "NULL argument");
    if (n_rows < 0 || row_elems < 0 || src_pitch < row_elems || dst_pitch < row_elems)
      return set_err(GCWT_ERR_INVALID, "bad rectangle (rows, elements per row, pitches)");
    if (!(flags & GCWT_HOST_PINNED) && dst_pitch != row_elems)
      return set_err(GCWT_ERR_INVALID, "a destination that is not page-locked takes dense rows (dst_pitch = row_elems)");
    HIP_TRY(rows_to_host(d_src, src_pitch, n_rows, row_elems, dst, dst_pitch, (flags & GCWT_OUT_F64) != 0,
                         (flags & GCWT_HOST_PINNED) != 0));
    return (int)GCWT_OK;
  });
}

static int gcwt_plan_create_impl(gcwt_plan** out, const gcwt_params* params) {
  if (!out || !params) return set_err(GCWT_ERR_INVALID, "NULL argument");
  *out = nullptr;
  // (held by a unique_ptr until it is handed over: build_host_plan may throw std::bad_alloc, which guarded()
  // turns into GCWT_ERR_NOMEM after the partly built plan is gone)
  std::unique_ptr<gcwt_plan> owner(new (std::nothrow) gcwt_plan());
  gcwt_plan* p = owner.get();
  if (!p) return set_err(GCWT_ERR_NOMEM, "out of host memory");
  std::string err;
  int rc = build_host_plan(*params, &p->hp, &err);
  if (rc != GCWT_OK) return set_err(rc, err);
  // the plan keeps its own copies of the arrays
  p->hp.prm.freqs_hz = p->hp.freqs.data();
  p->hp.prm.epoch_bounds = p->hp.bounds.data();
  p->hp.prm.n_epochs = (int32_t)(p->hp.bounds.size() / 2);
  p->device = params->device;
  p->high_precision = p->hp.high_precision;
  // options (options.h): read once, here; an execute never looks at them or at the environment
  p->use_synth16 = option_or("synth16", 0) == 1;
  p->synth_cols = option_or("synth_cols", 32) == 16 ? 16 : 32;
  p->synth7_narrow_r = (int)option_or("synth7_narrow_r", 2);
  p->fuse_blocks = option_or("fuse_blocks", 1) != 0;
  p->prune_inputs = option_or("prune_inputs", 1) != 0;
  p->fast_fft = option_or("slow_fft", 0) == 0;
  p->level_streams = option_or("level_streams", 1) != 0;
  if (option_is_set("interp_grid")) p->interp_grid = option_or("interp_grid", 0) != 0;
  p->synth_streams = option_or("synth_streams", 0) != 0;
  p->fold_mean = option_or("fold_mean", 1) != 0;
  p->early_interp = option_or("early_interp", 0) != 0;
  p->interp_split_r = (int)std::min<long long>(1 << 30, std::max<long long>(0, option_or("interp_split_r", 64)));
  p->interp_lgnb = (int)option_or("interp_lgnb", -1);
  p->use_synthp = kMeasureBuild && option_or("synthp", 0) != 0;   // (the kernel exists in the measure build only)
  p->synthp_lgnb = (int)option_or("synthp_lgnb", -1);
  p->synthp_help = (int)option_or("synthp_help", -1);
  p->use_graphs = option_or("graphs", 1) != 0;
  p->synth7_order = (int)option_or("synth7_order", 0);
  p->auto_threshold = 1e-9f * (float)option_or("auto_threshold_ppb", 1500);
  p->kappa_eps = 1e-9f * (float)option_or("auto_kappa_ppb", 160);
  p->oob_tol = 1e-12f * (float)option_or("auto_oob_ppt", 25000);
  p->fullband_group = (int)option_or("fullband_group", 0);
  p->fullband4 = option_or("fullband4", 1) != 0;
  p->synth_kernel = kMeasureBuild && option_or("synth_kernel", 7) == 8 ? 8 : 7;
  p->drop_stores = kMeasureBuild && option_is_set("synth_drop_stores") ? (int)std::max<long long>(1, option_or("synth_drop_stores", 1)) : 0;
  p->clock_probe = kMeasureBuild && option_is_set("clock_probe");
  for (const auto& s : p->hp.scales)
    if (s.method == GCWT_SCALE_DIRECT) p->max_direct_len = std::max(p->max_direct_len, s.length);
  *out = owner.release();
  return GCWT_OK;
}

void gcwt_plan_destroy(gcwt_plan* plan) {
  if (!plan) return;
  if (plan->uploaded || plan->stream) {
    if (plan->device >= 0) (void)hipSetDevice(plan->device);
    free_dev(plan);
  }
  delete plan;
}

int gcwt_plan_get_info(const gcwt_plan* plan, gcwt_plan_info* info) {
  if (!plan || !info) return set_err(GCWT_ERR_INVALID, "NULL argument");
  const HostPlan& hp = plan->hp;
  info->abi_version = GCWT_ABI_VERSION;
  info->n_levels = (int32_t)hp.levels.size();
  info->n_direct = hp.n_direct;
  info->n_spectral = (int32_t)hp.scales.size() - hp.n_direct - hp.n_fullband - hp.n_blockconv;
  info->n_fullband = hp.n_fullband;
  info->n_blockconv = hp.n_blockconv;
  info->reserved = 0;
  info->n_interp = 0;
  for (const auto& l : hp.levels)
    if (level_kernel(plan, l) == LK_INTERP) info->n_interp += (int32_t)l.scales.size();
  info->block = hp.block;
  int r = 1;
  for (const auto& l : hp.levels) r = std::max(r, l.decimation);
  info->max_decimation = r;
  info->fft_length = hp.max_p;
  // the planner's figure (X, x_R, XB, Z, bank, tables) plus what this file allocates on top of it
  {
    const int64_t C = hp.prm.n_channels, slots = C * hp.max_batch;
    int64_t extra = 0, xs = 0, y = 0;
    for (const EpochPlan& ep : hp.epochs) {
      for (size_t l = 0; l < hp.levels.size(); ++l)
        if (hp.levels[l].band_shift > 0) xs = std::max<int64_t>(xs, ep.lv[l].m);
      const int rows = ep.p1 >= 4 && hp.n_fullband == 0 ? ep.p1 / 2 + 1 : ep.p1;
      y = std::max<int64_t>(y, (int64_t)rows * kRowLen);
    }
    extra += 8 * 3 * slots * xs;                                        // shifted-band slices, one per level stream
    if (hp.high_precision && plan->fast_fft && hp.n_direct + hp.n_blockconv < hp.prm.n_freqs)
      extra += 16 * (slots * y + 8192);   // float64 intermediate + twiddles (what gcwt_plan_upload allocates: d_y, d_tw64)
    extra += 8 * (2 * (int64_t)hp.direct_total + (int64_t)hp.n_direct);   // literal taps and tap sums beside the running sums
    int64_t listed = 0;
    for (const LevelPlan& lp : hp.levels) listed += (int64_t)lp.scales.size();
    extra += 4 * (listed + 8) * 256 + 8 * 256 * (int64_t)hp.levels.size();   // gain rows in list order, half-sample twiddles
    extra += 8 * (int64_t)channel_sum_doubles((size_t)C) + 4 * (int64_t)hp.interp_coef.size();
    if (hp.high_precision && !hp.exact_only) {             // the detector's band sums and predictions (precision auto / high)
      int64_t max_rows = 1;
      for (const EpochPlan& ep : hp.epochs) max_rows = std::max<int64_t>(max_rows, ep.p1);
      extra += 4 * (slots * (max_rows * kRowBands + kSpecBands) + (int64_t)hp.prm.n_freqs * (int64_t)hp.epochs.size());
    }
    if (hp.n_fullband > 0)
      extra += std::min<int64_t>(plan->uploaded ? plan->fullband_cache_cap : kFullbandCacheBytes,
                                 8 * (int64_t)hp.n_fullband * hp.max_p * (int64_t)hp.epochs.size());
    info->workspace_bytes = hp.workspace_bytes + extra;
    // precision = auto: the exact sub-plans a recording with in-band interference made this plan create (at most two,
    // kept for later executes) are device memory of this plan too
    for (const gcwt_plan* sub : plan->sub_plan) {
      gcwt_plan_info si{};
      if (sub && gcwt_plan_get_info(sub, &si) == GCWT_OK) info->workspace_bytes += si.workspace_bytes;
    }
  }
  info->out_bytes = (int64_t)hp.out_elem_bytes * hp.prm.n_channels * hp.prm.n_freqs *
                    stride_cols(0, hp.prm.n_samples, plan->out_stride);
  return GCWT_OK;
}

int gcwt_plan_scale_info(const gcwt_plan* plan, int32_t* method, int32_t* decimation, int32_t* halo,
                         int32_t* hop, int64_t* length) {
  if (!plan) return set_err(GCWT_ERR_INVALID, "NULL plan");
  const HostPlan& hp = plan->hp;
  for (size_t i = 0; i < hp.scales.size(); ++i) {
    const ScalePlan& s = hp.scales[i];
    if (method) method[i] = s.method;
    if (decimation) decimation[i] = s.method == GCWT_SCALE_SPECTRAL ? s.decimation : 1;
    if (halo) halo[i] = s.level >= 0 ? hp.levels[s.level].halo : 0;
    if (hop) hop[i] = s.level >= 0 ? hp.levels[s.level].hop : 0;
    if (length) length[i] = s.length;
  }
  return GCWT_OK;
}

int gcwt_plan_scale_support(const gcwt_plan* plan, double* theta_hi, double* support, int32_t* n_bins) {
  if (!plan) return set_err(GCWT_ERR_INVALID, "NULL plan");
  const HostPlan& hp = plan->hp;
  for (size_t i = 0; i < hp.scales.size(); ++i) {
    const ScalePlan& s = hp.scales[i];
    if (theta_hi) theta_hi[i] = s.theta_hi;
    if (support) support[i] = s.support;
    if (n_bins) n_bins[i] = s.n_bins;
  }
  return GCWT_OK;
}

int gcwt_plan_set_profiling(gcwt_plan* plan, int enabled) {
  if (!plan) return set_err(GCWT_ERR_INVALID, "NULL plan");
  plan->profiling = enabled == 2 ? 2 : (enabled != 0 ? 1 : 0);
  return GCWT_OK;
}

int gcwt_plan_set_row_pitch(gcwt_plan* plan, int64_t pitch_samples) {
  if (!plan || pitch_samples < 0) return set_err(GCWT_ERR_INVALID, "bad row pitch");
  plan->row_pitch = pitch_samples;
  return GCWT_OK;
}

int gcwt_plan_set_output_stride(gcwt_plan* plan, int64_t stride) {
  if (!plan) return set_err(GCWT_ERR_INVALID, "NULL plan");
  if (stride < 1 || stride > 0x7fffffff) return set_err(GCWT_ERR_INVALID, "output stride must be an integer >= 1");
  if (plan->uploaded) return set_err(GCWT_ERR_INVALID, "output stride set after the plan's first upload or execute");
  // the strided stores find a sample's column with 32-bit arithmetic (kernels.h: stride_keep)
  if (stride > 1 && plan->hp.prm.n_samples >= ((int64_t)1 << 31))
    return set_err(GCWT_ERR_UNSUPPORTED, "output stride on recordings of 2^31 samples or more");
  plan->out_stride = stride;
  return GCWT_OK;
}

// ---- gcwt_plan_upload: streams, workspace, tables, the batches' work items, the table-building launches ----------
namespace {

// The host side of the tables an upload sends with hipMemcpyAsync: it lives until the plan's stream has taken them
// (the synchronize at the end of build_tables).
struct HostTables {
  std::vector<float2> tw4096, tw256, level_tw, half_tw;
  std::vector<BankScale> bank_sc;
  std::vector<DirectScale> direct_sc;
  std::vector<int32_t> bc_rows, scale_aux;
  ScaleLists lists;
  struct Batch {
    Synth16Items s16;
    Synth7Items s7;
    SynthiItems si;
    SynthpItems sp;
  };
  std::vector<Batch> batches;
};

// option cu_count (measurements: profiles/r06_bound.md): the plan's streams may use that many of the CUs only.  The
// mask's bits are dealt round-robin over the XCDs by the driver, so its first n bits are n / 8 CUs of each.
hipError_t make_stream(hipStream_t* q) {
  const int n_cu = (int)option_or("cu_count", 0);
  if (n_cu <= 0) return hipStreamCreateWithFlags(q, hipStreamNonBlocking);
  uint32_t mask[16] = {};
  for (int i = 0; i < n_cu && i < 512; ++i) mask[i >> 5] |= 1u << (i & 31);
  return hipExtStreamCreateWithCUMask(q, 16, mask);
}

int upload_streams(gcwt_plan* p) {
  HIP_TRY(make_stream(&p->stream));
  for (auto& q : p->aux) HIP_TRY(make_stream(&q));
  HIP_TRY(make_stream(&p->det_stream));
  return GCWT_OK;
}

// the float64 twiddle tables of fwd64.hip (the forward transform, the block convolution's forward pass)
int upload_fwd64_table(gcwt_plan* p) {
  std::vector<double2> tw(8192);
  fwd64_fill_tables(tw.data());
  int rc = upload_vec(&p->d_tw64, tw, p->stream);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(p->stream));       // `tw` goes out of scope
  return GCWT_OK;
}

// spectrum, float64 intermediate, x_R, block spectra, band-shift slices, full-band products: one workspace slot per
// (segment of a batch, channel)
int upload_workspace(gcwt_plan* p) {
  const HostPlan& hp = p->hp;
  int rc;
  if (hp.n_direct + hp.n_blockconv >= hp.prm.n_freqs) return GCWT_OK;   // no spectral or full-band scale: they share X
  const int64_t slots = (int64_t)hp.prm.n_channels * hp.max_batch;
  if ((rc = dev_alloc(&p->d_x, (size_t)(slots * hp.max_p_store)))) return rc;
  if (p->high_precision && p->fast_fft) {
    // rows 0 .. P1/2 of the intermediate (all of them when full-band scales read the whole spectrum)
    for (const EpochPlan& ep : hp.epochs) {
      const int rows = ep.p1 >= 4 && hp.n_fullband == 0 ? ep.p1 / 2 + 1 : ep.p1;
      p->y_stride = std::max<int64_t>(p->y_stride, (int64_t)rows * kRowLen);
    }
    if ((rc = dev_alloc(&p->d_y, (size_t)(slots * p->y_stride)))) return rc;
    if ((rc = upload_fwd64_table(p))) return rc;
  }
  if ((rc = dev_alloc(&p->d_xr, (size_t)(slots * hp.max_xr)))) return rc;
  if ((rc = dev_alloc(&p->d_xb, (size_t)(slots * hp.max_xb)))) return rc;
  for (const EpochPlan& ep : hp.epochs)
    for (size_t l = 0; l < hp.levels.size(); ++l)
      if (hp.levels[l].band_shift > 0) p->xs_stride = std::max(p->xs_stride, ep.lv[l].m);
  // one slice buffer per stream the level passes run on (pipeline.cpp: three streams)
  if (p->xs_stride > 0 && (rc = dev_alloc(&p->d_xs, (size_t)(3 * slots * p->xs_stride)))) return rc;
  if (hp.n_fullband > 0) {
    p->z_sets = std::min(hp.n_fullband, kFullbandSet);   // that many scales share a pass over X
    p->z_half = slots * hp.max_p;
    if ((rc = dev_alloc(&p->d_z, (size_t)(p->z_sets * p->z_half)))) return rc;
    if ((rc = dev_alloc(&p->d_hfull, (size_t)(p->z_sets * hp.max_p)))) return rc;
  }
  return GCWT_OK;
}

// what does not depend on the levels: amplitudes, the bank's and the direct kernels' buffers, the channel sums, the
// twiddle tables (computed in double on the host), the scales' descriptors, the block convolution's tables
int upload_constant_tables(gcwt_plan* p, HostTables* ht) {
  const HostPlan& hp = p->hp;
  const int64_t C = hp.prm.n_channels;
  const int S = hp.prm.n_freqs, B = hp.block;
  int rc;
  if ((rc = upload_vec(&p->d_amps, hp.amps, p->stream))) return rc;
  if (p->clock_probe) {
    if ((rc = dev_alloc(&p->d_probe, 8))) return rc;
    hipError_t he0 = hipMemsetAsync(p->d_probe, 0, 64, p->stream);
    if (he0 != hipSuccess) return hip_err(he0, "probe reset");
  }
  if ((rc = dev_alloc(&p->d_bank, (size_t)S * B))) return rc;
  if ((rc = dev_alloc(&p->d_gain, (size_t)S * B))) return rc;
  if ((rc = dev_alloc(&p->d_psi, (size_t)hp.direct_total))) return rc;
  if ((rc = dev_alloc(&p->d_psi_lit, (size_t)hp.direct_total))) return rc;
  if ((rc = dev_alloc(&p->d_psi_tail, (size_t)hp.n_direct))) return rc;
  {   // zero taps in front of every kernel and behind it up to a multiple of 8 (+8): k_direct reads whole groups
    hipError_t hz = hipMemsetAsync(p->d_psi, 0, sizeof(float2) * (size_t)std::max<int64_t>(1, hp.direct_total), p->stream);
    if (hz != hipSuccess) return hip_err(hz, "psi reset");
  }
  if ((rc = dev_alloc(&p->d_sums, channel_sum_doubles((size_t)C)))) return rc;
  {   // results and partial sums of k_channel_sum
    hipError_t hz = hipMemsetAsync(p->d_sums, 0, sizeof(double) * channel_sum_doubles((size_t)C), p->stream);
    if (hz != hipSuccess) return hip_err(hz, "sums reset");
  }

  ht->tw4096.resize(kRowLen / 2);
  ht->tw256.resize(256);
  ht->level_tw.resize((size_t)hp.level_twiddle_total);
  for (int j = 0; j < kRowLen / 2; ++j) {
    double a = -2.0 * M_PI * j / kRowLen;
    ht->tw4096[j] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  for (int q = 0; q < 256; ++q) {
    double a = 2.0 * M_PI * q / 256.0;
    ht->tw256[q] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  for (const LevelPlan& lp : hp.levels) {
    const int64_t n = (int64_t)kSynthCols * lp.decimation;
    for (int64_t q = 0; q < n; ++q) {
      double a = 2.0 * M_PI * (double)q / ((double)B * lp.decimation);
      ht->level_tw[lp.twiddle_offset + q] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
  }
  if ((rc = upload_vec(&p->d_tw4096, ht->tw4096, p->stream))) return rc;
  if ((rc = upload_vec(&p->d_tw256, ht->tw256, p->stream))) return rc;
  if ((rc = upload_vec(&p->d_level_tw, ht->level_tw, p->stream))) return rc;

  ht->bank_sc.resize(S);
  ht->direct_sc.resize(hp.n_direct);
  for (int i = 0; i < S; ++i) {
    const ScalePlan& s = hp.scales[i];
    ht->bank_sc[i] = {s.omega, s.half_delay, s.length, s.amp_offset, s.bin_lo, s.n_bins, s.decimation,
                      s.method == GCWT_SCALE_SPECTRAL ? 1 : 0,
                      s.method == GCWT_SCALE_SPECTRAL ? hp.levels[s.level].band_shift : 0, hp.morlet ? 1 : 0,
                      hp.morlet ? hp.prm.gamma : 0.0, s.sigma};
    if (s.method == GCWT_SCALE_DIRECT)
      ht->direct_sc[s.direct_index] = {s.omega, s.length, s.amp_offset, s.direct_offset, i, s.bin_lo, s.n_bins,
                                       direct_front_pad(s.length), hp.morlet ? 1 : 0, 0, hp.morlet ? hp.prm.gamma : 0.0,
                                       s.sigma, s.c0};
  }
  if ((rc = upload_vec(&p->d_bank_sc, ht->bank_sc, p->stream))) return rc;
  if ((rc = upload_vec(&p->d_direct_sc, ht->direct_sc, p->stream))) return rc;
  if (hp.n_blockconv > 0 || hp.n_fullband > 0) {
    // W_4096^(+(t + 16 j) a) at [256 j + 16 t + a]: the middle twiddles of the 4096-point inverse transforms of
    // k_bc_scales and k_fullband_rows as each thread meets them (the values tw4096_at<+1> gives)
    std::vector<float2> twt(kRowLen);
    for (int j = 0; j < 16; ++j)
      for (int tid = 0; tid < 256; ++tid) {
        const int idx = (((tid >> 4) + 16 * j) * (tid & 15)) & (kRowLen - 1);
        float2 w = ht->tw4096[idx & 2047];
        if (idx & 2048) w = make_float2(-w.x, -w.y);
        twt[256 * j + tid] = make_float2(w.x, -w.y);
      }
    if ((rc = upload_vec(&p->d_bc_tw, twt, p->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));         // `twt` goes out of scope
  }
  if (hp.n_blockconv > 0) {
    ht->bc_rows.assign(hp.bc_order.begin(), hp.bc_order.end());
    if ((rc = upload_vec(&p->d_bc_rows, ht->bc_rows, p->stream))) return rc;
    if ((rc = dev_alloc(&p->d_bc_h, (size_t)hp.n_blockconv * kRowLen))) return rc;
    if ((rc = dev_alloc(&p->d_bc_x, (size_t)(hp.bc_chunk_blocks * C) * kRowLen))) return rc;
    if (!p->d_tw64 && (rc = upload_fwd64_table(p))) return rc;
  }
  return GCWT_OK;
}

// the levels' scale lists and what goes with them, in list order
int upload_scale_tables(gcwt_plan* p, HostTables* ht) {
  const HostPlan& hp = p->hp;
  int rc;
  ht->lists = level_scale_lists(hp);
  ht->half_tw = half_twiddles(hp);
  ht->scale_aux = scale_aux(hp, ht->lists.list);
  if ((rc = upload_vec(&p->d_half_tw, ht->half_tw, p->stream))) return rc;
  if ((rc = upload_vec(&p->d_scale_list, ht->lists.list, p->stream))) return rc;
  if ((rc = upload_vec(&p->d_scale_aux, ht->scale_aux, p->stream))) return rc;
  if ((rc = upload_vec(&p->d_interp_coef, hp.interp_coef, p->stream))) return rc;
  p->n_listed = (int)ht->lists.list.size();
  // k_synth7 reads whole chunks of 8 rows: 8 rows of zeros behind the last level's
  const size_t n = ((size_t)p->n_listed + 8) * 256 * (hp.morlet ? 2 : 1);     // (Morlet plans: complex rows)
  if ((rc = dev_alloc(&p->d_gain_lv, n))) return rc;
  hipError_t hz = hipMemsetAsync(p->d_gain_lv, 0, sizeof(float) * n, p->stream);
  if (hz != hipSuccess) return hip_err(hz, "gain rows reset");
  return GCWT_OK;
}

// the work items of one launch batch (work_items.h) and their level tables
int upload_batch_items(gcwt_plan* p, size_t e, const ScaleLists& sl, HostTables::Batch* b) {
  const EpochPlan& ep = p->hp.epochs[e];
  EpochDev& dev = p->ep_dev[e];
  hipStream_t st = p->stream;
  int rc;
  b->s16 = synth16_items(p, ep);
  dev.n_items = (int)b->s16.items.size();
  if ((rc = upload_vec(&dev.items, b->s16.items, st))) return rc;
  if ((rc = upload_vec(&dev.levels, b->s16.levels, st))) return rc;
  b->s7 = synth7_items(p, ep, sl);
  dev.n_items7 = (int)b->s7.items.size();
  dev.n_items7w = (int)b->s7.wide.size();
  dev.n_items7n = (int)b->s7.narrow.size();
  if ((rc = upload_vec(&dev.items7n, b->s7.narrow, st))) return rc;
  if ((rc = upload_vec(&dev.items7, b->s7.items, st))) return rc;
  if ((rc = upload_vec(&dev.items7w, b->s7.wide, st))) return rc;
  if ((rc = upload_vec(&dev.levels7, b->s7.levels, st))) return rc;
  if ((rc = synthi_items(p, ep, sl, &b->si))) return rc;
  dev.split_i = b->si.split;
  dev.n_items_i = (int)b->si.items.size();
  if ((rc = upload_vec(&dev.items_i, b->si.items, st))) return rc;
  if ((rc = upload_vec(&dev.levels_i, b->si.levels, st))) return rc;
  if ((rc = synthp_items(p, ep, sl, &b->sp))) return rc;
  for (int k = 0; k < 2; ++k) {
    dev.n_items_p[k] = (int)b->sp.items[k].size();
    if ((rc = upload_vec(&dev.items_p[k], b->sp.items[k], st))) return rc;
  }
  return upload_vec(&dev.levels_p, b->sp.levels, st);
}

// precision = auto / high: the detector's tables (detect.hip)
int upload_detector(gcwt_plan* p) {
  const HostPlan& hp = p->hp;
  const int64_t C = hp.prm.n_channels;
  const int S = hp.prm.n_freqs;
  int rc;
  bool long_mode = false, any_level = false;
  for (const EpochPlan& ep : hp.epochs) long_mode = long_mode || ep.long_a > 1;
  std::vector<int32_t> scale_level((size_t)S, -1);
  for (int i = 0; i < S; ++i)
    if (hp.scales[i].method == GCWT_SCALE_SPECTRAL && hp.scales[i].level >= 0) { scale_level[(size_t)i] = hp.scales[i].level; any_level = true; }
  p->detect = hp.high_precision && !hp.exact_only && p->d_y && !long_mode && any_level;
  if (!p->detect) return GCWT_OK;
  const int64_t slots = (int64_t)C * hp.max_batch;
  int64_t max_rows = 1;                              // rows of the forward row pass: pipeline.cpp's rows_a
  for (const EpochPlan& ep : hp.epochs)
    max_rows = std::max<int64_t>(max_rows, ep.p1);
  if ((rc = dev_alloc(&p->d_hist, (size_t)(slots * max_rows * kRowBands)))) return rc;
  if ((rc = dev_alloc(&p->d_bands, (size_t)(slots * kSpecBands)))) return rc;
  if ((rc = dev_alloc(&p->d_pred, (size_t)S * (size_t)C * hp.epochs.size()))) return rc;
  if ((rc = upload_vec(&p->d_scale_level, scale_level, p->stream))) return rc;
  std::vector<int32_t> scale_length((size_t)S);
  for (int i = 0; i < S; ++i) scale_length[(size_t)i] = (int32_t)std::min<int64_t>(hp.scales[i].length, (int64_t)1 << 30);
  if ((rc = upload_vec(&p->d_scale_length, scale_length, p->stream))) return rc;
  std::vector<std::vector<PredLevel>> pred_levels(hp.epochs.size());
  for (size_t e = 0; e < hp.epochs.size(); ++e) {
    const EpochPlan& ep = hp.epochs[e];
    if (ep.batch_count == 0) continue;
    std::vector<PredLevel>& pl = pred_levels[e];
    pl.resize(hp.levels.size());
    for (size_t l = 0; l < hp.levels.size(); ++l) {
      const LevelPlan& lp = hp.levels[l];
      const LevelPlan& own = hp.levels[lp.xr_owner >= 0 ? (size_t)lp.xr_owner : l];   // whose x_R the level reads
      pl[l] = {lp.scales.empty() ? 0 : lp.decimation, lp.band_shift, 0.f, 0.f};
      if (own.taper_hi > 0.0 && own.band_shift == 0) {                                 // pipeline.cpp: RowTaper
        const double k1 = own.taper_hi * (double)ep.p / (2.0 * M_PI), k0 = 0.5 * k1;
        if (k1 - k0 >= 1.0) { pl[l].k0 = (float)k0; pl[l].k1 = (float)k1; }
      }
    }
    if ((rc = upload_vec(&p->ep_dev[e].pred_levels, pl, p->stream))) return rc;
  }
  p->last_pred.assign((size_t)S, 0.f);
  HIP_TRY(hipHostMalloc((void**)&p->h_pred, sizeof(float) * (size_t)S * (size_t)C * hp.epochs.size(), hipHostMallocDefault));
  HIP_TRY(hipStreamSynchronize(p->stream));       // the vectors of this function go out of scope
  return GCWT_OK;
}

// the launches that make the bank, the gain rows, the direct kernels and the block convolution's responses
int build_tables(gcwt_plan* p) {
  const HostPlan& hp = p->hp;
  const int S = hp.prm.n_freqs, B = hp.block;
  hipError_t he = launch_build_bank(p->d_bank, p->d_gain, p->d_bank_sc, p->d_amps, S, B, p->stream);
  if (he != hipSuccess) return hip_err(he, "build_bank");
  he = launch_scale_windows(p->d_gain, p->d_scale_list, p->n_listed, (float)hp.band_tol, p->d_gain_lv,
                            p->prune_inputs, p->stream);
  if (he != hipSuccess) return hip_err(he, "scale_windows");
  if (hp.morlet) {          // the rows k_synth7 reads are the bank's complex ones (the windows above are set from |H|)
    he = launch_gain_rows_complex(p->d_bank, p->d_scale_list, p->n_listed, reinterpret_cast<float2*>(p->d_gain_lv), p->stream);
    if (he != hipSuccess) return hip_err(he, "gain_rows_complex");
  }
  he = launch_build_direct(p->d_psi, p->d_direct_sc, hp.n_direct, p->max_direct_len, p->d_amps, p->d_psi_tail,
                           p->d_psi_lit, p->stream);
  if (he != hipSuccess) return hip_err(he, "build_direct");
  for (int k = 0; k < hp.n_blockconv; ++k) {      // H on the 4096-point grid of a block, over 4096 (exact.hip)
    he = launch_fullband_filter(p->d_bc_h + (int64_t)k * kRowLen, p->d_bank_sc, hp.bc_order[k], p->d_amps, 1, p->stream);
    if (he != hipSuccess) return hip_err(he, "blockconv responses");
  }
  he = hipStreamSynchronize(p->stream);  // the HostTables go out of scope
  if (he != hipSuccess) return hip_err(he, "plan upload");
  return GCWT_OK;
}

int upload_steps(gcwt_plan* p) {
  const HostPlan& hp = p->hp;
  HostTables ht;
  int rc;
  if ((rc = upload_streams(p))) return rc;
  if ((rc = upload_workspace(p))) return rc;
  if ((rc = upload_constant_tables(p, &ht))) return rc;
  if ((rc = upload_scale_tables(p, &ht))) return rc;
  p->ep_dev.resize(hp.epochs.size());
  ht.batches.resize(hp.epochs.size());
  for (size_t e = 0; e < hp.epochs.size(); ++e) {
    if (hp.epochs[e].batch_count == 0) continue;     // shares the tables of its batch's first segment
    if ((rc = upload_batch_items(p, e, ht.lists, &ht.batches[e]))) return rc;
  }
  if ((rc = upload_detector(p))) return rc;
  return build_tables(p);
}

}  // namespace

static int gcwt_plan_upload_impl(gcwt_plan* p) {
  if (!p) return set_err(GCWT_ERR_INVALID, "NULL plan");
  if (p->uploaded) return GCWT_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return set_err(GCWT_ERR_NO_DEVICE,
                   "no HIP device: libghostcwt needs an AMD GPU (gfx950); there is no CPU path");
  if (p->device >= 0) HIP_TRY(hipSetDevice(p->device));
  const int rc = upload_steps(p);
  if (rc) {                                        // whatever failed: nothing of a half-made upload stays
    free_dev(p);
    return rc;
  }
  if (p->hp.n_fullband > 0) {
    // full-band responses kept across executes: a quarter of what is free now (after the workspace), at most
    // 16 GiB; option fullband_cache_mb sets it (0: none are kept).  Nothing is allocated for it here: a response
    // enters the cache when its scale is first computed, and a failed allocation closes the cache.
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    p->fullband_cache_cap = std::min<int64_t>(kFullbandCacheBytes, (int64_t)(free_b / 4));
    if (p->is_sub_plan) p->fullband_cache_cap /= 2;      // two of them may live inside one parent
    if (option_is_set("fullband_cache_mb")) p->fullband_cache_cap = std::max<long long>(0, option_or("fullband_cache_mb", 0)) << 20;
  }
  p->uploaded = true;
  return GCWT_OK;
}

static int execute_range(gcwt_plan* p, const void* x, void* out, int64_t r0, int64_t r1, int flags);
static int gcwt_plan_create_impl(gcwt_plan** out, const gcwt_params* params);

// precision = auto: samples [r0, r1) of the scales `over` again (dout's rows start at sample out_r0), by a plan of precision = exact that holds just
// them (made on first use, kept per set of scales), from the same device-resident recording; its dense rows are
// copied over the fast path's.  The sub-plan computes its own channel means (same numbers: same kernel, same x).
static int reroute_scales(gcwt_plan* p, const float* dx, float* dout, int64_t out_r0, int64_t r0, int64_t r1, int64_t row_len,
                          const std::vector<int32_t>& over, int channel) {
  // channel >= 0: that channel alone, by the one-channel sub-plan (a recording with one bad electrode pays for one).
  // The sub-plans hold every scale and a run is masked to `over`: whatever the verdicts of a recording's segments
  // are -- every epoch its own set -- two plans serve them all, and a scale's numbers do not depend on the set it
  // is asked for in (a plan per set cost 35 ms each time a set came back after four others).
  const HostPlan& hp = p->hp;
  const int S = hp.prm.n_freqs;
  const int nch = channel >= 0 ? 1 : hp.prm.n_channels;
  gcwt_plan*& sub = p->sub_plan[channel >= 0 ? 1 : 0];
  if (!sub) {
    std::vector<double> f(hp.freqs.begin(), hp.freqs.end());
    gcwt_params prm = hp.prm;
    prm.freqs_hz = f.data();
    prm.n_freqs = (int32_t)f.size();
    prm.n_channels = nch;
    prm.precision = GCWT_PRECISION_EXACT;
    prm.device = p->device;
    int rc = gcwt_plan_create_impl(&sub, &prm);
    if (rc) { sub = nullptr; return rc; }
    const HostPlan& sh = sub->hp;
    if ((int)sh.scales.size() != S || sh.n_direct + sh.n_blockconv + sh.n_fullband != S) {
      gcwt_plan_destroy(sub); sub = nullptr;
      return set_err(GCWT_ERR_INVALID, "internal: the exact sub-plan keeps a decimated scale");
    }
    sub->is_sub_plan = true;
    sub->out_stride = p->out_stride;       // the rerouted rows land in the strided rows
    if ((rc = gcwt_plan_upload(sub))) { gcwt_plan_destroy(sub); sub = nullptr; return rc; }
    if (hipMalloc((void**)&sub->d_run_mask, (size_t)S) != hipSuccess) {
      (void)hipGetLastError();
      gcwt_plan_destroy(sub); sub = nullptr;
      return set_err(GCWT_ERR_NOMEM, "no device memory for the rerouted scales' mask");
    }
  }
  std::vector<unsigned char> mask((size_t)S, 0);
  for (int32_t i : over) mask[(size_t)i] = 1;
  HIP_TRY(hipMemcpy(sub->d_run_mask, mask.data(), (size_t)S, hipMemcpyHostToDevice));
  const int elem = hp.out_elem_bytes / (int)sizeof(float);
  const int64_t ch0 = channel >= 0 ? channel : 0;
  float* dst = dout + (ch0 * S * row_len + stride_cols(out_r0, r0, p->out_stride)) * elem;
  sub->row_pitch = row_len;
  sub->run_mask = mask.data();
  const int rc = execute_range(sub, dx + ch0 * hp.prm.n_samples, dst, r0, r1, GCWT_X_ON_DEVICE | GCWT_OUT_ON_DEVICE);
  sub->run_mask = nullptr;
  return rc;
}

// host input goes through the plan's d_in, host output through its d_out (drained to the caller at the end)
static int stage_buffers(gcwt_plan* p, const void* x, void* out, int flags, size_t in_bytes, size_t out_bytes,
                         const float** dx, float** dout) {
  if (flags & GCWT_X_ON_DEVICE) {
    *dx = (const float*)x;
  } else {
    if (p->d_in_bytes < in_bytes) {
      if (p->d_in) { (void)hipFree(p->d_in); p->d_in = nullptr; p->d_in_bytes = 0; }
      HIP_TRY(hipMalloc((void**)&p->d_in, in_bytes));
      p->d_in_bytes = in_bytes;
    }
    HIP_TRY(hipMemcpyAsync(p->d_in, x, in_bytes, hipMemcpyHostToDevice, p->stream));
    *dx = p->d_in;
  }
  if (flags & GCWT_OUT_ON_DEVICE) {
    *dout = (float*)out;
  } else {
    if (p->d_out_bytes < out_bytes) {
      if (p->d_out) { (void)hipFree(p->d_out); p->d_out = nullptr; p->d_out_bytes = 0; }
      HIP_TRY(hipMalloc(&p->d_out, out_bytes));
      p->d_out_bytes = out_bytes;
    }
    *dout = (float*)p->d_out;
  }
  return GCWT_OK;
}

// The launches of one execute: replayed from the plan's graph when the call is the one it was captured from, captured
// when the call comes a second time, else (and from a failed capture on) issued one by one.
static int run_or_replay(gcwt_plan* p, const gcwt_plan::GraphKey& key, bool graphable) {
  const float* dx = (const float*)key.x;
  float* dout = (float*)const_cast<void*>(key.out);
  if (graphable && p->graph_exec && key == p->graph_key) {
    HIP_TRY(hipGraphLaunch(p->graph_exec, p->stream));
    return GCWT_OK;
  }
  if (graphable && p->graph_seen_valid && key == p->graph_seen) {
    if (p->graph_exec) { (void)hipGraphExecDestroy(p->graph_exec); p->graph_exec = nullptr; }
    hipGraph_t graph = nullptr;
    bool ok = hipStreamBeginCapture(p->stream, hipStreamCaptureModeRelaxed) == hipSuccess;
    if (ok) {
      const int rc_cap = run_pipeline(p, dx, dout, key.r0, key.r1, key.row_len, key.reuse);
      const hipError_t he_end = hipStreamEndCapture(p->stream, &graph);
      ok = rc_cap == GCWT_OK && he_end == hipSuccess && graph != nullptr;
      if (ok) ok = hipGraphInstantiate(&p->graph_exec, graph, nullptr, nullptr, 0) == hipSuccess;
      if (graph) (void)hipGraphDestroy(graph);
    }
    if (ok) {
      p->graph_key = key;
      HIP_TRY(hipGraphLaunch(p->graph_exec, p->stream));
      return GCWT_OK;
    }
    // whatever did not capture: this plan runs eagerly from here on
    (void)hipGetLastError();
    p->graph_exec = nullptr;
    p->graph_failed = true;
    p->ev_used = 0;
  }
  p->graph_seen = key;
  p->graph_seen_valid = true;
  const int rc = run_pipeline(p, dx, dout, key.r0, key.r1, key.row_len, key.reuse);
  if (rc) {   // a failure between a fork and its join: nothing may still be running on any of the plan's streams
    (void)hipStreamSynchronize(p->stream);
    for (auto& q : p->aux) (void)hipStreamSynchronize(q);
    if (p->det_stream) (void)hipStreamSynchronize(p->det_stream);
  }
  return rc;
}

// precision = auto / high: read the predictions; auto makes the scales over the threshold again by the exact paths
// (a sub-plan with precision = exact for just those scales; its rows replace the fast path's)
static int apply_verdicts(gcwt_plan* p, const float* dx, float* dout, int64_t r0, int64_t r1, int64_t row_len) {
  const HostPlan& hp = p->hp;
  int rc;
  const size_t n_seg = hp.epochs.size(), Sz = (size_t)hp.prm.n_freqs, Cz = (size_t)hp.prm.n_channels;
  HIP_TRY(hipMemcpyAsync(p->h_pred, p->d_pred, sizeof(float) * Sz * Cz * n_seg, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  // The verdict is per segment (epoch or time block) and channel, so that a block request and the whole transform
  // decide alike for the samples they share.  A segment's scales over the threshold (on any of its flagged
  // channels) are made again for the segment's own core: for every channel when half of them or more are flagged,
  // else for the flagged channels one by one (a one-channel sub-plan: a recording with one bad electrode pays for
  // one); runs of neighbouring segments with the same verdict go in one request.
  std::fill(p->last_pred.begin(), p->last_pred.end(), 0.f);
  struct Verdict {
    std::vector<int32_t> scales, channels;
    bool operator==(const Verdict& o) const { return scales == o.scales && channels == o.channels; }
  };
  std::vector<Verdict> vd(n_seg);
  std::vector<char> any(Sz, 0);
  for (size_t e = 0; e < n_seg; ++e) {
    std::vector<char> sc(Sz, 0);
    for (size_t c = 0; c < Cz; ++c) {
      bool flagged = false;
      for (size_t i = 0; i < Sz; ++i) {
        const float v = p->h_pred[(e * Cz + c) * Sz + i];
        p->last_pred[i] = std::max(p->last_pred[i], v);
        if (v > p->auto_threshold) { sc[i] = 1; any[i] = 1; flagged = true; }
      }
      if (flagged) vd[e].channels.push_back((int32_t)c);
    }
    for (size_t i = 0; i < Sz; ++i)
      if (sc[i]) vd[e].scales.push_back((int32_t)i);
    if (2 * vd[e].channels.size() >= Cz) vd[e].channels.clear();            // empty list with scales: every channel
  }
  p->last_worst = 0.f;
  for (float v : p->last_pred) p->last_worst = std::max(p->last_worst, v);
  p->last_rerouted = 0;
  if (!hp.auto_precision) return GCWT_OK;
  // A scale that cannot be made again -- no device memory for the exact sub-plan or its workspace on a small or busy
  // GPU, a layout the exact paths do not take -- keeps the fast path's row: what precision = high returns, complete
  // and finite.  The execute succeeds, the report says so (a negative count) and gcwt_last_error why.
  bool gave_up = false;
  auto soft = [&](int code) {
    if (code != GCWT_ERR_NOMEM && code != GCWT_ERR_UNSUPPORTED) return false;
    (void)hipGetLastError();
    gave_up = true;
    return true;
  };
  for (size_t e = 0; e < n_seg && !gave_up;) {
    size_t e1 = e + 1;
    if (vd[e].scales.empty()) { e = e1; continue; }
    int64_t a = std::max(hp.epochs[e].core0, r0), b = std::min(hp.epochs[e].core1, r1);
    while (e1 < n_seg && vd[e1] == vd[e] && hp.epochs[e1].core0 >= hp.epochs[e1 - 1].core1) {   // (segments come in time order)
      b = std::min(hp.epochs[e1].core1, r1);
      ++e1;
    }
    if (b > a) {
      if (vd[e].channels.empty()) {
        rc = reroute_scales(p, dx, dout, r0, a, b, row_len, vd[e].scales, -1);
        if (rc && !soft(rc)) return rc;
      } else {
        for (int32_t c : vd[e].channels) {
          rc = reroute_scales(p, dx, dout, r0, a, b, row_len, vd[e].scales, c);
          if (rc && !soft(rc)) return rc;
          if (gave_up) break;
        }
      }
    }
    e = e1;
  }
  for (char c : any) p->last_rerouted += c;
  if (gave_up) p->last_rerouted = -p->last_rerouted;
  return GCWT_OK;
}

// gcwt_timings from the spans of a profiled execute.  A stage's time is the length of the union of its spans (the
// level passes run on three streams beside each other: their sum would count the same wall time up to three times).
static int fill_timings(gcwt_plan* p) {
  float acc[ST_COUNT] = {0};
  if (!p->spans.empty()) {
    const hipEvent_t t0 = p->spans.front().a;
    std::vector<std::pair<float, float>> iv[ST_COUNT];
    float last_end = 0;
    for (const auto& s : p->spans) {
      float a = 0, b = 0;
      HIP_TRY(hipEventElapsedTime(&a, t0, s.a));
      HIP_TRY(hipEventElapsedTime(&b, t0, s.b));
      iv[s.stage].push_back({a, b});
      if (s.stage == ST_INTERP) iv[ST_SYNTH].push_back({a, b});   // synth_ms: every synthesis kernel
      last_end = std::max(last_end, b);
    }
    for (int st = 0; st < ST_COUNT; ++st) {
      std::sort(iv[st].begin(), iv[st].end());
      float lo = 0, hi = -1;
      for (const auto& x : iv[st]) {
        if (hi < lo || x.first > hi) { if (hi >= lo) acc[st] += hi - lo; lo = x.first; hi = x.second; }
        else hi = std::max(hi, x.second);
      }
      if (hi >= lo) acc[st] += hi - lo;
    }
    p->last.total_ms = last_end;
  }
  p->last.mean_ms = acc[ST_MEAN];
  p->last.fwd_fft_ms = acc[ST_FWD];
  p->last.decimate_ms = acc[ST_DECIM];
  p->last.block_fft_ms = acc[ST_BLOCK];
  p->last.synth_ms = acc[ST_SYNTH];
  p->last.interp_ms = acc[ST_INTERP];
  p->last.direct_ms = acc[ST_DIRECT];
  p->last.fullband_ms = acc[ST_FULLBAND];
  p->last.blockconv_ms = acc[ST_BLOCKCONV];
  p->have_timings = true;
  return GCWT_OK;
}

static int execute_range(gcwt_plan* p, const void* x, void* out, int64_t r0, int64_t r1, int flags) {
  if ((flags & GCWT_OUT_F64) && (flags & GCWT_OUT_ON_DEVICE))
    return set_err(GCWT_ERR_INVALID, "GCWT_OUT_F64 applies to host output only");
  int rc = gcwt_plan_upload(p);
  if (rc) return rc;
  if (p->device >= 0) HIP_TRY(hipSetDevice(p->device));
  const HostPlan& hp = p->hp;
  const int64_t n_out = stride_cols(r0, r1, p->out_stride);   // output columns: the samples of [r0, r1) K divides
  const size_t rows = (size_t)hp.prm.n_channels * (size_t)hp.prm.n_freqs;
  if (n_out == 0) return GCWT_OK;                              // a block range between two kept samples
  // host output: dense for the caller, padded to 32 samples on the device so that every
  // row starts on a 128-byte boundary; device output: the caller's pitch (0 = dense)
  int64_t row_len;
  if (flags & GCWT_OUT_ON_DEVICE) {
    row_len = p->row_pitch ? p->row_pitch : n_out;
    if (row_len < n_out) return set_err(GCWT_ERR_INVALID, "row pitch shorter than the output rows");
  } else {
    row_len = (n_out + 31) & ~(int64_t)31;
  }
  const size_t in_bytes = sizeof(float) * (size_t)hp.prm.n_channels * (size_t)hp.prm.n_samples;
  const size_t out_bytes = hp.out_elem_bytes * rows * (size_t)row_len;
  const float* dx;
  float* dout;
  if ((rc = stage_buffers(p, x, out, flags, in_bytes, out_bytes, &dx, &dout))) return rc;
  p->ev_used = 0;
  p->spans.clear();
  if (p->profiling) { p->last = gcwt_timings{}; }
  const bool reuse = (flags & GCWT_REUSE_MEANS) && p->have_means;
  // graph replay: device in and out, nothing to time, no full-band scale (its response cache allocates on the way),
  // and a result small enough for the launches to matter (16 M coefficients)
  const bool graphable = !p->graph_failed && !p->profiling && (flags & GCWT_X_ON_DEVICE) && (flags & GCWT_OUT_ON_DEVICE) &&
                         hp.n_fullband == 0 && p->use_graphs && !p->run_mask &&
                         (int64_t)rows * n_out <= ((int64_t)1 << 24);
  if ((rc = run_or_replay(p, gcwt_plan::GraphKey{dx, dout, r0, r1, row_len, reuse}, graphable))) return rc;
  p->have_means = true;
  if (p->detect && (rc = apply_verdicts(p, dx, dout, r0, r1, row_len))) return rc;
  if (!(flags & GCWT_OUT_ON_DEVICE)) {
    // complex rows are float pairs: the same routine moves (and widens) them
    const size_t k = hp.out_elem_bytes / sizeof(float);
    hipError_t he = p->host_out.drain(dout, k * (size_t)row_len, rows, k * (size_t)n_out, out,
                                      (flags & GCWT_OUT_F64) != 0, p->stream);
    if (he != hipSuccess) {
      return hip_err(he, "host_out.drain");
    }
  }
  HIP_TRY(hipStreamSynchronize(p->stream));
  return p->profiling ? fill_timings(p) : GCWT_OK;
}

static int gcwt_execute_impl(gcwt_plan* p, const void* x, void* out, int flags) {
  if (!p || !x || !out) return set_err(GCWT_ERR_INVALID, "NULL argument");
  return execute_range(p, x, out, 0, p->hp.prm.n_samples, flags & ~GCWT_REUSE_MEANS);
}

static int gcwt_execute_block_impl(gcwt_plan* p, const void* x, void* out, int64_t start, int64_t length,
                       int flags) {
  if (!p || !x || !out) return set_err(GCWT_ERR_INVALID, "NULL argument");
  if (start < 0 || length <= 0 || start + length > p->hp.prm.n_samples)
    return set_err(GCWT_ERR_INVALID, "block range outside the recording");
  return execute_range(p, x, out, start, start + length, flags);
}

int gcwt_plan_segment_count(const gcwt_plan* p) { return p ? (int)p->hp.epochs.size() : -1; }

int gcwt_plan_segment_info(const gcwt_plan* p, int segment, int64_t* core_start, int64_t* core_stop,
                           int64_t* fft_length) {
  if (!p) return set_err(GCWT_ERR_INVALID, "NULL plan");
  if (segment < 0 || segment >= (int)p->hp.epochs.size())
    return set_err(GCWT_ERR_INVALID, "segment out of range");
  const EpochPlan& ep = p->hp.epochs[segment];
  if (core_start) *core_start = ep.core0;
  if (core_stop) *core_stop = ep.core1;
  if (fft_length) *fft_length = ep.p;
  return GCWT_OK;
}

int gcwt_filter_bank(gcwt_plan* p, float* bank) {
  if (!p || !bank) return set_err(GCWT_ERR_INVALID, "NULL argument");
  int rc = gcwt_plan_upload(p);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(bank, p->d_bank, sizeof(float2) * (size_t)p->hp.prm.n_freqs * p->hp.block,
                    hipMemcpyDeviceToHost));
  return GCWT_OK;
}

int gcwt_direct_kernel(gcwt_plan* p, int scale, float* psi) {
  if (!p || !psi) return set_err(GCWT_ERR_INVALID, "NULL argument");
  if (scale < 0 || scale >= p->hp.prm.n_freqs) return set_err(GCWT_ERR_INVALID, "scale out of range");
  const ScalePlan& s = p->hp.scales[scale];
  if (s.method != GCWT_SCALE_DIRECT) return set_err(GCWT_ERR_INVALID, "not a direct scale");
  int rc = gcwt_plan_upload(p);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(psi, p->d_psi_lit + s.direct_offset + direct_front_pad(s.length), sizeof(float2) * (size_t)s.length,
                    hipMemcpyDeviceToHost));
  return GCWT_OK;
}

int gcwt_plan_precision_report(const gcwt_plan* p, float* predicted, float* worst, int32_t* n_rerouted) {
  if (!p) return set_err(GCWT_ERR_INVALID, "NULL plan");
  const size_t S = (size_t)p->hp.prm.n_freqs;
  if (predicted)
    for (size_t i = 0; i < S; ++i) predicted[i] = i < p->last_pred.size() ? p->last_pred[i] : 0.f;
  if (worst) *worst = p->last_worst;
  if (n_rerouted) *n_rerouted = p->last_rerouted;
  return GCWT_OK;
}

// test hook: the two terms of the prediction (rounding of the level's stages; what the level leaves out) of workspace
// slot 0 of the last batch the last execute ran, S floats each, and the level energies (n_levels floats, may be NULL)
int gcwt_debug_precision_terms(gcwt_plan* p, float* rounding, float* left_out, float* level_energy, float* band_energy) {
  if (!p || !rounding || !left_out) return set_err(GCWT_ERR_INVALID, "NULL argument");
  if (!p->detect || p->last_batch_slots <= 0) return set_err(GCWT_ERR_INVALID, "no execute with the detector on yet");
  const int S = p->hp.prm.n_freqs, L = (int)p->hp.levels.size();
  // scratch predictions: the kernel writes pred[(segment, channel, scale)] -- every slot's segment is 0 here, so C rows of S
  struct Scratch {
    float* p = nullptr;
    ~Scratch() { if (p) (void)hipFree(p); }
  } sc, lv, pr;
  const size_t Cn = (size_t)p->hp.prm.n_channels;
  HIP_TRY(hipMalloc((void**)&sc.p, sizeof(float) * 2 * (size_t)S * p->last_batch_slots));
  HIP_TRY(hipMalloc((void**)&lv.p, sizeof(float) * (size_t)L * p->last_batch_slots));
  HIP_TRY(hipMalloc((void**)&pr.p, sizeof(float) * (size_t)S * Cn));
  PredSegs dbg_segs{};
  dbg_segs.n_channels = p->hp.prm.n_channels;
  // the kernel writes the terms of the scales on a decimated level and the energies of levels that have one: the rest
  // must read as zero, not as whatever the allocation held
  hipError_t he = hipMemsetAsync(sc.p, 0, sizeof(float) * 2 * (size_t)S * p->last_batch_slots, p->stream);
  if (he == hipSuccess) he = hipMemsetAsync(lv.p, 0, sizeof(float) * (size_t)L * p->last_batch_slots, p->stream);
  if (he == hipSuccess)
    he = launch_precision_predict(p->d_bands, p->d_gain, p->d_scale_level, p->d_scale_length, p->ep_dev[p->last_batch].pred_levels, S, L,
                                           p->last_pt, p->kappa_eps, p->oob_tol, pr.p, lv.p, sc.p, p->last_batch_slots, dbg_segs, p->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(rounding, sc.p, sizeof(float) * (size_t)S, hipMemcpyDeviceToHost, p->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(left_out, sc.p + S, sizeof(float) * (size_t)S, hipMemcpyDeviceToHost, p->stream);
  if (he == hipSuccess && level_energy) he = hipMemcpyAsync(level_energy, lv.p, sizeof(float) * (size_t)L, hipMemcpyDeviceToHost, p->stream);
  if (he == hipSuccess && band_energy) he = hipMemcpyAsync(band_energy, p->d_bands, sizeof(float) * (size_t)kSpecBands, hipMemcpyDeviceToHost, p->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(p->stream);
  if (he != hipSuccess) return hip_err(he, "precision terms");
  return GCWT_OK;
}

int gcwt_get_timings(const gcwt_plan* p, gcwt_timings* t) {
  if (!p || !t) return set_err(GCWT_ERR_INVALID, "NULL argument");
  if (!p->have_timings) return set_err(GCWT_ERR_INVALID, "no profiled execute yet");
  *t = p->last;
  return GCWT_OK;
}

// ---- exception-safe entry points ------------------------------------------
int gcwt_plan_create(gcwt_plan** out, const gcwt_params* params) {
  return guarded([&] { return gcwt_plan_create_impl(out, params); });
}

int gcwt_plan_upload(gcwt_plan* p) {
  return guarded([&] { return gcwt_plan_upload_impl(p); });
}

int gcwt_execute(gcwt_plan* p, const void* x, void* out, int flags) {
  return guarded([&] { return gcwt_execute_impl(p, x, out, flags); });
}

int gcwt_execute_block(gcwt_plan* p, const void* x, void* out, int64_t start, int64_t length,
                       int flags) {
  return guarded([&] { return gcwt_execute_block_impl(p, x, out, start, length, flags); });
}


// ---- debug hooks (include/ghostcwt_debug.h) --------------------------------
int gcwt_debug_measure_build(void) { return kMeasureBuild ? 1 : 0; }

int gcwt_debug_level_count(const gcwt_plan* p) { return p ? (int)p->hp.levels.size() : -1; }

int gcwt_debug_level_info(const gcwt_plan* p, int epoch, int level, int32_t* decimation,
                          int32_t* halo, int32_t* hop, int32_t* nblk, int64_t* m) {
  if (!p) return set_err(GCWT_ERR_INVALID, "NULL plan");
  if (epoch < 0 || epoch >= (int)p->hp.epochs.size() || level < 0 ||
      level >= (int)p->hp.levels.size())
    return set_err(GCWT_ERR_INVALID, "epoch/level out of range");
  const LevelPlan& lp = p->hp.levels[level];
  const EpochLevel& el = p->hp.epochs[epoch].lv[level];
  if (decimation) *decimation = lp.decimation;
  if (halo) *halo = lp.halo;
  if (hop) *hop = lp.hop;
  if (nblk) *nblk = el.nblk;
  if (m) *m = el.m;
  return GCWT_OK;
}

int gcwt_debug_level_band_shift(const gcwt_plan* p, int level, int32_t* shift) {
  if (!p || !shift) return set_err(GCWT_ERR_INVALID, "NULL argument");
  if (level < 0 || level >= (int)p->hp.levels.size()) return set_err(GCWT_ERR_INVALID, "level out of range");
  *shift = p->hp.levels[level].band_shift;
  return GCWT_OK;
}

int gcwt_debug_set_option(const char* name, int64_t value, int clear) {
  const int rc = option_set(name, (long long)value, clear != 0);
  if (rc == -1) return set_err(GCWT_ERR_INVALID, std::string("unknown option: ") + (name ? name : "(null)"));
  if (rc == -2) return set_err(GCWT_ERR_UNSUPPORTED, std::string("option ") + name + " exists in libghostcwt_measure.so only");
  return GCWT_OK;
}

int gcwt_debug_level_low_cut(const gcwt_plan* p, int level, double* theta_cut) {
  if (!p || !theta_cut) return set_err(GCWT_ERR_INVALID, "NULL argument");
  if (level < 0 || level >= (int)p->hp.levels.size()) return set_err(GCWT_ERR_INVALID, "level out of range");
  const LevelPlan& own = p->hp.levels[p->hp.levels[level].xr_owner];
  *theta_cut = p->hp.high_precision && own.band_shift == 0 ? own.taper_hi : 0.0;
  return GCWT_OK;
}

int gcwt_debug_scale_theta_lo(const gcwt_plan* p, double* theta_lo) {
  if (!p || !theta_lo) return set_err(GCWT_ERR_INVALID, "NULL argument");
  for (size_t i = 0; i < p->hp.scales.size(); ++i) theta_lo[i] = p->hp.scales[i].theta_lo;
  return GCWT_OK;
}

int gcwt_debug_mean_folded(const gcwt_plan* p) {
  if (!p) return set_err(GCWT_ERR_INVALID, "NULL plan");
  return p->last_fold ? 1 : 0;
}

int gcwt_debug_graph_state(const gcwt_plan* p) {
  if (!p) return set_err(GCWT_ERR_INVALID, "NULL plan");
  return p->graph_failed ? -1 : p->graph_exec ? 1 : 0;
}

int gcwt_debug_blockconv_groups(const gcwt_plan* p, int32_t* first, int32_t* count, int32_t* hop, int32_t* back,
                                int32_t* order, int max_groups, int max_order) {
  if (!p) return set_err(GCWT_ERR_INVALID, "NULL plan");
  const HostPlan& hp = p->hp;
  const int n = (int)hp.bc_groups.size();
  for (int g = 0; g < n && g < max_groups; ++g) {
    if (first) first[g] = hp.bc_groups[g].first;
    if (count) count[g] = hp.bc_groups[g].count;
    if (hop) hop[g] = hp.bc_groups[g].hop;
    if (back) back[g] = hp.bc_groups[g].back;
  }
  if (order) for (int k = 0; k < hp.n_blockconv && k < max_order; ++k) order[k] = hp.bc_order[k];
  return n;
}

int gcwt_debug_interp_level(const gcwt_plan* p, int level, int32_t* q, int32_t* factor, double* alpha,
                            double* err_bound, float* coef, int64_t max_floats) {
  if (!p) return set_err(GCWT_ERR_INVALID, "NULL plan");
  if (level < 0 || level >= (int)p->hp.levels.size()) return set_err(GCWT_ERR_INVALID, "level out of range");
  const LevelPlan& lp = p->hp.levels[level];
  const bool on = level_kernel(p, lp) == LK_INTERP;
  if (q) *q = on ? lp.interp_q : 0;
  if (factor) *factor = on ? lp.interp_factor : 0;
  if (alpha) *alpha = lp.interp_alpha;
  if (err_bound) *err_bound = lp.interp_err;
  if (coef && on) {
    const int64_t n = (int64_t)2 * lp.interp_factor * 8;
    if (n > max_floats) return set_err(GCWT_ERR_INVALID, "destination too small");
    memcpy(coef, p->hp.interp_coef.data() + lp.coef_offset, sizeof(float) * (size_t)n);
  }
  return GCWT_OK;
}

int gcwt_debug_scale_demod(const gcwt_plan* p, int32_t* demod) {
  if (!p || !demod) return set_err(GCWT_ERR_INVALID, "NULL argument");
  for (size_t i = 0; i < p->hp.scales.size(); ++i) demod[i] = p->hp.scales[i].demod_bin;
  return GCWT_OK;
}

int gcwt_debug_scale_theta_neg(const gcwt_plan* p, double* theta_neg) {
  if (!p || !theta_neg) return set_err(GCWT_ERR_INVALID, "NULL argument");
  for (size_t i = 0; i < p->hp.scales.size(); ++i) theta_neg[i] = p->hp.scales[i].theta_neg;
  return GCWT_OK;
}

int gcwt_debug_batch_of(const gcwt_plan* p, int segment, int32_t* first, int32_t* count) {
  if (!p) return set_err(GCWT_ERR_INVALID, "NULL plan");
  if (segment < 0 || segment >= (int)p->hp.epochs.size())
    return set_err(GCWT_ERR_INVALID, "segment out of range");
  const int f = p->hp.epochs[segment].batch_first;
  if (first) *first = f;
  if (count) *count = p->hp.epochs[f].batch_count;
  return GCWT_OK;
}

int gcwt_debug_scale_lists(gcwt_plan* p, int32_t* level_first, int32_t* level_plain, int32_t* row, int32_t* j_hi,
                           int32_t max_entries) {
  if (!p) return set_err(GCWT_ERR_INVALID, "NULL plan");
  ScaleLists sl = level_scale_lists(p->hp);
  std::vector<int32_t>& list = sl.list;
  const std::vector<int>&first = sl.scale_off, &plain = sl.n_plain;
  const int n = (int)list.size();
  for (size_t l = 0; l < first.size(); ++l) {
    if (level_first) level_first[l] = first[l];
    if (level_plain) level_plain[l] = plain[l];
  }
  if (level_first) level_first[first.size()] = n;
  if (n > max_entries || (!row && !j_hi)) return n;
  const bool on_device = p->uploaded && p->d_scale_list && p->n_listed == n;
  if (on_device && n > 0) {                 // the entries as the kernels read them: k_scale_windows has set the top bytes
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipMemcpy(list.data(), p->d_scale_list, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < n; ++i) {
    if (row) row[i] = list[i] & kScaleIndexMask;
    if (j_hi) j_hi[i] = on_device ? 16 - (int32_t)((uint32_t)list[i] >> 24) : 0;
  }
  return n;
}

int gcwt_debug_work_items(const gcwt_plan* p, int kernel, int batch, int32_t* out, int32_t max_ints) {
  if (!p) return set_err(GCWT_ERR_INVALID, "NULL plan");
  const HostPlan& hp = p->hp;
  size_t e = 0;                               // the batch's first segment
  for (int b = 0; e < hp.epochs.size() && b < batch; ++b) e += (size_t)std::max(1, hp.epochs[e].batch_count);
  if (batch < 0 || e >= hp.epochs.size()) return set_err(GCWT_ERR_INVALID, "batch out of range");
  const EpochPlan& ep = hp.epochs[e];
  const ScaleLists sl = level_scale_lists(hp);
  std::vector<int32_t> flat;
  auto put = [&](const auto& items) {         // every item type is a record of int32 fields
    const int32_t* q = reinterpret_cast<const int32_t*>(items.data());
    flat.insert(flat.end(), q, q + items.size() * (sizeof(items[0]) / sizeof(int32_t)));
  };
  if (kernel == GCWT_DEBUG_ITEMS_SYNTH16) {
    put(synth16_items(p, ep).items);
  } else if (kernel == GCWT_DEBUG_ITEMS_SYNTH7 || kernel == GCWT_DEBUG_ITEMS_SYNTH7_WIDE || kernel == GCWT_DEBUG_ITEMS_SYNTH7_NARROW) {
    const Synth7Items s7 = synth7_items(p, ep, sl);
    put(kernel == GCWT_DEBUG_ITEMS_SYNTH7 ? s7.items : kernel == GCWT_DEBUG_ITEMS_SYNTH7_WIDE ? s7.wide : s7.narrow);
  } else if (kernel == GCWT_DEBUG_ITEMS_INTERP) {
    SynthiItems si;
    const int rc = synthi_items(p, ep, sl, &si);
    if (rc) return rc;
    flat.push_back(si.split);
    put(si.items);
  } else if (kernel == GCWT_DEBUG_ITEMS_PIPELINED) {
    SynthpItems sp;
    const int rc = synthp_items(p, ep, sl, &sp);
    if (rc) return rc;
    flat.push_back((int32_t)sp.items[0].size());
    put(sp.items[0]);
    put(sp.items[1]);
  } else {
    return set_err(GCWT_ERR_INVALID, "unknown kernel");
  }
  if (out && (int64_t)flat.size() <= max_ints) std::copy(flat.begin(), flat.end(), out);
  return (int)flat.size();
}

int gcwt_debug_exact_gain(const gcwt_plan* p, int scale, const int64_t* a, int64_t b, int64_t n,
                          double* gain) {
  if (!p || !a || !gain || b <= 0) return set_err(GCWT_ERR_INVALID, "bad argument");
  if (scale < 0 || scale >= (int)p->hp.scales.size()) return set_err(GCWT_ERR_INVALID, "scale out of range");
  const ScalePlan& s = p->hp.scales[scale];
  for (int64_t i = 0; i < n; ++i) {
    if (p->hp.morlet) {           // |H| of the closed form (its k = 0 term, real and positive, inside a scale's band)
      double hr, hi;
      morlet_response(p->hp.prm.gamma, s.sigma, s.half_delay, a[i], b, &hr, &hi);
      gain[i] = std::sqrt(hr * hr + hi * hi);
      continue;
    }
    gain[i] = exact_gain(p->hp.amps.data() + s.amp_offset, s.bin_lo, s.n_bins, s.length, a[i], b);
  }
  return GCWT_OK;
}

int gcwt_debug_clock(gcwt_plan* p, double* ghz, double* workgroup_seconds) {
  if (!p || !ghz) return set_err(GCWT_ERR_INVALID, "NULL argument");
  if (!p->d_probe)
    return set_err(GCWT_ERR_INVALID, kMeasureBuild ? "plan was not created with GHOSTCWT_CLOCK_PROBE=1"
                                                   : "the clock probe exists only in libghostcwt_measure.so (make measure)");
  unsigned long long v[8] = {};
  HIP_TRY(hipMemcpy(v, p->d_probe, sizeof(v), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(p->d_probe, 0, sizeof(v)));
  *ghz = v[1] ? (double)v[0] / (double)v[1] * 0.1 : 0.0;
  if (workgroup_seconds) *workgroup_seconds = (double)v[1] * 1e-8;
  if (kMeasureBuild && option_is_set("clock_phases") && v[6])   // mean microseconds into a k_synth7 workgroup's life at its marks
    fprintf(stderr, "k_synth7 workgroups %llu: loads parked %.2f us, spectra exchanged %.2f, spectra done %.2f, loop starts %.2f, ends %.2f\n",
            v[6], v[2] * 0.01 / v[6], v[3] * 0.01 / v[6], v[4] * 0.01 / v[6], v[5] * 0.01 / v[6], v[1] * 0.01 / v[6]);
  return GCWT_OK;
}

int gcwt_debug_fetch(gcwt_plan* p, int what, int channel, int epoch, int level, float* dst,
                     int64_t max_complex) {
  if (!p || !dst) return set_err(GCWT_ERR_INVALID, "NULL argument");
  if (!p->uploaded) return set_err(GCWT_ERR_INVALID, "plan has not run");
  const HostPlan& hp = p->hp;
  if (epoch < 0 || epoch >= (int)hp.epochs.size() || channel < 0 || channel >= hp.prm.n_channels)
    return set_err(GCWT_ERR_INVALID, "epoch/channel out of range");
  const EpochPlan& ep = hp.epochs[epoch];
  // workspace slot of (segment, channel) after a full execute: position in its batch
  const int64_t slot = (int64_t)(epoch - ep.batch_first) * hp.prm.n_channels + channel;
  const float2* src = nullptr;
  int64_t n = 0;
  if (what == GCWT_DEBUG_SPECTRUM) {
    src = p->d_x + slot * ep.p_store;
    n = ep.p_store;
  } else {
    if (level < 0 || level >= (int)hp.levels.size()) return set_err(GCWT_ERR_INVALID, "level out of range");
    if (what == GCWT_DEBUG_DECIMATED) {
      src = p->d_xr + slot * hp.max_xr + ep.lv[level].xr_offset;
      n = ep.lv[level].m;
    } else if (what == GCWT_DEBUG_BLOCK_SPECTRA) {
      src = p->d_xb + slot * hp.max_xb + ep.lv[level].xb_offset;
      n = (int64_t)ep.lv[level].nblk * hp.block;
    } else {
      return set_err(GCWT_ERR_INVALID, "unknown buffer");
    }
  }
  if (n > max_complex) return set_err(GCWT_ERR_INVALID, "destination too small");
  HIP_TRY(hipMemcpy(dst, src, sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost));
  return (int)0;
}

}  // extern "C"

// accessors for comm.cpp
int gcwt_internal_refresh_bank(gcwt_plan* p) {   // derived tables follow a (broadcast) bank
  hipError_t he = launch_bank_gain(p->d_bank, p->d_gain, p->d_bank_sc, p->hp.prm.n_freqs, p->stream);
  if (he != hipSuccess) return hip_err(he, "bank_gain");
  he = launch_scale_windows(p->d_gain, p->d_scale_list, p->n_listed, (float)p->hp.band_tol, p->d_gain_lv,
                            p->prune_inputs, p->stream);
  if (he != hipSuccess) return hip_err(he, "scale_windows");
  if (p->hp.morlet) {
    he = launch_gain_rows_complex(p->d_bank, p->d_scale_list, p->n_listed, reinterpret_cast<float2*>(p->d_gain_lv), p->stream);
    if (he != hipSuccess) return hip_err(he, "gain_rows_complex");
  }
  return GCWT_OK;
}
int gcwt_internal_set_error(int code, const char* msg) { return set_err(code, msg); }
