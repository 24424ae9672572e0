// work_items.cpp -- the work-item cuts of the synthesis kernels (work_items.h).
#include "work_items.h"

#include <algorithm>
#include <cmath>

#include "interp.h"

namespace gcwt {

bool level_pipelined(const gcwt_plan* p, const LevelPlan& lp) {
  return p->use_synthp && lp.interp_q == 2 && lp.interp_factor >= 4 && lp.interp_factor <= kSynthpMaxFactor &&
         lp.scales.size() <= 256;
}
LevelKernel level_kernel(const gcwt_plan* p, const LevelPlan& lp) {
  // (the 16-column kernel knows nothing of a band shift: shifted levels keep k_synth7 whatever the option says)
  if (p->use_synth16 && lp.band_shift == 0) return LK_SYNTH16;
  if (lp.interp_q > 0) return LK_INTERP;
  // (a shifted band is built into k_synth7 and k_synthi only; k_synth7<WIDE> takes its long halos)
  return lp.fast || (lp.band_shift > 0 && lp.scales.size() <= 256) ? LK_SYNTH7 : LK_SYNTH16;
}

ScaleLists level_scale_lists(const HostPlan& hp) {
  ScaleLists sl;
  sl.scale_off.assign(hp.levels.size(), 0);
  sl.n_plain.assign(hp.levels.size(), 0);
  for (size_t l = 0; l < hp.levels.size(); ++l) {
    sl.scale_off[l] = (int)sl.list.size();
    for (int sidx : hp.levels[l].scales)
      if (hp.morlet || hp.scales[sidx].half_delay == 0.0) sl.list.push_back(sidx);
    sl.n_plain[l] = (int)sl.list.size() - sl.scale_off[l];
    for (int sidx : hp.levels[l].scales)
      if (!hp.morlet && hp.scales[sidx].half_delay != 0.0) sl.list.push_back(sidx);
  }
  return sl;
}

std::vector<float2> half_twiddles(const HostPlan& hp) {
  std::vector<float2> half_tw(hp.levels.size() * 256);
  for (size_t l = 0; l < hp.levels.size(); ++l) {
    for (int k = 0; k < 256; ++k) {
      const double a = -M_PI * (k - hp.levels[l].band_shift) / (256.0 * hp.levels[l].decimation);
      half_tw[l * 256 + k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
  }
  return half_tw;
}

std::vector<int32_t> scale_aux(const HostPlan& hp, const std::vector<int32_t>& list) {
  std::vector<int32_t> aux;
  for (int sidx : list)
    aux.push_back(hp.scales[sidx].demod_bin | (!hp.morlet && hp.scales[sidx].half_delay != 0.0 ? 1 << 16 : 0));
  return aux;
}

// each level goes to the production kernel when its layout allows (16 <= halo <= 32, at
// most 256 scales), else to the 16-column kernel; GHOSTCWT_SYNTH16=1 sends everything there
Synth16Items synth16_items(const gcwt_plan* p, const EpochPlan& ep) {
  const HostPlan& hp = p->hp;
  Synth16Items out;
  for (size_t i = 0; i < ep.items.size(); ++i)
    if (level_kernel(p, hp.levels[ep.items[i].level]) == LK_SYNTH16)
      out.items.push_back({ep.items[i].level, ep.items[i].scale, ep.items[i].blk0, ep.items[i].nblk});
  out.levels.resize(hp.levels.size());
  for (size_t l = 0; l < out.levels.size(); ++l)
    out.levels[l] = {hp.levels[l].decimation, hp.levels[l].hop, hp.levels[l].halo, ep.lv[l].blk_lo,
                     ep.lv[l].xb_offset, hp.levels[l].twiddle_offset};
  return out;
}

Synth7Items synth7_items(const gcwt_plan* p, const EpochPlan& ep, const ScaleLists& sl) {
  const HostPlan& hp = p->hp;
  Synth7Items out;
  out.levels.resize(hp.levels.size());
  for (size_t l = 0; l < out.levels.size(); ++l) {
    const LevelPlan& lp = hp.levels[l];
    int lg = 0;
    while ((1 << lg) < lp.decimation) ++lg;
    out.levels[l] = {lp.decimation, lg, lp.hop, lp.halo, ep.lv[l].nblk, (int32_t)lp.scales.size(),
                     sl.scale_off[l], ep.lv[l].blk_lo, sl.n_plain[l], (int32_t)(l * 256), lp.band_shift, 0, ep.lv[l].xb_offset,
                     lp.twiddle_offset, ep.lv[l].xr_offset, ep.lv[l].m - 1};
    const bool narrow = lp.halo <= 48 && lp.decimation <= p->synth7_narrow_r && p->synth_cols == 32;
    const int cols = narrow ? 16 : p->synth_cols;
    const int bpb = std::max(1, cols / lp.decimation);
    const int n_rtiles = std::max(1, lp.decimation / cols);
    if (level_kernel(p, lp) != LK_SYNTH7) continue;
    for (int b0 = 0; b0 < ep.lv[l].nblk; b0 += bpb)
      for (int rt = 0; rt < n_rtiles; ++rt) (lp.halo > 48 ? out.wide : narrow ? out.narrow : out.items).push_back({(int32_t)l, b0, rt, 0});
  }
  // order of the k_synth7 items (option synth7_order, A/B runs): 0 as listed (levels in plan order, R = 2 first),
  // 1 reversed, 2 the levels' items dealt in turn
  if (p->synth7_order == 1) std::reverse(out.items.begin(), out.items.end());
  else if (p->synth7_order == 2) {
    std::vector<std::vector<Synth7Item>> by(hp.levels.size());
    for (const auto& it : out.items) by[(size_t)it.level].push_back(it);
    std::vector<Synth7Item> mixed;
    std::vector<double> pos(by.size(), 0.0);
    size_t left = out.items.size();
    while (left) {                                   // always the level that is furthest behind its share
      size_t best = by.size(); double frac = 2.0;
      for (size_t l = 0; l < by.size(); ++l)
        if (pos[l] < (double)by[l].size() && pos[l] / (double)by[l].size() < frac) { frac = pos[l] / (double)by[l].size(); best = l; }
      mixed.push_back(by[best][(size_t)pos[best]]);
      pos[best] += 1.0; --left;
    }
    out.items.swap(mixed);
  }
  return out;
}

namespace {

// the interpolated levels of a plan that `pipelined` or the plain interpolating kernel takes, the longest-running
// (largest R) first
std::vector<int> interp_levels(const gcwt_plan* p, bool pipelined) {
  const HostPlan& hp = p->hp;
  std::vector<int> order;
  for (size_t l = 0; l < hp.levels.size(); ++l)
    if (level_kernel(p, hp.levels[l]) == LK_INTERP && level_pipelined(p, hp.levels[l]) == pipelined) order.push_back((int)l);
  std::sort(order.begin(), order.end(), [&](int x, int y) { return hp.levels[x].decimation > hp.levels[y].decimation; });
  return order;
}

// The cut both interpolating kernels share.  `cut(target, emit)` lists the items of a launch when a run of passes
// (rounds) is cut at `target` output bytes, calling emit(item, its bytes, its group) for each; `target` is halved
// until the launch has `enough` workgroups -- a few rounds of them per CU -- over the batch's channel slots, or is
// down to 512 KiB, or after seven halvings.  The list is then ordered group 0 before group 1, each largest first, so
// that what is still running when a launch ends is the small items.  Returns the number of items of group 0.
template <typename Item, typename Cut>
int cut_largest_first(int64_t n_ch_slots, int64_t enough, Cut cut, std::vector<Item>* items) {
  std::vector<int64_t> bytes;
  std::vector<char> group;
  auto emit = [&](const Item& it, int64_t b, int g) { items->push_back(it); bytes.push_back(b); group.push_back((char)g); };
  int64_t target = (int64_t)2 << 20;
  for (int attempt = 0;; ++attempt) {
    items->clear();
    bytes.clear();
    group.clear();
    cut(target, emit);
    if ((int64_t)items->size() * n_ch_slots >= enough || target <= ((int64_t)1 << 19) || attempt > 6) break;
    target >>= 1;
  }
  std::vector<size_t> order(items->size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) {
    return group[x] != group[y] ? group[x] < group[y] : bytes[x] > bytes[y];
  });
  std::vector<Item> sorted(items->size());
  for (size_t i = 0; i < order.size(); ++i) sorted[i] = (*items)[order[i]];
  items->swap(sorted);
  return (int)std::count(group.begin(), group.end(), (char)0);
}

}  // namespace

// interpolated levels: one workgroup per block, the longest-running (largest R) first
int synthi_items(const gcwt_plan* p, const EpochPlan& ep, const ScaleLists& sl, SynthiItems* out) {
  const HostPlan& hp = p->hp;
  std::vector<std::pair<int, int>> pending;          // (level, log2 blocks per workgroup)
  out->levels.assign(hp.levels.size(), SynthiLevel{});
  for (int l : interp_levels(p, false)) {
    const LevelPlan& lp = hp.levels[l];
    int lgq = 0;
    while ((1 << lgq) < lp.interp_q) ++lgq;
    // Blocks per workgroup: a workgroup's prologue (its blocks' spectra, 16 threads each) takes
    // about as long whatever their number, and a block of a low decimation is little work:
    // two blocks per workgroup up to R = 32, one from R = 64 up (measured per level,
    // profiles/r03_synth_study.md; the 16 columns of a pass are blocks x scales x phases) -- with two phases per scale;
    // with four (R >= 32 since round 5) two blocks leave two scales per pass and one block is the better cut (R = 32:
    // 1.56 against 1.63 - 1.66 ms)
    int lgnb = lp.decimation <= 32 && lp.interp_q <= 2 ? 1 : 0;
    if (p->interp_lgnb >= 0) lgnb = std::min(p->interp_lgnb, 2);
    while (lgnb > 0 && (lp.interp_q << lgnb) > kInterpMaxPhases) --lgnb;
    // what k_synthi's indexing assumes (synthi.hip); the planner guarantees it
    if (lp.interp_q < 2 || lp.interp_q > kInterpMaxPhases || (lp.interp_q & (lp.interp_q - 1)) ||
        lp.interp_factor * lp.interp_q != lp.decimation || lp.interp_factor < 4 ||
        lp.interp_factor > kInterpMaxFactor || lp.scales.size() > 256 || lp.halo < 16 ||
        lp.hop != hp.block - 2 * lp.halo || lp.hop < 1 || hp.block != 256 || (lp.interp_taps != 6 && lp.interp_taps != 8))
      return set_err(GCWT_ERR_INVALID, "internal: interpolated level outside the kernel's limits");
    out->levels[l] = {lp.decimation, lp.interp_q, lgq, lp.interp_factor, lp.hop, lp.halo, ep.lv[l].nblk,
                      (int32_t)lp.scales.size(), sl.scale_off[l], ep.lv[l].blk_lo, lgnb, lp.interp_taps, lp.twiddle_offset,
                      ep.lv[l].xr_offset, ep.lv[l].m - 1, lp.coef_offset};
    pending.push_back({l, lgnb});
  }
  // A workgroup walks all the scales of its blocks unless that is too much for one: the passes
  // of a level's walk (kInterpCols / (q nb) scales each) are cut into runs of at most
  // `target` output bytes, and where a single pass is more than that (high decimations: one
  // pass of two scales of a block is 14 MB at R = 8192) its wave-tasks are shared out over
  // several workgroups, each of which repeats the pass's transforms (17 q / R of the work).
  // `target` is halved until the launch has a few rounds of workgroups per CU.  The list is
  // ordered largest first, so that what is still running when the launch ends is the small items.  A run's prologue -- its blocks' spectra -- costs ~8 us.
  // One array in two parts, the levels below interp_split_r first, each part largest first; the parts are a
  // launch each (pipeline.cpp: interp_launches).  interp_split_r = 0: the first part is empty, one list, one launch.
  const int64_t n_ch_slots = (int64_t)hp.prm.n_channels * std::max(1, ep.batch_count);
  out->split = cut_largest_first(n_ch_slots, 3072, [&](int64_t target, auto& emit) {
    for (const auto& pl : pending) {
      const LevelPlan& lp = hp.levels[pl.first];
      const int nb = 1 << pl.second, ns = kInterpCols / (lp.interp_q * nb);
      const int n_pass = ((int)lp.scales.size() + ns - 1) / ns;
      const int64_t pass_bytes = (int64_t)ns * nb * lp.hop * lp.decimation * 4;
      const int run = (int)std::max<int64_t>(1, std::min<int64_t>(n_pass, target / std::max<int64_t>(1, pass_bytes)));
      const int wps = (lp.hop * (lp.decimation >> 2) + 63) >> 6;     // wave-tasks per (block, scale): synthi.hip
      const int quads = (wps + 3) / 4;
      const int parts = run > 1 ? 1 : (int)std::min<int64_t>(quads, (pass_bytes + target - 1) / target);
      const int late = lp.decimation >= p->interp_split_r;
      for (int b0 = 0; b0 < ep.lv[pl.first].nblk; b0 += nb)
        for (int p0 = 0; p0 < n_pass; p0 += run)
          for (int part = 0; part < parts; ++part) {
            const int lo = 4 * (int)((int64_t)quads * part / parts);
            const int hi = std::min(wps, 4 * (int)((int64_t)quads * (part + 1) / parts));
            const int np = std::min(run, n_pass - p0);
            emit(SynthiItem{(int32_t)pl.first, b0, p0, np, lo, hi}, (int64_t)np * pass_bytes * (hi - lo) / std::max(1, wps), late);
          }
    }
  }, &out->items);
  return GCWT_OK;
}

// pipelined kernel: a workgroup owns nb consecutive blocks and walks the level's scales 4 / nb at a time (a
// round: 8 columns, 4 z slots).  Blocks per workgroup by decimation, so that a (round, scale) run is at least a
// few dozen wave-tasks of 256 samples for the six consumer waves: four blocks up to R = 16, two at R = 32, one
// beyond.  A run of rounds is cut at `target` bytes of rows like k_synthi's passes; largest items first.
int synthp_items(const gcwt_plan* p, const EpochPlan& ep, const ScaleLists& sl, SynthpItems* out) {
  const HostPlan& hp = p->hp;
  const std::vector<int> order_p = interp_levels(p, true);
  std::vector<SynthpLevel>& lvp = out->levels;
  lvp.assign(hp.levels.size(), SynthpLevel{});
  for (int l : order_p) {
    const LevelPlan& lp = hp.levels[l];
    int lgnb = lp.decimation <= 16 ? 2 : lp.decimation <= 32 ? 1 : 0;
    if (p->synthp_lgnb >= 0) lgnb = std::min(p->synthp_lgnb, 2);
    if (lp.interp_factor * 2 != lp.decimation || lp.halo < 16 || lp.hop != hp.block - 2 * lp.halo || lp.hop < 1 ||
        hp.block != 256 || (lp.hop * lp.decimation) % (4 * lp.interp_factor) != 0)
      return set_err(GCWT_ERR_INVALID, "internal: pipelined level outside the kernel's limits");
    // what the two producer waves take of a round's tasks after making the next round's z (about 4.5 tasks' worth
    // of instructions each): all eight waves done together when (T - h) / 6 = 4.5 + h / 2
    const double tasks = 4.0 * lp.hop * lp.decimation / 256.0;
    int help = (int)std::lround(128.0 * std::max(0.0, (tasks - 27.0) / (4.0 * tasks)));
    if (p->synthp_help >= 0) help = std::min(p->synthp_help, 64);
    lvp[l] = {lp.decimation, lp.interp_factor, lp.hop, lp.halo, ep.lv[l].nblk, (int32_t)lp.scales.size(),
              sl.scale_off[l], ep.lv[l].blk_lo, lgnb, sl.n_plain[l], (int32_t)(l * 256), help, lp.twiddle_offset,
              ep.lv[l].xr_offset, ep.lv[l].m - 1, lp.coef_offset};
  }
  const int64_t n_ch_slots = (int64_t)hp.prm.n_channels * std::max(1, ep.batch_count);
  std::vector<SynthpItem> all;                 // the levels with I > 4 (group 0), then those with I = 4: a launch each
  const int n0 = cut_largest_first(n_ch_slots, 2048, [&](int64_t target, auto& emit) {
    for (int l : order_p) {
      const LevelPlan& lp = hp.levels[l];
      const int nb = 1 << lvp[l].log2nb, ns = kSynthpSlots / nb;
      const int n_rounds = ((int)lp.scales.size() + ns - 1) / ns;
      const int64_t round_bytes = (int64_t)ns * nb * lp.hop * lp.decimation * 4;
      const int run = (int)std::max<int64_t>(1, std::min<int64_t>(n_rounds, target / std::max<int64_t>(1, round_bytes)));
      const int k = lp.interp_factor == 4 ? 1 : 0;
      for (int b0 = 0; b0 < ep.lv[l].nblk; b0 += nb)
        for (int r0 = 0; r0 < n_rounds; r0 += run) {
          const int nr = std::min(run, n_rounds - r0);
          emit(SynthpItem{(int32_t)l, b0, r0, nr}, (int64_t)nr * round_bytes, k);
        }
    }
  }, &all);
  out->items[0].assign(all.begin(), all.begin() + n0);
  out->items[1].assign(all.begin() + n0, all.end());
  return GCWT_OK;
}

}  // namespace gcwt
