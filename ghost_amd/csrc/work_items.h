// work_items.h -- how a plan's levels become the work items of the synthesis kernels: which kernel makes a level, the
// order of its scales, and per launch batch the lists of workgroup items with their level tables.  Host code that makes
// no HIP call: gcwt_plan_upload sends what these functions return, gcwt_debug_work_items shows it without a device.
#pragma once
#include <cstdint>
#include <vector>

#include "plan_state.h"

namespace gcwt {

// Which synthesis kernel makes a level: the interpolating one when the planner designed it
// (amplitude / power, R >= 16), else k_synth7 when the block layout allows, else the 16-column
// fallback.  GHOSTCWT_SYNTH16=1 sends everything to the fallback (A/B tests).
enum LevelKernel { LK_SYNTH16 = 0, LK_SYNTH7 = 7, LK_INTERP = 9 };
LevelKernel level_kernel(const gcwt_plan* p, const LevelPlan& lp);
// an interpolated level goes to the pipelined kernel (synthp.hip) when its layout fits: two phases per scale, a
// lane's sub-sample positions fixed by the lane (I <= 256), whole lane-tasks per block (hop R a multiple of 4 I)
bool level_pipelined(const gcwt_plan* p, const LevelPlan& lp);

// The levels' scale lists, one after the other (d_scale_list before k_scale_windows adds the windows): per level the
// odd kernel lengths (no half-sample delay, real filter) first, even ones after; a Morlet scale's delay is in its
// complex row (k_gain_rows_complex), so all of them are "plain" and the half-sample ramp is never applied.
// scale_off[l]: the level's first entry, n_plain[l]: how many of its entries are plain.
struct ScaleLists {
  std::vector<int32_t> list;
  std::vector<int> scale_off, n_plain;
};
ScaleLists level_scale_lists(const HostPlan& hp);
// [levels][256] exp(-i pi (k - band_shift) / (256 R)): the half-sample ramp of the even kernel lengths
std::vector<float2> half_twiddles(const HostPlan& hp);
// per list entry: demodulation bin | (even kernel length) << 16 (synthi.hip)
std::vector<int32_t> scale_aux(const HostPlan& hp, const std::vector<int32_t>& list);

// The items of one launch batch (`ep`: its first segment) and the level tables they index, per kernel.
struct Synth16Items {
  std::vector<SynthItemDev> items;
  std::vector<SynthLevelDev> levels;
};
struct Synth7Items {
  std::vector<Synth7Item> items, wide, narrow;   // k_synth7, its wide-halo and its 16-column instantiation
  std::vector<Synth7Level> levels;
};
struct SynthiItems {
  std::vector<SynthiItem> items;
  std::vector<SynthiLevel> levels;
  int split = 0;                                  // items[0 .. split): the levels below gcwt_plan::interp_split_r
};
struct SynthpItems {
  std::vector<SynthpItem> items[2];               // [1]: levels with I = 4
  std::vector<SynthpLevel> levels;
};
Synth16Items synth16_items(const gcwt_plan* p, const EpochPlan& ep);
Synth7Items synth7_items(const gcwt_plan* p, const EpochPlan& ep, const ScaleLists& sl);
// GCWT_ERR_INVALID ("internal: ... outside the kernel's limits") where a level breaks what its kernel's indexing assumes
int synthi_items(const gcwt_plan* p, const EpochPlan& ep, const ScaleLists& sl, SynthiItems* out);
int synthp_items(const gcwt_plan* p, const EpochPlan& ep, const ScaleLists& sl, SynthpItems* out);

}  // namespace gcwt
