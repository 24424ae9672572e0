// coherence.cpp -- the host side of gcwt_coherence (include/ghostcwt.h): argument checks, the pair list cut into
// tile-pair tasks, the launch (coherence.hip).  Plan-independent, like gcwt_rows_to_host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>

#include "../../include/ghostcwt_debug.h"
#include "coherence.h"
#include "errors.h"
#include "resident_op.h"

static_assert(gcwt::kCohTile == GCWT_COHERENCE_TILE, "ghostcwt_debug.h names the tile the kernel is built for");

namespace gcwt {

void coherence_tasks(int32_t n_channels, const int32_t* pairs, int32_t n_pairs, std::vector<CohTask>* tasks,
                     std::vector<CohEntry>* entries) {
  const int n_tiles = (n_channels + kCohTile - 1) / kCohTile;
  auto valid_rows = [&](int tile) {                        // the channels a (ragged last) tile holds
    const int n = std::min(kCohTile, n_channels - tile * kCohTile);
    return (uint32_t)((1u << n) - 1u);
  };
  std::map<std::pair<int, int>, std::vector<CohEntry>> by_tiles;      // ordered: (tile_a, tile_b)
  for (int32_t p = 0; p < n_pairs; ++p) {
    int a = pairs[2 * p], b = pairs[2 * p + 1], conj = 0;
    // the cell's first index is a channel of the lower tile (of the lower channel inside one tile): the other order
    // of a pair is the same cell, conjugated
    if (a > b) { std::swap(a, b); conj = 1; }
    const int cell = (a % kCohTile) * kCohTile + b % kCohTile;
    by_tiles[{a / kCohTile, b / kCohTile}].push_back({cell, conj, p});
  }
  tasks->clear();
  entries->clear();
  std::vector<char> has_power(n_tiles, 0);
  for (auto& kv : by_tiles) {
    CohTask t{};
    t.tile_a = kv.first.first;
    t.tile_b = kv.first.second;
    t.entry_first = (int32_t)entries->size();
    t.n_entries = (int32_t)kv.second.size();
    for (const CohEntry& e : kv.second) {
      t.cells |= 1ull << e.cell;
      t.rows_a |= 1u << (e.cell / kCohTile);
      t.rows_b |= 1u << (e.cell % kCohTile);
      entries->push_back(e);
    }
    if (!has_power[t.tile_a]) { t.flags |= 1; t.rows_a |= valid_rows(t.tile_a); has_power[t.tile_a] = 1; }
    if (!has_power[t.tile_b]) { t.flags |= 2; t.rows_b |= valid_rows(t.tile_b); has_power[t.tile_b] = 1; }
    if (t.tile_a == t.tile_b) t.rows_a = t.rows_b = t.rows_a | t.rows_b;   // one set of rows, read once
    tasks->push_back(t);
  }
  for (int tile = 0; tile < n_tiles; ++tile) {
    if (has_power[tile]) continue;
    CohTask t{};
    t.tile_a = t.tile_b = tile;
    t.flags = 1;
    t.entry_first = (int32_t)entries->size();
    t.rows_a = t.rows_b = valid_rows(tile);
    tasks->push_back(t);
  }
}

}  // namespace gcwt

using namespace gcwt;

namespace {

constexpr const char* kOp = "gcwt_coherence";

int check_pairs(int32_t n_channels, const int32_t* pairs, int32_t n_pairs) {
  const int rc = check_channels(kOp, n_channels);
  if (rc) return rc;
  if (n_pairs < 0 || (n_pairs > 0 && !pairs)) return fail(GCWT_ERR_INVALID, "gcwt_coherence: pairs is NULL or n_pairs negative");
  for (int32_t p = 0; p < n_pairs; ++p) {
    const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || b < 0 || a >= n_channels || b >= n_channels)
      return fail(GCWT_ERR_INVALID, "gcwt_coherence: pair " + std::to_string(p) + " names a channel outside [0, n_channels)");
    if (a == b) return fail(GCWT_ERR_INVALID, "gcwt_coherence: pair " + std::to_string(p) + " is a channel with itself");
  }
  return GCWT_OK;
}

}  // namespace

extern "C" {

int gcwt_debug_coherence_tasks(int32_t n_channels, const int32_t* pairs, int32_t n_pairs, int32_t* tile_a,
                               int32_t* tile_b, int32_t* flags, int32_t* entry_first, int32_t* entries,
                               int32_t max_tasks) {
  return guarded([&] {
    const int rc = check_pairs(n_channels, pairs, n_pairs);
    if (rc) return rc;
    std::vector<gcwt::CohTask> tasks;
    std::vector<gcwt::CohEntry> ent;
    gcwt::coherence_tasks(n_channels, pairs, n_pairs, &tasks, &ent);
    const int n = (int)tasks.size();
    for (int i = 0; i < std::min(n, (int)max_tasks); ++i) {
      if (tile_a) tile_a[i] = tasks[i].tile_a;
      if (tile_b) tile_b[i] = tasks[i].tile_b;
      if (flags) flags[i] = tasks[i].flags;
      if (entry_first) { entry_first[i] = tasks[i].entry_first; entry_first[i + 1] = tasks[i].entry_first + tasks[i].n_entries; }
    }
    if (entries && n <= max_tasks)
      for (size_t e = 0; e < ent.size(); ++e) {
        entries[3 * e] = ent[e].cell;
        entries[3 * e + 1] = ent[e].conjugate;
        entries[3 * e + 2] = ent[e].out_row;
      }
    return n;
  });
}

int gcwt_coherence(const float* d_rows, int64_t pitch, int32_t n_channels, int32_t n_scales, int64_t n_cols,
                   const int32_t* pairs, int32_t n_pairs, int64_t window, float* d_power, float* d_cross,
                   float* d_coherence, int64_t out_pitch) {
  return guarded([&] {
    if (!d_rows) return fail(GCWT_ERR_INVALID, "gcwt_coherence: d_rows is NULL");
    int rc = check_rows(kOp, n_scales, n_cols, pitch);
    if (rc) return rc;
    rc = check_window(kOp, window);
    if (rc) return rc;
    rc = check_pairs(n_channels, pairs, n_pairs);
    if (rc) return rc;
    if (!d_power && (n_pairs == 0 || (!d_cross && !d_coherence)))
      return fail(GCWT_ERR_INVALID, "gcwt_coherence: nothing to compute (no output, or no pairs and no d_power)");
    const int64_t n_bins = (n_cols + window - 1) / window;
    if (out_pitch < n_bins) return fail(GCWT_ERR_INVALID, "gcwt_coherence: out_pitch is below the number of bins, ceil(n_cols / window)");

    rc = resolve_device(kOp, d_rows, {d_power, d_cross, d_coherence});
    if (rc) return rc;

    std::vector<gcwt::CohTask> tasks;
    std::vector<gcwt::CohEntry> ent;
    gcwt::coherence_tasks(n_channels, pairs, n_pairs, &tasks, &ent);
    if (!d_power)                                          // the entry-less tasks only make power
      while (!tasks.empty() && tasks.back().n_entries == 0) tasks.pop_back();

    // a task's run of bins: about 4096 columns for each of the workgroup's four waves, fewer runs where the grid
    // would not fit
    int64_t run_bins = 4 * std::max<int64_t>(1, (4096 + window - 1) / window);
    auto runs = [&] { return (n_bins + run_bins - 1) / run_bins; };
    while ((int64_t)tasks.size() * runs() * n_scales > 0x7fffffff) run_bins *= 2;

    // one copy: the tasks, then their entries (one of zeros where there is none)
    if (ent.empty()) ent.push_back(gcwt::CohEntry{});
    DeviceTable tab;
    const size_t at_tasks = tab.add(tasks.data(), sizeof(gcwt::CohTask) * tasks.size());
    const size_t at_entries = tab.add(ent.data(), sizeof(gcwt::CohEntry) * ent.size());
    rc = tab.upload(kOp, nullptr);
    if (rc) return rc;

    gcwt::CohArgs a{};
    a.rows = reinterpret_cast<const float2*>(d_rows);
    a.pitch = pitch; a.n_cols = n_cols; a.window = window; a.n_bins = n_bins; a.out_pitch = out_pitch;
    a.n_channels = n_channels; a.n_scales = n_scales; a.n_tasks = (int32_t)tasks.size();
    a.run_bins = run_bins; a.n_runs = runs();
    a.tasks = tab.at<gcwt::CohTask>(at_tasks);
    a.entries = tab.at<gcwt::CohEntry>(at_entries);
    a.power = d_power; a.cross = reinterpret_cast<float2*>(d_cross); a.coherence = d_coherence;
    return finish(kOp, gcwt::launch_coherence(a, nullptr));
  });
}

}  // extern "C"
