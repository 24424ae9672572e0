// squeeze.hip -- the synchrosqueezed transform of a run of rows of a resident complex result (include/ghostcwt.h:
// gcwt_squeeze; profiles/squeeze.md).  The input rows are first .. first + R - 1; g, floor2 and nu are per-row tables,
// edges[0 .. L] the ascending edges of L frequency cells.  For a channel c, an input row r and a column t, every operation
// a single correctly rounded float32 one (wave_reduce.h: norm2; phase_advance.h: the frequency; no fast-math, no
// contraction):
//   frequency = phase_advance_hz(W[c, r, tp], W[c, r, tm], tp - tm, nu[r], hz_per_cycle) with tm = max(t - 1, seg.start),
//     tp = min(t + 1, seg.stop - 1) inside the segment of t: ridge.hip's, on every row; it does not depend on floor2
//   the entry is out where !(norm2(w) > floor2[r]), frequency is NaN, frequency < edges[0] or frequency >= edges[L];
//     else its cell is the largest l with edges[l] <= frequency, by binary search on the float32 values
//   index = the output row, l or L - 1 - l with `descending`; -1 where the entry is out
//   coefficients[c, row, t]: from (0, 0), the input rows walked in ascending r, every entry that is not out does
//     acc.x = fmaf(g[r], w.x, acc.x);  acc.y = fmaf(g[r], w.y, acc.y)  on its own row: one chain per cell and column
//   power = norm2(coefficients)
// No atomics and no cross-lane sums: a lane owns its columns, the chain of a cell runs along the rows inside that lane,
// and what it reads is its own rows at the columns tm, t and tp.  Nothing depends on the column count, the pitch, the
// tiling, the grouping of the cells or which outputs are asked for, and two runs agree in bits.
//
// The cut: a workgroup of four waves takes one channel, a tile of kSqCols columns and a group of up to kSqCells
// consecutive output rows; a lane owns two adjacent columns.  The accumulators live in LDS as acc[cell][slot][lane]
// float2, slot the lane's first or second column: whichever cells the lanes of a wave hit, they touch consecutive 8-byte
// words, and a cell is 4 KiB from the next, so neither the 32-lane groups of the reads nor the 16-lane groups of the
// writes meet on a bank.  A lane reads and writes no word but its own: there is no barrier.  The workgroup walks the
// input rows in ascending order, kSqDepth rows' loads in flight -- 16 bytes per lane where rows and output rows start on
// 16 bytes (`aligned`), else 8 bytes per column.  The neighbour columns come from the adjacent lanes; the first and the
// last lane of a wave load theirs (one load instruction with two lanes, into lines the wave beside reads anyway).  With
// more cells than one group holds each group walks the rows again and keeps what lands in its own cells.  A group needs
// no search: the 17 edges of its own 16 cells are wave-uniform and sit in scalar registers, and the cell of an entry that
// lies between the first and the last of them is the number of inner edges at or below its frequency -- 15 compares, no
// memory.  Group 0 alone writes frequency; of index every group writes the entries of its own cells and group 0 the -1
// of those that are out, so every entry is written once.  Where nothing is summed (neither coefficients nor power)
// there is one group, and it finds the cell by binary search over all the edges, read per lane.  After the walk a lane
// stores its columns of the group's cells, a wave whole runs of the tile's columns.  The tables are read through the
// constant address space.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "phase_advance.h"
#include "squeeze.h"
#include "wave_reduce.h"

// A product and the sum it feeds stay two roundings unless the code says fmaf.
#pragma clang fp contract(off)

namespace gcwt {

namespace {

constexpr int kSqDepth = 4;                                 // rows whose loads are in flight

// the output row of an entry with |w|^2 = r2 and frequency f, or -1 (e0 = edges[0], e_top = edges[n_cells])
__device__ __forceinline__ int cell_row(const SqArgs& a, Const<float> edges, float e0, float e_top, bool exists, float r2,
                                        float floor2, float f) {
  if (!(exists && r2 > floor2 && f >= e0 && f < e_top)) return -1;          // (a NaN fails both comparisons)
  int lo = 0, hi = a.n_cells - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (edges[mid] <= f) lo = mid; else hi = mid - 1;
  }
  return a.descending ? a.n_cells - 1 - lo : lo;
}

// The same answer for one group of cells, without memory: ge[0 .. kSqCells] are the ascending edges of the group's cells
// (wave-uniform; +inf behind the group's last cell), g_top the upper edge of its last cell.  -> the entry's place among
// the group's output rows, or -1: the entry is out or its cell is another group's.  The cell is the number of inner
// edges at or below f, which for ascending edges is the largest l with edges[l] <= f.
__device__ __forceinline__ int group_slot(const float (&ge)[kSqCells + 1], float g_top, int rows_here, bool descending, bool in,
                                          float f) {
  if (!(in && f >= ge[0] && f < g_top)) return -1;                          // (a NaN fails both comparisons)
  int k = 0;
#pragma unroll
  for (int j = 1; j < kSqCells; ++j) k += f >= ge[j] ? 1 : 0;
  return descending ? rows_here - 1 - k : k;
}

// one entry enters the chain of its cell: the prescribed sequence (k: its place among the group's rows, or -1)
__device__ __forceinline__ void add_entry(float2* acc, int k, float g, float2 w) {
  if (k >= 0) {
    float2 s = acc[k * kSqCols];
    s.x = fmaf(g, w.x, s.x);
    s.y = fmaf(g, w.y, s.y);
    acc[k * kSqCols] = s;
  }
}

// FULL: all kSqCols columns of the tile exist.  ALIGNED: SqArgs::aligned
template <bool FULL, bool ALIGNED>
__device__ __forceinline__ void run_tile(const SqArgs& a, float2* lds, int ch, int grp, int64_t ct) {
  const int lane = threadIdx.x & 63;
  const int64_t c0 = ct * kSqCols + (int64_t)threadIdx.x * kSqLaneCols;        // this lane's columns: c0 and c0 + 1
  const bool ok0 = FULL || c0 < a.n_cols, ok1 = FULL || c0 + 1 < a.n_cols;
  const int row0 = grp * kSqCells, rows_here = std::min(kSqCells, a.n_cells - row0);   // the group's output rows
  const bool sums = a.coefficients || a.power, first_group = grp == 0;
  const bool store_f = first_group && a.frequency, store_i = first_group && a.index;

  // acc[cell][slot][lane]: this lane's words are lds[cell * kSqCols + slot * kSqThreads + threadIdx.x]
  float2* const acc0 = lds + threadIdx.x;
  float2* const acc1 = acc0 + kSqThreads;
  if (sums)
    for (int k = 0; k < rows_here; ++k) acc0[k * kSqCols] = acc1[k * kSqCols] = make_float2(0.f, 0.f);

  // the segments of the two columns (host-checked: ascending, each starting where the one before stops, covering
  // [0, n_cols)): the last one that starts at or before c0, and for c0 + 1 that one or the next.  Which neighbours a
  // column has follows: the one before it from its segment's start, the one behind it from its segment's stop.
  bool before0 = false, behind0 = false, before1 = false, behind1 = false;
  if (ok0) {
    const Const<longlong2> seg = constant(a.segments);
    int64_t lo = 0, hi = a.n_segments - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (seg[mid].x <= c0) lo = mid; else hi = mid - 1;
    }
    int64_t start = seg[lo].x, stop = seg[lo].y;
    before0 = c0 - 1 >= start;
    behind0 = c0 + 1 <= stop - 1;
    if (ok1) {
      if (c0 + 1 >= stop && lo + 1 < a.n_segments) { start = seg[lo + 1].x; stop = seg[lo + 1].y; }
      before1 = c0 >= start;
      behind1 = c0 + 2 <= stop - 1;
    }
  }
  const int span0 = (int)before0 + (int)behind0, span1 = (int)before1 + (int)behind1;
  // the wave's two outer columns: the first lane's c0 - 1 and the last lane's c0 + 2, where a segment reaches them
  // (then 0 <= the column < n_cols)
  const bool outer = (lane == 0 && before0) || (lane == 63 && behind1);
  const int outer_at = lane == 0 ? -1 : 2;

  const Const<float> wg = constant(a.g), wfloor = constant(a.floor2), wnu = constant(a.nu), edges = constant(a.edges);
  const float e0 = edges[0], e_top = edges[a.n_cells];
  // the group's cells, ascending: [cell_lo, cell_lo + rows_here), and their edges
  const int cell_lo = a.descending ? a.n_cells - row0 - rows_here : row0;
  float ge[kSqCells + 1];
#pragma unroll
  for (int j = 0; j <= kSqCells; ++j) ge[j] = j < rows_here ? edges[cell_lo + j] : __builtin_inff();
  const float g_top = edges[cell_lo + rows_here];
  // ALIGNED: pitch is even and c0 is, so c0 < n_cols <= pitch puts c0 + 1 inside the row's pitch
  const float2* base = a.rows + (int64_t)ch * a.n_scales * a.pitch + c0;
  const int64_t out = (int64_t)ch * a.count * a.out_pitch + c0;               // of frequency and index, the run's first row
  const int end = a.first + a.count;
  for (int r = a.first; r < end; r += kSqDepth) {
    float4 v[kSqDepth];
    float2 edge[kSqDepth];
#pragma unroll
    for (int i = 0; i < kSqDepth; ++i) {
      v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      edge[i] = make_float2(0.f, 0.f);
      if (r + i < end) {                                     // (wave-uniform)
        const float2* row = base + (int64_t)(r + i) * a.pitch;
        if (ALIGNED) {
          if (ok0) v[i] = *reinterpret_cast<const float4*>(row);
        } else {
          if (ok0) { const float2 w = row[0]; v[i].x = w.x; v[i].y = w.y; }
          if (ok1) { const float2 w = row[1]; v[i].z = w.x; v[i].w = w.y; }
        }
        if (outer) edge[i] = row[outer_at];
      }
    }
#pragma unroll
    for (int i = 0; i < kSqDepth; ++i) {
      if (r + i >= end) continue;
      const float2 w0 = make_float2(v[i].x, v[i].y), w1 = make_float2(v[i].z, v[i].w);
      // the column before c0 is the second of the lane before, the column behind c0 + 1 the first of the lane behind
      float2 left = make_float2(__shfl_up(w1.x, 1), __shfl_up(w1.y, 1));
      float2 right = make_float2(__shfl_down(w0.x, 1), __shfl_down(w0.y, 1));
      if (lane == 0) left = edge[i];
      if (lane == 63) right = edge[i];
      const float nu = wnu[r + i], g = wg[r + i], floor2 = wfloor[r + i];
      const float f0 = phase_advance_hz(behind0 ? w1 : w0, before0 ? left : w0, span0, nu, a.hz_per_cycle);
      const float f1 = phase_advance_hz(behind1 ? right : w1, before1 ? w0 : w1, span1, nu, a.hz_per_cycle);
      const int64_t o = out + (int64_t)(r + i - a.first) * a.out_pitch;
      if (ALIGNED && ok1) {                                  // (o is even: out_pitch and c0 are)
        if (store_f) *reinterpret_cast<float2*>(a.frequency + o) = make_float2(f0, f1);
      } else if (ok0) {
        if (store_f) a.frequency[o] = f0;
        if (store_f && ok1) a.frequency[o + 1] = f1;
      }
      if (sums) {
        // this group's cells only, from registers.  index: the group that holds an entry's cell writes its row, group 0
        // writes the -1 of the entries that are out: every entry is written once
        const bool in0 = ok0 && norm2(w0) > floor2, in1 = ok1 && norm2(w1) > floor2;
        const int k0 = group_slot(ge, g_top, rows_here, a.descending, in0, f0);
        const int k1 = group_slot(ge, g_top, rows_here, a.descending, in1, f1);
        add_entry(acc0, k0, g, w0);
        add_entry(acc1, k1, g, w1);
        if (a.index) {
          if (k0 >= 0) a.index[o] = row0 + k0;
          else if (first_group && ok0 && !(in0 && f0 >= e0 && f0 < e_top)) a.index[o] = -1;
          if (k1 >= 0) a.index[o + 1] = row0 + k1;
          else if (first_group && ok1 && !(in1 && f1 >= e0 && f1 < e_top)) a.index[o + 1] = -1;
        }
      } else if (store_i) {                                  // nothing is summed: one group, the search over all cells
        const int at0 = cell_row(a, edges, e0, e_top, ok0, norm2(w0), floor2, f0);
        const int at1 = cell_row(a, edges, e0, e_top, ok1, norm2(w1), floor2, f1);
        if (ALIGNED && ok1) {
          *reinterpret_cast<int2*>(a.index + o) = make_int2(at0, at1);
        } else if (ok0) {
          a.index[o] = at0;
          if (ok1) a.index[o + 1] = at1;
        }
      }
    }
  }

  if (!ok0 || !sums) return;
  for (int k = 0; k < rows_here; ++k) {
    const float2 z0 = acc0[k * kSqCols], z1 = acc1[k * kSqCols];
    const int64_t o = ((int64_t)ch * a.n_cells + row0 + k) * a.out_pitch + c0;
    if (ALIGNED && ok1) {
      if (a.coefficients) *reinterpret_cast<float4*>(a.coefficients + o) = make_float4(z0.x, z0.y, z1.x, z1.y);
      if (a.power) *reinterpret_cast<float2*>(a.power + o) = make_float2(norm2(z0), norm2(z1));
    } else {
      if (a.coefficients) a.coefficients[o] = z0;
      if (a.power) a.power[o] = norm2(z0);
      if (ok1) {
        if (a.coefficients) a.coefficients[o + 1] = z1;
        if (a.power) a.power[o + 1] = norm2(z1);
      }
    }
  }
}

__global__ void __launch_bounds__(kSqThreads) k_squeeze(SqArgs a) {
  __shared__ float2 lds[kSqCells * kSqCols];
  const TileOfUnit at = shared_place(a.n_groups);            // unit = (channel, column tile)
  if (at.unit >= a.n_units) return;                          // (the last group's padding)
  const int grp = at.tile, ch = (int)(at.unit / a.n_ctiles);
  const int64_t ct = at.unit % a.n_ctiles;
  const bool full = (ct + 1) * kSqCols <= a.n_cols;
  if (a.aligned) {
    if (full) run_tile<true, true>(a, lds, ch, grp, ct);
    else run_tile<false, true>(a, lds, ch, grp, ct);
  } else {
    if (full) run_tile<true, false>(a, lds, ch, grp, ct);
    else run_tile<false, false>(a, lds, ch, grp, ct);
  }
}

}  // namespace

hipError_t launch_squeeze(const SqArgs& a, hipStream_t st) {
  const int64_t blocks = squeeze_blocks(a);
  if (blocks <= 0 || blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_squeeze, dim3((unsigned)blocks), dim3(kSqThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace gcwt
