// How a level's nodes become work items of the level kernels (hip/tree_*_kernels.hip), written once for the two level
// planners that promise the same trees bit for bit: the host-planned loop (common/tree_grow.hpp grow_group) and the
// device-planned one (hip/tree_resident.hip level_plan_kernel). Both evaluate the functions below for the sibling
// flags, the per-node work counts, every item, the zero segments and the parameter slots, so the layout cannot
// change on one side only; host/tree_grow_cpu.cpp tmog_level_items_cpu loops over them for the CPU test
// (tests/test_level_items_cpu.py). Stateless free functions of scalars and small PODs, no allocation; the planners
// keep their own loops, scans and buffers.
#pragma once
#include <cstdint>

#include "common/tmog_abi.h"
#include "common/tree_rules.hpp"

namespace tmog {

using ::FeatGroup;

constexpr int64_t kCsrRows = TMOG_CSR_ITEM_ROWS;    // rows per CSR histogram item (GPU)
constexpr int64_t kPartRows = TMOG_PART_ITEM_ROWS;  // rows per partition item (GPU)

// Per-node bits of a level plan.
enum : int {
  kNodeCan = 1,       // may split (scanned)
  kNodeNeed = 2,      // needs a histogram: scanned, or built as the subtraction partner of its sibling
  kNodePairLeft = 4,  // left node of a sibling pair whose bigger node is derived as parent - smaller
  kNodeDerived = 8    // that derived (big) node: no histogram items, still partition items
};
// What of a built node's histogram is zeroed before its items accumulate into it.
enum : int { kZeroNone, kZeroNode, kZeroCsr };

TMOG_HD int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// Items that cover `count` rows in slices of `step`: an empty node still takes one.
TMOG_HD int64_t row_items(int64_t count, int64_t step) {
  const int64_t k = ceil_div(count, step);
  return k > 1 ? k : 1;
}

// ---- sibling flags
TMOG_HD int root_flags(bool can) { return (can ? kNodeCan : 0) | kNodeNeed; }   // level 0: every root is built
// (left, right) children with their can_split results and counts. With subtraction a splittable node whose sibling
// cannot split still gets its histogram from the parent's: the sibling is built too when it is the smaller one
// (scan skipped: its may-split slot is 0), and a pair that both need one builds the smaller, derives the bigger.
TMOG_HD void sibling_flags(bool can_l, bool can_r, int64_t lc, int64_t rc, bool subtract, int* fl, int* fr) {
  bool nl = can_l, nr = can_r;
  if (subtract && build_sibling(can_l, nl, lc, nr, rc)) nl = nr = true;
  const bool pair = subtract && nl && nr;
  const bool left_big = left_is_big(lc, rc);
  *fl = (can_l ? kNodeCan : 0) | (nl ? kNodeNeed : 0) | (pair ? kNodePairLeft : 0) |
        (pair && left_big ? kNodeDerived : 0);
  *fr = (can_r ? kNodeCan : 0) | (nr ? kNodeNeed : 0) | (pair && !left_big ? kNodeDerived : 0);
}

// ---- per-node work counts
struct NodeWork {
  int64_t nch, ncsr;    // row chunks of a chunk_rows group / of the CSR group
  int64_t n_part;       // partition items (every node that needs a histogram)
  int64_t n_wide;       // wide-load histogram items (built nodes only, as the next three)
  int64_t n_other;      // every other histogram item
  int64_t n_general;    // ... of which on the byte-gather path (neither CSR nor wide-load)
  int zero;             // kZero*
};
// Statistic chunks apply to the groups that accumulate in LDS: register and CSR groups take one item per row chunk.
TMOG_HD int64_t group_items(int gflags, int64_t nch, int64_t ncsr, int n_sc) {
  return ((gflags & TMOG_ITEM_CSR) ? ncsr : nch) * ((gflags & (TMOG_ITEM_CSR | TMOG_ITEM_REG)) ? 1 : n_sc);
}
// fl: the node's flag bits; hsz: words of its histogram; live_dense: GroupLayout (-1: no dense prefix).
TMOG_HD NodeWork node_work(int fl, int64_t count, int64_t chunk_rows, const FeatGroup* groups, int n_groups, int n_sc,
                           int64_t live_dense, int64_t hsz) {
  NodeWork w;
  const bool need = (fl & kNodeNeed) != 0, build = need && !(fl & kNodeDerived);
  w.nch = row_items(count, chunk_rows);
  w.ncsr = row_items(count, kCsrRows);
  w.n_part = need ? row_items(count, kPartRows) : 0;
  w.n_wide = w.n_other = w.n_general = 0;
  bool has_csr = false;
  if (build)
    for (int g = 0; g < n_groups; ++g) {
      const int gfl = groups[g].flags;
      const int64_t k = group_items(gfl, w.nch, w.ncsr, n_sc);
      if (gfl & TMOG_ITEM_WIDE) w.n_wide += k;
      else w.n_other += k;
      if (!(gfl & (TMOG_ITEM_CSR | TMOG_ITEM_WIDE))) w.n_general += k;
      has_csr |= (gfl & TMOG_ITEM_CSR) != 0;
    }
  // a node split over several items accumulates atomically. When only the CSR group is split (kCsrRows-row slices),
  // the single-chunk multi-bin groups still write their words exclusively: only the one-present-bin region past
  // the dense prefix needs zeroing
  const bool dense_split = live_dense >= 0 && live_dense < hsz;
  w.zero = kZeroNone;
  if (build && w.nch > 1) w.zero = kZeroNode;
  else if (has_csr && w.ncsr > 1) w.zero = dense_split ? kZeroCsr : kZeroNode;
  return w;
}
// The zero segment of a node of class cls (not kZeroNone) whose histogram is hsz words at hoff.
TMOG_HD void zero_segment(int cls, int64_t hoff, int64_t hsz, int64_t live_dense, int64_t* off, int64_t* size) {
  *off = cls == kZeroCsr ? hoff + live_dense : hoff;
  *size = cls == kZeroCsr ? hsz - live_dense : hsz;
}

// ---- items
// The k-th histogram item of the built node in slot `node` within the wide-load (wide) or the other section,
// k < NodeWork.n_wide / n_other: group, then statistic chunk, then row chunk. The only place that assembles excl.
TMOG_HD HistItem hist_item_at(bool wide, int32_t node, int64_t k, int64_t begin, int64_t count, int64_t chunk_rows,
                              const FeatGroup* groups, int n_groups, int n_sc, int64_t live_dense) {
  const int64_t nch = row_items(count, chunk_rows), ncsr = row_items(count, kCsrRows);
  HistItem h;
  h.node = node;
  h.fg0 = h.nf = h.excl = 0;
  h.begin = begin;
  h.count = 0;                                      // (k past the section: an empty item)
  for (int g = 0; g < n_groups; ++g) {
    const FeatGroup gr = groups[g];
    const bool reg = gr.flags & TMOG_ITEM_REG, csr = gr.flags & TMOG_ITEM_CSR, wd = gr.flags & TMOG_ITEM_WIDE;
    if (wd != wide) continue;
    const int64_t nit = csr ? ncsr : nch;
    const int64_t ng = group_items(gr.flags, nch, ncsr, n_sc);
    if (k >= ng) {
      k -= ng;
      continue;
    }
    const int64_t sc = k / nit, ci = k - sc * nit;
    const int64_t step = csr ? kCsrRows : chunk_rows;
    h.fg0 = gr.f0;
    h.nf = gr.nf;
    h.excl = (nit == 1 ? TMOG_ITEM_SOLE : 0) | (gr.flags & (TMOG_ITEM_REG | TMOG_ITEM_CSR | TMOG_ITEM_WIDE)) |
             ((reg || csr) && live_dense >= 0 ? TMOG_ITEM_LIVE0 : 0) | (int32_t)(sc << TMOG_ITEM_SC_SHIFT);
    h.begin = begin + ci * step;
    h.count = count - ci * step < step ? count - ci * step : step;
    break;
  }
  return h;
}
// The k-th partition item of the node in slot `node`, k < NodeWork.n_part: short slices (each is a chain of 256-row
// steps with cursor atomics).
TMOG_HD PartItem part_item_at(int32_t node, int64_t k, int64_t begin, int64_t count) {
  PartItem p;
  p.node = node;
  p.pad = 0;
  p.begin = begin + k * kPartRows;
  p.count = count - k * kPartRows < kPartRows ? count - k * kPartRows : kPartRows;
  p.out_left = p.out_right = 0;
  return p;
}
// Leaf collection: a node's rows in chunk_rows slices (none for an empty node); `out` is where its first row goes.
TMOG_HD int64_t leaf_items(int64_t count, int64_t chunk_rows) { return count > 0 ? ceil_div(count, chunk_rows) : 0; }
TMOG_HD LeafItem leaf_item_at(int64_t k, int64_t begin, int64_t count, int64_t chunk_rows, int64_t out, int32_t gid,
                              int32_t buf) {
  const int64_t o = k * chunk_rows;
  LeafItem it;
  it.begin = begin + o;
  it.count = count - o < chunk_rows ? count - o : chunk_rows;
  it.out = out + o;
  it.gid = gid;
  it.buf = buf;
  return it;
}

// ---- the node's parameter block (kPrm* of tree_rules.hpp). paired: scanned with its sibling by the pair scan.
TMOG_HD void fill_node_params(float* P, double min_inst, double min_gain, double mcw, double lambda, bool paired,
                              bool allow_missing, double eps, bool may_split) {
  P[kPrmMinInst] = (float)min_inst;
  P[kPrmMinGain] = (float)min_gain;
  P[kPrmMcw] = (float)mcw;
  P[kPrmLambda] = (float)lambda;
  P[kPrmPaired] = paired ? 1.f : 0.f;
  P[kPrmAllowMissing] = allow_missing ? 1.f : 0.f;
  P[kPrmEps] = (float)eps;
  P[kPrmMaySplit] = may_split ? 1.f : 0.f;
}

// ---- host-only bounds of a level's item counts, from the group's total rows: the sizes of the device planner's
// item buffers and of the grids it launches before the counts exist. m nodes with histograms / n nodes collected.
inline int64_t hist_items_bound(const FeatGroup* groups, int n_groups, int64_t chunk_rows, int n_sc, int64_t total,
                                int64_t m) {
  int64_t h = 0;
  for (int g = 0; g < n_groups; ++g) {
    const int64_t rows = total / ((groups[g].flags & TMOG_ITEM_CSR) ? kCsrRows : chunk_rows) + m + 1;
    h += group_items(groups[g].flags, rows, rows, n_sc);
  }
  return h;
}
inline int64_t part_items_bound(int64_t total, int64_t m) { return total / kPartRows + m + 1; }
inline int64_t leaf_items_bound(int64_t chunk_rows, int64_t total, int64_t n) {
  return total / (chunk_rows > 1 ? chunk_rows : 1) + n + 1;
}

}  // namespace tmog
