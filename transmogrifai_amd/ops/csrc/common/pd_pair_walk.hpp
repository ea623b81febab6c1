// The rectangle enumeration of the two-way partial dependence engine (hip/pd_pair_kernels.hip and its host twin
// host/pd_pairs_cpu.cpp), written once. For one (row, tree) and a pair of split-column slots (ua, ub) the tree's
// answer over the (bin_a, bin_b) grid is piecewise constant on rectangles, and constant everywhere unless one of
// the two columns lies on the row's own path. The functions below find the anchor (the first node of the base path
// whose column is ua or ub), tile the grid below it by strips without a stack or an array of path nodes, and turn a
// rectangle into the corners of a 2-D integer difference.
#pragma once
#include "common/forest_walk.hpp"

namespace tmog {

// The first internal node of the row's base path from `node` whose column slot is ua or ub, or -1 when the path
// reaches its leaf without one (own_bin(nd): the row's own bin of slot nd.u). A slot of -1 (a column no tree
// splits on) matches nothing.
template <class Idx, class OwnBin>
TMOG_HD Idx pd_pair_anchor(const WalkNode* nodes, int missing_bin, Idx node, int ua, int ub, OwnBin own_bin) {
  for (;;) {
    const WalkNode nd = nodes[node];
    if (nd.leaf()) return (Idx)-1;
    if (nd.u == ua || nd.u == ub) return node;
    node = node_goes_left(own_bin(nd), nd, missing_bin) ? nd.left : nd.right;
  }
}

// Tiles the lines [i_begin, i_end) of the NB x NB grid (first axis: column ua) below `anchor` by rectangles of one
// leaf each and calls emit(i_lo, i_hi, j_lo, j_hi, leaf) for every one, bounds inclusive. NO is the number of
// ordinary bins; with a missing bin (NO < NB, missing_bin == NO) the grid's last line and last column are the
// missing bin's and come as rectangles of their own: (i_lo .. i_hi, NO, NO) an interval of the last column,
// (NO, NO, j_lo .. j_hi) an interval of the last line, (NO, NO, NO, NO) the corner. Every cell of the lines is
// covered exactly once, whatever i_begin is, so a caller may serve the lines in chunks.
//
// One walk from the anchor with column ua at bin i and ub at bin j (all others at the row's own bins) ends in a
// leaf that holds on [i, hi_i] x [j, hi_j]: hi_i is the smallest split bin of the ua-nodes at which the walk turns
// left, hi_j likewise -- each node looks at one coordinate only, and a right turn stays a right turn as the
// coordinate grows. A strip starts at line i: pass 1 sweeps j = 0, hi_j + 1, ... (and the missing j) and takes
// strip_hi = min hi_i; pass 2 sweeps again and emits [i, strip_hi] x [j, hi_j]; the next strip starts at
// strip_hi + 1. The missing line is one more sweep along the ua-nodes' default directions. Returns the number of
// walks.
template <class Idx, class OwnBin, class Emit>
TMOG_HD int64_t pd_pair_rectangles(const WalkNode* nodes, int missing_bin, Idx anchor, int ua, int ub, int NO, int NB,
                                   int i_begin, int i_end, OwnBin own_bin, Emit emit) {
  int64_t walks = 0;
  auto walk_at = [&](int bi, int bj, int* hi_i, int* hi_j) {
    ++walks;
    return walk_to_leaf(nodes, missing_bin, anchor, [&](const WalkNode& nd, Idx) {
      if (nd.u == ua) {
        if (node_goes_left(bi, nd, missing_bin) && nd.split_bin() < *hi_i) *hi_i = nd.split_bin();
        return bi;
      }
      if (nd.u == ub) {
        if (node_goes_left(bj, nd, missing_bin) && nd.split_bin() < *hi_j) *hi_j = nd.split_bin();
        return bj;
      }
      return (int)own_bin(nd);
    });
  };
  const bool has_missing = NO < NB;
  const int o_end = i_end < NO ? i_end : NO;
  int i = i_begin;
  while (i < o_end) {
    int strip_hi = o_end - 1;
    for (int j = 0; j < NO;) {
      int hj = NO - 1;
      walk_at(i, j, &strip_hi, &hj);
      j = hj + 1;
    }
    if (has_missing) {
      int hj = 0;
      walk_at(i, missing_bin, &strip_hi, &hj);
    }
    int unused = strip_hi;
    for (int j = 0; j < NO;) {
      int hj = NO - 1;
      const Idx leaf = walk_at(i, j, &unused, &hj);
      emit(i, strip_hi, j, hj, leaf);
      j = hj + 1;
    }
    if (has_missing) {
      int hj = 0;
      const Idx leaf = walk_at(i, missing_bin, &unused, &hj);
      emit(i, strip_hi, NO, NO, leaf);
    }
    i = strip_hi + 1;
  }
  if (has_missing && i_begin <= NO && NO < i_end) {
    int unused = 0;
    for (int j = 0; j < NO;) {
      int hj = NO - 1;
      const Idx leaf = walk_at(missing_bin, j, &unused, &hj);
      emit(NO, NO, j, hj, leaf);
      j = hj + 1;
    }
    int hj = 0;
    const Idx leaf = walk_at(missing_bin, missing_bin, &unused, &hj);
    emit(NO, NO, NO, NO, leaf);
  }
  return walks;
}

// A rectangle of pd_pair_rectangles as a difference: add(i, j, negate) is called for every corner that takes the
// rectangle's delta d (negate: -d). o_end is the end of the caller's ordinary lines (min(i_end, NO)): the caller
// takes its prefix sums over its own lines only, so corners past them, and past the last ordinary bin, are dropped.
// An ordinary rectangle has the four corners of a 2-D difference; an interval of the last column or of the last
// line the two ends of a 1-D difference along it; the corner cell takes d itself.
template <class Add>
TMOG_HD void pd_pair_corners(int i_lo, int i_hi, int j_lo, int j_hi, int NO, int o_end, Add add) {
  add(i_lo, j_lo, false);
  if (i_lo < NO && i_hi + 1 < o_end) add(i_hi + 1, j_lo, true);
  if (j_lo < NO && j_hi + 1 < NO) {
    add(i_lo, j_hi + 1, true);
    if (i_lo < NO && i_hi + 1 < o_end) add(i_hi + 1, j_hi + 1, false);
  }
}

}  // namespace tmog
