// What the forest explanation engines (path-perturbation LOCO, partial dependence / ICE and its two-way surfaces
// -- common/pd_pair_walk.hpp has their rectangle enumeration --, TreeSHAP) share between
// their HIP kernels and their host twins, written once: the packed node record and the walk over it, the
// fixed-point contribution, and the decoding of a merged TreeSHAP path element. The kernels and the twins promise
// the same integers bit for bit; all of them evaluate the functions below, so a rule cannot change on one side only.
#pragma once
#include "common/tree_rules.hpp"

namespace tmog {

// One node of a flat forest as models/tree_engine.py forest_loco_plan packs it, 16 bytes: the slot u of the split
// column among the forest's sorted distinct split columns, the split bin with the default direction folded in,
// and the children (left < 0: a leaf; the record's index is also the row of the leaf values).
// Device arrays are 16-byte aligned, so a kernel fetches a record with one 16-byte load; host arrays come from
// numpy with no such promise.
#ifdef __HIPCC__
#define TMOG_NODE_ALIGN alignas(16)
#else
#define TMOG_NODE_ALIGN
#endif
struct TMOG_NODE_ALIGN WalkNode {
  int32_t u;        // slot of the split column
  int32_t bin_dl;   // split bin | default_left << 16
  int32_t left;
  int32_t right;
  TMOG_HD bool leaf() const { return left < 0; }
  TMOG_HD int split_bin() const { return bin_dl & 0xFFFF; }
};
static_assert(sizeof(WalkNode) == 16, "packed node record: four 32-bit words");

// Does a row that shows `bin` to this node go left (missing bin and default direction as in scoring).
TMOG_HD bool node_goes_left(int bin, const WalkNode& nd, int missing_bin) {
  return goes_left((uint8_t)bin, nd.split_bin(), [&] { return (nd.bin_dl >> 16) != 0; }, missing_bin);
}

// The walk from `node` down to its leaf, which it returns. bin_of(nd, node) gives the bin that the internal node
// `node` with record nd sees: the row's own bin of slot nd.u (staged bins on the device, xr[used[u]] on the host),
// or whatever the caller puts in its place. It is called once per internal node in path order, so it may also
// look at the path (count, record, tighten a bound).
template <class Idx, class BinOf>
TMOG_HD Idx walk_to_leaf(const WalkNode* nodes, int missing_bin, Idx node, BinOf bin_of) {
  for (;;) {
    const WalkNode nd = nodes[node];
    if (nd.leaf()) return node;
    node = node_goes_left(bin_of(nd, node), nd, missing_bin) ? nd.left : nd.right;
  }
}
// The same walk from `node` down to `stop`, an internal node of that path: the kernels keep no array of path nodes
// and look at the part of a path above a node by walking it again.
template <class Idx, class BinOf>
TMOG_HD void walk_prefix(const WalkNode* nodes, int missing_bin, Idx node, Idx stop, BinOf bin_of) {
  while (node != stop) {
    const WalkNode nd = nodes[node];
    node = node_goes_left(bin_of(nd, node), nd, missing_bin) ? nd.left : nd.right;
  }
}

// The fixed-point contribution of a tree of weight w whose answer moves from leaf value v0 to v1 (fx_base: the
// answer v itself): formed in fp64 from the fp32 values without contraction, scaled by the power of two `scale`
// and rounded to nearest-even -- __double2ll_rn on the device and llrint on the host are the same rounding. Sums
// of these integers do not depend on any order, which is what makes the engines reproducible and device = host.
TMOG_HD int64_t fx_round(double x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __double2ll_rn(x);
#else
  return std::llrint(x);
#endif
}
TMOG_HD int64_t fx_delta(double w, float v1, float v0, double scale) {
  TMOG_FP_EXACT
  return fx_round(w * ((double)v1 - (double)v0) * scale);
}
TMOG_HD int64_t fx_base(double w, float v, double scale) {
  TMOG_FP_EXACT
  return fx_round(w * (double)v * scale);
}

// A merged TreeSHAP path element's range word (models/tree_engine.py forest_paths):
// lo | hi << 12 | (the missing bin satisfies it) << 24. Does a row whose column shows `bin` satisfy the element.
TMOG_HD bool element_satisfied(int rng, int bin, int missing_bin) {
  const int lo = rng & 0xFFF, hi = (rng >> 12) & 0xFFF;
  return (missing_bin >= 0 && bin == missing_bin) ? ((rng >> 24) & 1) != 0 : (lo <= bin && bin <= hi);
}

}  // namespace tmog
