// Exact leave-one-column-out (LOCO) sums of the tree engine's flat forests by path perturbation, CDNA4 (gfx950).
//
// Replacing column c of a row by the bin of the value 0 can change tree t's answer only if c is tested on the path
// the row already takes through t. Per (row, tree) the kernel therefore
//   1. walks the base path (tmog::walk_to_leaf) and adds w_t v[leaf] to the base slot; a node of that path is FLIPPED
//      when the zero bin of its column decides differently from the row's bin (missing bin and default direction
//      take part as in scoring);
//   2. walks the base path once more; every flipped node belongs to the candidate of its column (slot u) and, if
//      the column is in a group, to the group's candidate (slot U + g). A candidate is handled at its FIRST flipped
//      node on the path: the walk is redone from that node with the override applied at every node of the candidate
//      met from there on (a column that repeats on the path, group members that follow one another), and if it ends
//      in another leaf, w_t (v[leaf'] - v[leaf]) is added to the candidate's slot. The nodes above the first flipped
//      node do not change direction, so the prefix of the path is shared and needs no re-walk.
// "Was this candidate flipped higher up" is answered by walking the prefix of the base path again (only from the
// second flipped node of a path on): no per-lane array of path nodes, whatever the depth (Spark allows 30), so
// nothing spills to scratch.
//
// Mapping: a workgroup owns a tile of rows and stages the bins of the used columns of its rows, and the per-slot
// zero bin and group, in LDS; its lanes take (row, tree) pairs, rows fastest, so the lanes of a wave walk the same
// tree (node records are 16-byte loads shared through L2 / L1, diverging only with depth). Nodes come as the packed
// records of common/forest_walk.hpp; hip/row_tile.hpp has the tile scaffold and the tile-size rule.
//
// Accumulation is order-independent, hence bitwise reproducible and equal to the host twin (host/loco_cpu.cpp):
// each contribution is rounded to int64 fixed point (tmog::fx_base / fx_delta have the rule) and added to the
// workgroup's LDS tile [rows][U + G + 1][C] with 64-bit LDS integer atomics; the tile is converted to fp64 and
// written with plain stores at the end.
// Bound of the scale: with S = sum_t |w_t| max |value_t|, the base slot's partial sums stay within S and a delta
// slot's within 2 S (each tree adds at most |w_t| (|v'| + |v|)); scale is the power of two with S * scale < 2^61,
// so every partial sum is below 2^62 in magnitude and the at most T roundings of 1/2 each cannot reach 2^63.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip/tmog_hip_abi.h"
#include "hip/row_tile.hpp"
#include "common/forest_walk.hpp"

namespace {

using tmog::kTileThreads;
using Node = tmog::WalkNode;

struct LocoArgs : tmog::RowTile {
  const int32_t* slot_meta;   // [U] zero bin | (group + 1) << 8
  int G;
  int T;
  const int64_t* tree_off;
  const Node* nodes;
  const float* value;
  int KV;
  const float* tree_weight;
  const int32_t* tree_out;
  double* out;
};

// Adds tree weight w times the leaf values v, or times the move from v0 to v1, to the KV cells at dst.
__device__ __forceinline__ void loco_add(unsigned long long* dst, const LocoArgs& a, double w, const float* v) {
  for (int c = 0; c < a.KV; ++c) atomicAdd(dst + c, (unsigned long long)tmog::fx_base(w, v[c], a.scale));
}
__device__ __forceinline__ void loco_add(unsigned long long* dst, const LocoArgs& a, double w, const float* v1,
                                         const float* v0) {
  for (int c = 0; c < a.KV; ++c) atomicAdd(dst + c, (unsigned long long)tmog::fx_delta(w, v1[c], v0[c], a.scale));
}

__global__ void __launch_bounds__(kTileThreads) forest_loco_kernel(LocoArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t blk0 = tmog::tile_first_row(a);
  if (blk0 >= a.n) return;
  const int nrow = tmog::tile_row_count(a, blk0);
  const int slots = (a.U + a.G + 1) * a.C;
  const size_t nacc = (size_t)a.tile_rows * slots;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);
  int32_t* meta = reinterpret_cast<int32_t*>(smem + nacc * 8);
  uint8_t* sbin = smem + nacc * 8 + (size_t)a.ustride * 4;
  tmog::zero_tile(acc, nacc);
  for (int k = threadIdx.x; k < a.U; k += kTileThreads) meta[k] = a.slot_meta[k];
  tmog::stage_used_bins(a, blk0, nrow, sbin);
  __syncthreads();
  const int items = nrow * a.T;
  for (int it = threadIdx.x; it < items; it += kTileThreads) {
    const int t = it / nrow, r = it - t * nrow;
    const int root = (int)a.tree_off[t];
    if ((int)a.tree_off[t + 1] <= root) continue;
    const uint8_t* xr = sbin + (size_t)r * a.ustride;
    // a node is flipped when the zero bin of its column decides differently from the row's bin
    auto left = [&](const Node& nd) { return tmog::node_goes_left(xr[nd.u], nd, a.missing_bin); };
    auto flipped = [&](const Node& nd, bool l) {
      return l != tmog::node_goes_left(meta[nd.u] & 0xFF, nd, a.missing_bin);
    };
    // 1. the base path
    int nflip = 0;
    const int leaf = tmog::walk_to_leaf(a.nodes, a.missing_bin, root, [&](const Node& nd, int) {
      nflip += flipped(nd, left(nd));
      return (int)xr[nd.u];
    });
    const double w = (double)a.tree_weight[t];
    const float* v0 = a.value + (size_t)leaf * a.KV;
    unsigned long long* dst = acc + (size_t)r * slots + a.tree_out[t];
    loco_add(dst + (size_t)(a.U + a.G) * a.C, a, w, v0);
    if (nflip == 0) continue;
    // 2. every candidate from its first flipped node: the walk with the override at the candidate's nodes
    auto perturbed = [&](int node, auto over) {
      return tmog::walk_to_leaf(a.nodes, a.missing_bin, node, [&](const Node& nd, int) {
        return over(nd.u) ? (meta[nd.u] & 0xFF) : (int)xr[nd.u];
      });
    };
    int seen = 0, node = root;
    for (;;) {
      const Node nd = a.nodes[node];
      if (nd.leaf()) break;
      const bool l = left(nd);
      if (flipped(nd, l)) {
        const int u = nd.u, g = (meta[u] >> 8) - 1;
        bool seen_u = false, seen_g = false;
        if (seen > 0)                          // was the candidate flipped higher up on the base path
          tmog::walk_prefix(a.nodes, a.missing_bin, root, node, [&](const Node& pd, int) {
            if (flipped(pd, left(pd))) {
              seen_u = seen_u || pd.u == u;
              seen_g = seen_g || (g >= 0 && (meta[pd.u] >> 8) - 1 == g);
            }
            return (int)xr[pd.u];
          });
        ++seen;
        if (!seen_u) {
          const int other = perturbed(node, [&](int x) { return x == u; });
          if (other != leaf) loco_add(dst + (size_t)u * a.C, a, w, a.value + (size_t)other * a.KV, v0);
        }
        if (g >= 0 && !seen_g) {
          const int other = perturbed(node, [&](int x) { return (meta[x] >> 8) - 1 == g; });
          if (other != leaf) loco_add(dst + (size_t)(a.U + g) * a.C, a, w, a.value + (size_t)other * a.KV, v0);
        }
        if (seen == nflip) break;              // nothing below can flip
      }
      node = l ? nd.left : nd.right;
    }
  }
  __syncthreads();
  tmog::store_tile_fp64(a.out + (size_t)blk0 * slots, acc, (size_t)nrow * slots, 1.0 / a.scale);
}

size_t loco_lds_bytes(int rows, int slots, int ustride) {
  return (size_t)rows * slots * 8 + (size_t)ustride * 4 + (size_t)rows * ustride;
}

}  // namespace

extern "C" {

// The device twin of tmog_forest_loco_cpu (common/tmog_abi.h has the contract), all arrays in device memory; nodes
// holds n_nodes records. Returns -3 when one row's tile exceeds the LDS limit, -4 when the launch does not fit
// 32-bit indices (nodes, (row, tree) items of a tile, workgroups).
int tmog_hip_forest_loco(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                         const int32_t* slot_meta, int G, int64_t T, const int64_t* tree_off, const int32_t* nodes,
                         int64_t n_nodes, const float* value, int KV, const float* tree_weight,
                         const int32_t* tree_out, int missing_bin, int C, double scale, double* out,
                         hipStream_t stream) {
  if (n == 0) return 0;
  const int ustride = tmog::ustride_of(U);
  const int64_t slots64 = ((int64_t)U + G + 1) * C;
  if (slots64 * 8 > (int64_t)tmog::kTileLdsLimit) return -3;
  if (n_nodes > 0x7FFFFFFF || T * tmog::kTileMaxRows > 0x7FFFFFFF) return -4;
  const int slots = (int)slots64;
  auto bytes = [&](int rows) { return loco_lds_bytes(rows, slots, ustride); };
  if (bytes(1) > tmog::kTileLdsLimit) return -3;
  const int rows = tmog::pick_tile_rows(bytes);
  LocoArgs a{{Xb, F, n, row_list, U, used, C, scale, missing_bin, rows, ustride}, slot_meta, G, (int)T, tree_off,
             reinterpret_cast<const Node*>(nodes), value, KV, tree_weight, tree_out, out};
  return tmog::launch_lds<forest_loco_kernel>((n + rows - 1) / rows, 1, bytes(rows), stream, a);
}

}  // extern "C"
