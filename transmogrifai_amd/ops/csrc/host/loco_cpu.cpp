// Host twin of ../hip/loco_kernels.hip: exact leave-one-column-out sums of a flat forest by path perturbation.
//
// Same contract and the same fixed-point rounding as the kernel (its header has the algorithm and the bound of the
// scale, common/forest_walk.hpp the node record, the walk and the rounding rule): the contributions are summed as
// integers, so the result does not depend on the order of the trees and equals the device's bit for bit. Rows are
// independent (OpenMP).
#include <cstdint>
#include <vector>
#include <omp.h>

#include "common/tmog_abi.h"
#include "common/forest_walk.hpp"

using Node = tmog::WalkNode;

extern "C" {

int tmog_forest_loco_cpu(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                         const int32_t* slot_meta, int G, int64_t T, const int64_t* tree_off, const int32_t* nodes,
                         const float* value, int KV, const float* tree_weight, const int32_t* tree_out,
                         int missing_bin, int C, double scale, double* out) {
  const Node* nd = reinterpret_cast<const Node*>(nodes);
  const int64_t slots = (int64_t)(U + G + 1) * C;
  const double inv = 1.0 / scale;
#pragma omp parallel
  {
    std::vector<int64_t> acc(slots);
    std::vector<int64_t> path;      // the flipped internal nodes of the base path
#pragma omp for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t row = row_list ? row_list[i] : i;
      const uint8_t* xr = Xb + row * (int64_t)F;
      for (int64_t k = 0; k < slots; ++k) acc[k] = 0;
      for (int64_t t = 0; t < T; ++t) {
        if (tree_off[t + 1] <= tree_off[t]) continue;
        path.clear();
        const int64_t leaf = tmog::walk_to_leaf(nd, missing_bin, tree_off[t], [&](const Node& x, int64_t node) {
          const int b = xr[used[x.u]];
          if (tmog::node_goes_left(b, x, missing_bin) != tmog::node_goes_left(slot_meta[x.u] & 0xFF, x, missing_bin))
            path.push_back(node);
          return b;
        });
        const double w = (double)tree_weight[t];
        const float* v0 = value + leaf * KV;
        const int64_t col = tree_out[t];
        for (int c = 0; c < KV; ++c) acc[(int64_t)(U + G) * C + col + c] += tmog::fx_base(w, v0[c], scale);
        // the walk from `node` with the zero bin at the slots that over(u) names, added to `slot` if it ends elsewhere
        auto add = [&](int64_t slot, int64_t node, auto over) {
          const int64_t other = tmog::walk_to_leaf(nd, missing_bin, node, [&](const Node& x, int64_t) {
            return over(x.u) ? (slot_meta[x.u] & 0xFF) : (int)xr[used[x.u]];
          });
          if (other == leaf) return;
          const float* v1 = value + other * KV;
          for (int c = 0; c < KV; ++c) acc[slot * C + col + c] += tmog::fx_delta(w, v1[c], v0[c], scale);
        };
        for (size_t k = 0; k < path.size(); ++k) {
          const int u = nd[path[k]].u, g = (slot_meta[u] >> 8) - 1;
          bool seen_u = false, seen_g = false;      // a candidate is counted once, from its first flipped node
          for (size_t j = 0; j < k; ++j) {
            const int uj = nd[path[j]].u;
            seen_u = seen_u || uj == u;
            seen_g = seen_g || (g >= 0 && (slot_meta[uj] >> 8) - 1 == g);
          }
          if (!seen_u) add(u, path[k], [&](int x) { return x == u; });
          if (g >= 0 && !seen_g) add(U + g, path[k], [&](int x) { return (slot_meta[x] >> 8) - 1 == g; });
        }
      }
      double* o = out + i * slots;
      for (int64_t k = 0; k < slots; ++k) o[k] = (double)acc[k] * inv;
    }
  }
  return 0;
}

}  // extern "C"
