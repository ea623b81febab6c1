// Host twin of ../hip/loco_kernels.hip: exact leave-one-column-out sums of a flat forest by path perturbation.
//
// Same contract and the same fixed-point rounding as the kernel (its header has the rule and the bound of the
// scale): every contribution is formed in fp64 from the fp32 tree weight and leaf values, scaled by the power of
// two `scale`, rounded to int64 and summed as integers, so the result does not depend on the order of the trees
// and equals the device's bit for bit. Rows are independent (OpenMP).
#include <cmath>
#include <cstdint>
#include <vector>
#include <omp.h>

#include "common/tmog_abi.h"
#include "common/tree_rules.hpp"

namespace {

struct LocoForest {
  const int32_t* nodes;   // [.][4]: used slot u | split bin + (default_left << 16) | left | right (left < 0: leaf)
  const int32_t* meta;    // [U]: zero bin + ((group + 1) << 8)
  int missing_bin;
};

// The walk from `node` down to its leaf; over(u) says whether slot u's column is replaced by its zero bin.
template <class Over>
inline int64_t loco_walk(const LocoForest& f, const uint8_t* xr, const int32_t* used, int64_t node, Over over) {
  for (;;) {
    const int32_t* nd = f.nodes + node * 4;
    if (nd[2] < 0) return node;
    const int u = nd[0];
    const uint8_t b = over(u) ? (uint8_t)(f.meta[u] & 0xFF) : xr[used[u]];
    node = tmog::goes_left(b, nd[1] & 0xFFFF, [&] { return (nd[1] >> 16) != 0; }, f.missing_bin) ? nd[2] : nd[3];
  }
}

}  // namespace

extern "C" {

int tmog_forest_loco_cpu(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                         const int32_t* slot_meta, int G, int64_t T, const int64_t* tree_off, const int32_t* nodes,
                         const float* value, int KV, const float* tree_weight, const int32_t* tree_out,
                         int missing_bin, int C, double scale, double* out) {
  const LocoForest f{nodes, slot_meta, missing_bin};
  const int64_t slots = (int64_t)(U + G + 1) * C;
  const double inv = 1.0 / scale;
#pragma omp parallel
  {
    std::vector<int64_t> acc(slots);
    std::vector<int64_t> path;      // internal nodes of the base path
    std::vector<uint8_t> flip;
#pragma omp for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t row = row_list ? row_list[i] : i;
      const uint8_t* xr = Xb + row * (int64_t)F;
      for (int64_t k = 0; k < slots; ++k) acc[k] = 0;
      for (int64_t t = 0; t < T; ++t) {
        if (tree_off[t + 1] <= tree_off[t]) continue;
        path.clear();
        flip.clear();
        int64_t node = tree_off[t];
        for (;;) {
          const int32_t* nd = nodes + node * 4;
          if (nd[2] < 0) break;
          const int u = nd[0], sb = nd[1] & 0xFFFF;
          auto dl = [&] { return (nd[1] >> 16) != 0; };
          const bool l = tmog::goes_left(xr[used[u]], sb, dl, missing_bin);
          const bool lz = tmog::goes_left((uint8_t)(slot_meta[u] & 0xFF), sb, dl, missing_bin);
          path.push_back(node);
          flip.push_back(l != lz);
          node = l ? nd[2] : nd[3];
        }
        const int64_t leaf = node;
        const double w = (double)tree_weight[t];
        const float* v0 = value + leaf * KV;
        const int64_t col = tree_out[t];
        for (int c = 0; c < KV; ++c)
          acc[(int64_t)(U + G) * C + col + c] += std::llrint(w * (double)v0[c] * scale);
        auto add = [&](int64_t slot, int64_t other) {
          if (other == leaf) return;
          const float* v1 = value + other * KV;
          for (int c = 0; c < KV; ++c)
            acc[slot * C + col + c] += std::llrint(w * ((double)v1[c] - (double)v0[c]) * scale);
        };
        for (size_t k = 0; k < path.size(); ++k) {
          if (!flip[k]) continue;
          const int u = nodes[path[k] * 4], g = (slot_meta[u] >> 8) - 1;
          bool seen_u = false, seen_g = false;      // a candidate is counted once, from its first flipped node
          for (size_t j = 0; j < k; ++j) {
            if (!flip[j]) continue;
            const int uj = nodes[path[j] * 4];
            seen_u = seen_u || uj == u;
            seen_g = seen_g || (g >= 0 && (slot_meta[uj] >> 8) - 1 == g);
          }
          if (!seen_u) add(u, loco_walk(f, xr, used, path[k], [&](int x) { return x == u; }));
          if (g >= 0 && !seen_g)
            add(U + g, loco_walk(f, xr, used, path[k], [&](int x) { return (slot_meta[x] >> 8) - 1 == g; }));
        }
      }
      double* o = out + i * slots;
      for (int64_t k = 0; k < slots; ++k) o[k] = (double)acc[k] * inv;
    }
  }
  return 0;
}

}  // extern "C"
