// Host twin of ../hip/pd_kernels.hip: exact partial dependence / ICE curves of a flat forest over the complete bin
// grid of the requested columns, by one step function per (row, tree, requested column on the row's path).
//
// Same contract and the same integers as the kernel (its header has the algorithm and the bound of the scale,
// common/forest_walk.hpp the node record, the walk and the rounding rule): a step that ends in another leaf than
// the base path adds d = fx_delta(w, v', v0, scale) at its first bin and -d past its last, the epilogue takes the
// integer prefix sum and adds the base, so the result does not depend on any order and equals the device's bit
// for bit. Rows are independent (OpenMP); the sum mode adds the rows' differences per thread and merges the
// threads' integers.
#include <cstdint>
#include <vector>
#include <omp.h>

#include "common/tmog_abi.h"
#include "common/forest_walk.hpp"

using Node = tmog::WalkNode;

extern "C" {

int tmog_forest_pd_cpu(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                       const int32_t* slot_of_used, int Q, int NB, int64_t T, const int64_t* tree_off,
                       const int32_t* nodes, const float* value, int KV, const float* tree_weight,
                       const int32_t* tree_out, int missing_bin, int C, double scale, int mode, double* out,
                       int64_t* walks) {
  (void)U;
  if (NB < 1 || NB > 256) return -1;
  if (missing_bin >= 0 && missing_bin < NB && missing_bin != NB - 1) return -1;
  const int NO = (missing_bin >= 0 && missing_bin < NB) ? NB - 1 : NB;
  const Node* nd = reinterpret_cast<const Node*>(nodes);
  const int64_t qstride = (int64_t)NB * C, total = (int64_t)Q * qstride;
  const double inv = 1.0 / scale;
  std::vector<int64_t> sum(mode != 0 ? total + C : 0, 0);   // the merged differences, then the bases
  int64_t n_base = 0, n_step = 0;
#pragma omp parallel reduction(+ : n_base, n_step)
  {
    std::vector<int64_t> acc(total, 0), base(C, 0);
    std::vector<int64_t> path;      // internal nodes of the base path
    // the integer prefix sum over the ordinary bins, plus the base
    auto finish = [&](double* o) {
      for (int64_t q = 0; q < Q; ++q)
        for (int c = 0; c < C; ++c) {
          int64_t* p = acc.data() + q * qstride + c;
          int64_t run = base[c];
          for (int b = 0; b < NO; ++b) {
            run = (int64_t)((uint64_t)run + (uint64_t)p[(int64_t)b * C]);
            o[q * qstride + (int64_t)b * C + c] = (double)run * inv;
          }
          if (NO < NB)
            o[q * qstride + (int64_t)NO * C + c] =
                (double)(int64_t)((uint64_t)p[(int64_t)NO * C] + (uint64_t)base[c]) * inv;
        }
    };
#pragma omp for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t row = row_list ? row_list[i] : i;
      const uint8_t* xr = Xb + row * (int64_t)F;
      if (mode == 0) {
        for (auto& x : acc) x = 0;
        for (auto& x : base) x = 0;
      }
      for (int64_t t = 0; t < T; ++t) {
        if (tree_off[t + 1] <= tree_off[t]) continue;
        path.clear();
        const int64_t leaf = tmog::walk_to_leaf(nd, missing_bin, tree_off[t], [&](const Node& x, int64_t node) {
          path.push_back(node);
          return (int)xr[used[x.u]];
        });
        ++n_base;
        const double w = (double)tree_weight[t];
        const float* v0 = value + leaf * KV;
        const int64_t col = tree_out[t];
        for (int c = 0; c < KV; ++c)
          base[col + c] = (int64_t)((uint64_t)base[col + c] + (uint64_t)tmog::fx_base(w, v0[c], scale));
        auto add = [&](int64_t at, int c, int64_t d) { acc[at + c] = (int64_t)((uint64_t)acc[at + c] + (uint64_t)d); };
        for (size_t k = 0; k < path.size(); ++k) {
          const int u = nd[path[k]].u, q = slot_of_used[u];
          if (q < 0) continue;
          bool seen_u = false;            // a column is handled once, at its first node on the path
          for (size_t j = 0; j < k && !seen_u; ++j) seen_u = nd[path[j]].u == u;
          if (seen_u) continue;
          // the walk from the node with column u at bin b; hi is lowered to the split bin of every node of that
          // column at which the walk turns left
          auto walk_at = [&](int b, int* hi) {
            ++n_step;
            return tmog::walk_to_leaf(nd, missing_bin, path[k], [&](const Node& x, int64_t) {
              if (x.u != u) return (int)xr[used[x.u]];
              if (tmog::node_goes_left(b, x, missing_bin) && x.split_bin() < *hi) *hi = x.split_bin();
              return b;
            });
          };
          const int64_t dq = q * qstride + col;
          int b = 0;
          while (b < NO) {
            int hi = NO - 1;
            const int64_t other = walk_at(b, &hi);
            if (other != leaf) {
              const float* v1 = value + other * KV;
              for (int c = 0; c < KV; ++c) {
                const int64_t d = tmog::fx_delta(w, v1[c], v0[c], scale);
                add(dq + (int64_t)b * C, c, d);
                if (hi + 1 < NO) add(dq + (int64_t)(hi + 1) * C, c, (int64_t)(0 - (uint64_t)d));
              }
            }
            b = hi + 1;
          }
          if (NO < NB) {                  // the missing bin: one walk along the default directions
            int hi = 0;
            const int64_t other = walk_at(missing_bin, &hi);
            if (other != leaf) {
              const float* v1 = value + other * KV;
              for (int c = 0; c < KV; ++c)
                add(dq + (int64_t)NO * C, c, tmog::fx_delta(w, v1[c], v0[c], scale));
            }
          }
        }
      }
      if (mode == 0) finish(out + i * total);
    }
    if (mode != 0) {
      // the threads' differences and bases are linear in the rows: merge the integers, finish once
#pragma omp critical
      {
        for (int64_t k = 0; k < total; ++k) sum[k] = (int64_t)((uint64_t)sum[k] + (uint64_t)acc[k]);
        for (int c = 0; c < C; ++c) sum[total + c] = (int64_t)((uint64_t)sum[total + c] + (uint64_t)base[c]);
      }
#pragma omp barrier
#pragma omp single
      {
        for (int64_t k = 0; k < total; ++k) acc[k] = sum[k];
        for (int c = 0; c < C; ++c) base[c] = sum[total + c];
        finish(out);
      }
    }
  }
  if (walks) {
    walks[0] += n_base;
    walks[1] += n_step;
  }
  return 0;
}

}  // extern "C"
