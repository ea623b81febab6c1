// Host twin of ../hip/pd_pair_kernels.hip: exact two-way partial dependence surfaces of a flat forest over the
// complete bin grid of the requested column pairs, by the rectangles of one leaf below the first node of the row's
// path that tests either column.
//
// Same contract and the same integers as the kernel (its header has the mapping and the bound of the scale,
// common/pd_pair_walk.hpp the enumeration and the corners of a rectangle's difference): a rectangle that ends in
// another leaf than the base path adds d = fx_delta(w, v', v0, scale) at its corners, the epilogue takes the integer
// prefix sums (along the second axis, then along the first; the missing bin's line and column one way only) and
// adds the base, so the result does not depend on any order and equals the device's bit for bit. Rows are
// independent (OpenMP); the sum mode adds the rows' differences per thread and merges the threads' integers.
#include <algorithm>
#include <cstdint>
#include <vector>
#include <omp.h>

#include "common/tmog_abi.h"
#include "common/pd_pair_walk.hpp"

using Node = tmog::WalkNode;

extern "C" {

int tmog_forest_pd_pairs_cpu(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                             const int32_t* pair_slots, int Pn, int NB, int64_t T, const int64_t* tree_off,
                             const int32_t* nodes, const float* value, int KV, const float* tree_weight,
                             const int32_t* tree_out, int missing_bin, int C, double scale, int mode, double* out,
                             int64_t* walks) {
  (void)U;
  if (NB < 1 || NB > 256) return -1;
  if (missing_bin >= 0 && missing_bin < NB && missing_bin != NB - 1) return -1;
  const int NO = (missing_bin >= 0 && missing_bin < NB) ? NB - 1 : NB;
  const Node* nd = reinterpret_cast<const Node*>(nodes);
  const int64_t lstride = (int64_t)NB * C, pstride = (int64_t)NB * lstride, total = (int64_t)Pn * pstride;
  const double inv = 1.0 / scale;
  auto wadd = [](int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); };
  std::vector<int64_t> sum(mode != 0 ? total + C : 0, 0);   // the merged differences, then the bases
  int64_t n_base = 0, n_anchor = 0, n_rect = 0;
  // every thread holds the surfaces of all pairs: no more threads than rows
  const int threads = (int)std::min<int64_t>(std::max<int64_t>(n, 1), omp_get_max_threads());
#pragma omp parallel num_threads(threads) reduction(+ : n_base, n_anchor, n_rect)
  {
    std::vector<int64_t> acc(total, 0), base(C, 0);
    // the integer prefix sums over the ordinary bins, plus the base
    auto finish = [&](double* o) {
      for (int64_t p = 0; p < Pn; ++p)
        for (int c = 0; c < C; ++c) {
          int64_t* s = acc.data() + p * pstride + c;
          auto cell = [&](int i, int j) -> int64_t& { return s[i * lstride + (int64_t)j * C]; };
          for (int i = 0; i < NB; ++i) {                     // along the second axis, the missing line included
            int64_t run = 0;
            for (int j = 0; j < NO; ++j) cell(i, j) = run = wadd(run, cell(i, j));
          }
          for (int j = 0; j < NB; ++j) {                     // along the first axis, the missing column included
            int64_t run = 0;
            for (int i = 0; i < NO; ++i) cell(i, j) = run = wadd(run, cell(i, j));
          }
          for (int64_t k = 0; k < (int64_t)NB * NB; ++k)
            o[p * pstride + k * C + c] = (double)wadd(s[k * C], base[c]) * inv;
        }
    };
#pragma omp for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t row = row_list ? row_list[i] : i;
      const uint8_t* xr = Xb + row * (int64_t)F;
      auto own = [&](const Node& x) { return (int)xr[used[x.u]]; };
      if (mode == 0) {
        for (auto& x : acc) x = 0;
        for (auto& x : base) x = 0;
      }
      for (int64_t t = 0; t < T; ++t) {
        if (tree_off[t + 1] <= tree_off[t]) continue;
        const int64_t root = tree_off[t];
        const int64_t leaf = tmog::walk_to_leaf(nd, missing_bin, root, [&](const Node& x, int64_t) { return own(x); });
        ++n_base;
        const double w = (double)tree_weight[t];
        const float* v0 = value + leaf * KV;
        const int64_t col = tree_out[t];
        for (int c = 0; c < KV; ++c) base[col + c] = wadd(base[col + c], tmog::fx_base(w, v0[c], scale));
        for (int64_t p = 0; p < Pn; ++p) {
          const int ua = pair_slots[2 * p], ub = pair_slots[2 * p + 1];
          const int64_t anchor = tmog::pd_pair_anchor(nd, missing_bin, root, ua, ub, own);
          ++n_anchor;
          if (anchor < 0) continue;
          int64_t* dp = acc.data() + p * pstride + col;
          n_rect += tmog::pd_pair_rectangles(
              nd, missing_bin, anchor, ua, ub, NO, NB, 0, NB, own,
              [&](int i_lo, int i_hi, int j_lo, int j_hi, int64_t other) {
                if (other == leaf) return;
                const float* v1 = value + other * KV;
                for (int c = 0; c < KV; ++c) {
                  const int64_t d = tmog::fx_delta(w, v1[c], v0[c], scale);
                  tmog::pd_pair_corners(i_lo, i_hi, j_lo, j_hi, NO, NO, [&](int ci, int cj, bool neg) {
                    int64_t* at = dp + ci * lstride + (int64_t)cj * C + c;
                    *at = wadd(*at, neg ? (int64_t)(0 - (uint64_t)d) : d);
                  });
                }
              });
        }
      }
      if (mode == 0) finish(out + i * total);
    }
    if (mode != 0) {
      // the threads' differences and bases are linear in the rows: merge the integers, finish once
#pragma omp critical
      {
        for (int64_t k = 0; k < total; ++k) sum[k] = wadd(sum[k], acc[k]);
        for (int c = 0; c < C; ++c) sum[total + c] = wadd(sum[total + c], base[c]);
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
    walks[1] += n_anchor;
    walks[2] += n_rect;
  }
  return 0;
}

}  // extern "C"
