// Exact two-way partial dependence surfaces of the tree engine's flat forests over the complete bin grid of the
// requested column pairs, CDNA4 (gfx950).
//
//   ice2[r, p, i, j, :] = sum_t w_t value_t[leaf_t(x_r with column a_p replaced by bin i and b_p by bin j)]
//   sum2[p, i, j, :]    = sum_r ice2[r, p, i, j, :]                                   i, j in [0, NB)
//
// Moving two columns of a row can change tree t's answer only if one of them is tested on the path the row already
// takes, and below the first such node (the anchor) the answer is piecewise constant on rectangles of the grid.
// Per (row, tree) the kernel walks the base path (tmog::walk_to_leaf) and adds w_t v[leaf0] to the row's base; per
// pair it finds the anchor (tmog::pd_pair_anchor) and tiles the grid below it by strips
// (tmog::pd_pair_rectangles of common/pd_pair_walk.hpp, which has the argument): a handful of walks per
// (row, tree, pair) instead of NB^2 rescorings, no per-lane array of path nodes, nothing in scratch.
//
// A rectangle that ends in another leaf than the base path is stored as a 2-D integer difference: with
// d = tmog::fx_delta(w, v[leaf'], v[leaf0], scale), +d at its first cell, -d past its last bin on either axis and
// +d past both (tmog::pd_pair_corners; corners past the last ordinary bin are dropped). The missing bin, the last
// point of both axes when the forest has one, stays out of the 2-D differences: the last column takes 1-D
// differences along the first axis, the last line 1-D differences along the second, the corner its d directly.
// The epilogue takes the integer prefix sums along the second axis (every line), then along the first (every
// column, ordinary lines only), and adds the base. d is rounded once and added and subtracted as the same integer,
// so the prefix sums are exact and the result does not depend on any order: bitwise reproducible and equal to the
// host twin (host/pd_pairs_cpu.cpp).
//
// Mapping: the row tile of hip/row_tile.hpp -- a workgroup owns a tile of rows, stages the bins of the used columns
// of its rows in LDS, its lanes take (row, tree) items, rows fastest; nodes are the packed records of
// common/forest_walk.hpp. A surface is NB * NB * C * 8 bytes (33.8 KB at 65 bins, 5.2 MB at 256 bins x 10 output
// columns), so gridDim.y chunks over the pairs AND over the first grid axis: a chunk owns the lines [i0, i1) of
// its pairs. It starts its strips at line i0 and ends them at i1 (any first line gives a valid tiling, and every
// tiling gives the same integers), so a line chunk repeats the anchor search but not the other chunks' walks, and
// its prefix sum along the first axis stays inside the chunk. The missing line belongs to the chunk that holds
// i = NO. Modes:
//   0 per-record surfaces   LDS tile [rows][pc][lc][NB][C]; stored as fp64 to out[n][Pn][NB][NB][C];
//   1 sum                   one [pc][lc][NB][C] tile per workgroup that all its rows add to (the prefix sums are
//                           linear), added to the int64 buffer out[Pn][NB][NB][C] with 64-bit global integer
//                           atomics, nonzero entries only. Only the bases keep a slot per row.
//
// Bound of the scale: each (row, tree) puts exactly one delta on a cell, as on a point of a 1-D curve, so the
// bound of pd_kernels.hip carries over: with S = sum_t |w_t| max |value_t| a row's base stays within S and a cell
// within 3 S; mode 0 takes the plan's scale (S * scale < 2^61), the sum scale / 2^ceil(log2 n). Partial sums of a
// 2-D difference can leave that range on the way; two's-complement wrap-around is harmless while the result fits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip/tmog_hip_abi.h"
#include "hip/row_tile.hpp"
#include "common/pd_pair_walk.hpp"

namespace {

using tmog::kTileThreads;
using Node = tmog::WalkNode;

struct PdPairArgs : tmog::RowTile {
  const int32_t* pair_slots;     // [Pn][2] slots (ua, ub) of the pair's columns among the used ones, or -1
  int Pn;
  int NB;                        // grid points per axis, the missing bin (last) included
  int NO;                        // ordinary bins: NB, or NB - 1 with a missing bin
  int T;
  const int64_t* tree_off;
  const Node* nodes;
  const float* value;
  int KV;
  const float* tree_weight;
  const int32_t* tree_out;
  int mode;
  void* out;
  int acc_rows;                  // rows of the LDS tile: tile_rows, or 1 (the sum)
  int pc;                        // pairs per chunk
  int lc;                        // grid lines (first axis) per chunk
  int nlc;                       // line chunks per pair chunk
};

__global__ void __launch_bounds__(kTileThreads) forest_pd_pairs_kernel(PdPairArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t blk0 = tmog::tile_first_row(a);
  if (blk0 >= a.n) return;
  const int nrow = tmog::tile_row_count(a, blk0);
  const int pci = (int)blockIdx.y / a.nlc, lci = (int)blockIdx.y - pci * a.nlc;
  const int p0 = pci * a.pc, np = min(a.pc, a.Pn - p0);
  const int i0 = lci * a.lc, i1 = min(i0 + a.lc, a.NB), nl = i1 - i0;
  const int o_end = min(i1, a.NO);                   // end of the chunk's ordinary lines
  const int lstride = a.NB * a.C;                    // one grid line
  const size_t pstride = (size_t)a.lc * lstride;     // one pair of one row of the tile
  const size_t rstride = (size_t)a.pc * pstride;     // one row of the tile
  const size_t nacc = (size_t)a.acc_rows * rstride;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);
  unsigned long long* base = acc + nacc;             // [tile_rows][C]
  uint8_t* sbin = reinterpret_cast<uint8_t*>(base + (size_t)a.tile_rows * a.C);
  tmog::zero_tile(acc, nacc + (size_t)a.tile_rows * a.C);
  tmog::stage_used_bins(a, blk0, nrow, sbin);
  __syncthreads();
  const int items = nrow * a.T;
  for (int it = threadIdx.x; it < items; it += kTileThreads) {
    const int t = it / nrow, r = it - t * nrow;
    const int root = (int)a.tree_off[t];
    if ((int)a.tree_off[t + 1] <= root) continue;
    const uint8_t* xr = sbin + (size_t)r * a.ustride;
    auto own = [&](const Node& nd) { return (int)xr[nd.u]; };
    const int leaf = tmog::walk_to_leaf(a.nodes, a.missing_bin, root, [&](const Node& nd, int) { return own(nd); });
    const double w = (double)a.tree_weight[t];
    const float* v0 = a.value + (size_t)leaf * a.KV;
    const int col = a.tree_out[t];
    for (int c = 0; c < a.KV; ++c)
      atomicAdd(base + (size_t)r * a.C + col + c, (unsigned long long)tmog::fx_base(w, v0[c], a.scale));
    unsigned long long* tile = acc + (a.acc_rows > 1 ? (size_t)r * rstride : 0) + col;
    for (int p = 0; p < np; ++p) {
      const int ua = a.pair_slots[2 * (p0 + p)], ub = a.pair_slots[2 * (p0 + p) + 1];
      const int anchor = tmog::pd_pair_anchor(a.nodes, a.missing_bin, root, ua, ub, own);
      if (anchor < 0) continue;
      unsigned long long* dp = tile + (size_t)p * pstride;
      tmog::pd_pair_rectangles(a.nodes, a.missing_bin, anchor, ua, ub, a.NO, a.NB, i0, i1, own,
                               [&](int i_lo, int i_hi, int j_lo, int j_hi, int other) {
        if (other == leaf) return;
        const float* v1 = a.value + (size_t)other * a.KV;
        for (int c = 0; c < a.KV; ++c) {
          const unsigned long long d = (unsigned long long)tmog::fx_delta(w, v1[c], v0[c], a.scale);
          tmog::pd_pair_corners(i_lo, i_hi, j_lo, j_hi, a.NO, o_end, [&](int ci, int cj, bool neg) {
            atomicAdd(dp + (size_t)(ci - i0) * lstride + cj * a.C + c, neg ? 0ull - d : d);
          });
        }
      });
    }
  }
  __syncthreads();
  const int nr = a.mode == 0 ? nrow : 1;
  if (a.mode != 0) {                           // the sum's tile is shared already; its rows' bases add up
    for (int c = threadIdx.x; c < a.C; c += kTileThreads) {
      unsigned long long s = 0ull;
      for (int r = 1; r < nrow; ++r) s += base[(size_t)r * a.C + c];
      base[c] += s;
    }
  }
  // integer prefix sums: along the second axis on every line of the chunk (the missing line included) ...
  const int nline = nr * np * nl * a.C;
  for (int it = threadIdx.x; it < nline; it += kTileThreads) {
    const int c = it % a.C, k = it / a.C;
    const int l = k % nl, rp = k / nl;
    const int p = rp % np, r = rp / np;
    unsigned long long* s = acc + (size_t)r * rstride + (size_t)p * pstride + (size_t)l * lstride + c;
    unsigned long long run = 0ull;
    for (int j = 0; j < a.NO; ++j) {
      run += s[(size_t)j * a.C];
      s[(size_t)j * a.C] = run;
    }
  }
  __syncthreads();
  // ... then along the first axis on every column (the missing column included), ordinary lines only
  const int ncol = nr * np * lstride;
  for (int it = threadIdx.x; it < ncol; it += kTileThreads) {
    const int jc = it % lstride, rp = it / lstride;
    const int p = rp % np, r = rp / np;
    unsigned long long* s = acc + (size_t)r * rstride + (size_t)p * pstride + jc;
    unsigned long long run = 0ull;
    for (int l = 0; l < o_end - i0; ++l) {
      run += s[(size_t)l * lstride];
      s[(size_t)l * lstride] = run;
    }
  }
  __syncthreads();
  // the chunk's lines of a surface are contiguous in the tile and in the result
  const size_t live = (size_t)nl * lstride;
  const size_t surface = (size_t)a.NB * lstride;
  const size_t total = (size_t)nr * np * live;
  if (a.mode == 0) {
    const double inv = 1.0 / a.scale;
    double* o = reinterpret_cast<double*>(a.out);
    for (size_t i = threadIdx.x; i < total; i += kTileThreads) {
      const size_t k = i % live, rp = i / live;
      const size_t p = rp % np, r = rp / np;
      const unsigned long long v = acc[r * rstride + p * pstride + k] + base[r * a.C + k % a.C];
      o[((size_t)(blk0 + r) * a.Pn + p0 + p) * surface + (size_t)i0 * lstride + k] = tmog::tile_value(v, inv);
    }
  } else {
    unsigned long long* o = reinterpret_cast<unsigned long long*>(a.out);
    for (size_t i = threadIdx.x; i < total; i += kTileThreads) {
      const size_t k = i % live, p = i / live;
      const unsigned long long v = acc[p * pstride + k] + base[k % a.C];
      if (v != 0ull) atomicAdd(o + (p0 + p) * surface + (size_t)i0 * lstride + k, v);
    }
  }
}

size_t pd_pairs_lds_bytes(int rows, int acc_rows, int pc, int lc, int64_t lstride, int C, int ustride) {
  return ((size_t)acc_rows * pc * lc * lstride + (size_t)rows * C) * 8 + (size_t)rows * ustride;
}

}  // namespace

extern "C" {

// The device twin of tmog_forest_pd_pairs_cpu (common/tmog_abi.h has the contract), all arrays in device memory;
// nodes holds n_nodes records. mode 0: out is fp64 [n][Pn][NB][NB][C]; mode 1: out is a zero-initialised int64
// [Pn][NB][NB][C] that the fixed-point sums at `scale` are added to. Returns -1 for bad arguments, -3 when one
// row x one grid line (NB x C x 8 bytes plus staging) exceeds the LDS limit, -4 when the launch does not fit 32-bit
// indices or the grid.
int tmog_hip_forest_pd_pairs(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                             const int32_t* pair_slots, int Pn, int NB, int64_t T, const int64_t* tree_off,
                             const int32_t* nodes, int64_t n_nodes, const float* value, int KV,
                             const float* tree_weight, const int32_t* tree_out, int missing_bin, int C, double scale,
                             int mode, void* out, hipStream_t stream) {
  if (n == 0 || Pn == 0) return 0;
  if (NB < 1 || NB > 256 || mode < 0 || mode > 1 || Pn < 0) return -1;
  if (missing_bin >= 0 && missing_bin < NB && missing_bin != NB - 1) return -1;
  const int NO = (missing_bin >= 0 && missing_bin < NB) ? NB - 1 : NB;
  const int ustride = tmog::ustride_of(U);
  const int64_t lstride = (int64_t)NB * C;
  if (lstride * 8 > (int64_t)tmog::kTileLdsLimit) return -3;
  if (pd_pairs_lds_bytes(1, 1, 1, 1, lstride, C, ustride) > tmog::kTileLdsLimit) return -3;
  if (n_nodes > 0x7FFFFFFF || T * tmog::kTileMaxRows > 0x7FFFFFFF || (int64_t)Pn * NB * lstride > 0x7FFFFFFF)
    return -4;
  // three dimensions to size, rows, pairs per chunk and lines per chunk: down to 16 rows first, then fewer pairs,
  // then fewer lines, while the tile exceeds the two-workgroup share; then fewer rows while it exceeds the limit
  const bool shared = mode == 1;
  int rows = tmog::kTileMaxRows, pc = Pn, lc = NB;
  auto bytes = [&] { return pd_pairs_lds_bytes(rows, shared ? 1 : rows, pc, lc, lstride, C, ustride); };
  while (bytes() > tmog::kTileLdsShare && (rows > 16 || pc > 1 || lc > 1)) {
    if (rows > 16) rows >>= 1;
    else if (pc > 1) pc = (pc + 1) >> 1;
    else lc = (lc + 1) >> 1;
  }
  while (rows > 1 && bytes() > tmog::kTileLdsLimit) rows >>= 1;
  if (bytes() > tmog::kTileLdsLimit) return -3;
  const int64_t blocks = (n + rows - 1) / rows;
  const int nlc = (NB + lc - 1) / lc;
  const int64_t chunks = (int64_t)((Pn + pc - 1) / pc) * nlc;
  if (blocks > 0x7FFFFFFF || chunks > 65535) return -4;
  PdPairArgs a{{Xb, F, n, row_list, U, used, C, scale, missing_bin, rows, ustride}, pair_slots, Pn, NB, NO, (int)T,
               tree_off, reinterpret_cast<const Node*>(nodes), value, KV, tree_weight, tree_out, mode, out,
               shared ? 1 : rows, pc, lc, nlc};
  return tmog::launch_lds<forest_pd_pairs_kernel>(blocks, chunks, bytes(), stream, a);
}

}  // extern "C"
