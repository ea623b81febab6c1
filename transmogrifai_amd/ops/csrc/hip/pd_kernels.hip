// Exact partial dependence (PDP) and individual conditional expectation (ICE) curves of the tree engine's flat
// forests over the complete bin grid of the requested columns, CDNA4 (gfx950).
//
//   ice[r, q, b, :] = sum_t w_t value_t[leaf_t(x_r with column cols[q] replaced by bin b)]      b in [0, NB)
//   pd_sum[q, b, :] = sum_r ice[r, q, b, :]
//
// Moving column c of a row can change tree t's answer only if c is tested on the path the row already takes, and
// below the first such node the answer as a function of the bin is a step function. Per (row, tree) the kernel
//   1. walks the base path (tmog::walk_to_leaf), adds w_t v[leaf0] to the row's base and counts the nodes of the path
//      whose column is requested;
//   2. walks the base path once more; at the FIRST node of every requested column on the path it produces the
//      column's step function without a stack: starting with bin b = 0 it walks from that node to a leaf, deciding
//      the nodes of the same column by b (tightening hi = min(hi, split_bin) on every left turn) and all others by
//      the row's own bins, emits the leaf for bins b .. hi and goes on with b = hi + 1. The number of walks is the
//      number of distinct reachable leaves; a branch that a repeated column makes unreachable is never visited.
//      The missing bin (the last grid point, when the forest has one) takes one walk of its own along the nodes'
//      default directions.
// "Did this column occur higher up" is answered by walking the prefix of the base path again (only from the second
// requested node of a path on; tmog::walk_prefix of common/forest_walk.hpp): no per-lane array of path nodes,
// nothing in scratch.
//
// A step [b, hi] that ends in another leaf than the base path is stored as a difference: with
// d = tmog::fx_delta(w, v[leaf'], v[leaf0], scale), +d at grid slot b and -d at slot hi + 1 (dropped past the last
// ordinary bin); the missing bin's d goes straight to its slot. The epilogue takes the integer prefix sum over the
// ordinary bins and adds the base. d is rounded once and added and subtracted as the same integer, so the prefix
// sums are exact and the result does not depend on any order: bitwise reproducible and equal to the host twin
// (host/pd_cpu.cpp).
//
// Mapping: the row tile of hip/row_tile.hpp -- a workgroup owns a tile of rows, stages the bins of the used columns
// of its rows in LDS, its lanes take (row, tree) pairs, rows fastest; nodes are the packed records of
// common/forest_walk.hpp. The requested columns are chunked over gridDim.y so that the tile fits LDS. Modes:
//   0 ICE   LDS tile [rows][Qc][NB][C]; stored as fp64 to out[n][Q][NB][C] with plain stores;
//   1 sum   one [Qc][NB][C] tile per workgroup that all its rows add to (the prefix sum is linear, so summing the
//           differences first gives the same integers), added to the int64 buffer out[Q][NB][C] with 64-bit global
//           integer atomics (associative: bitwise reproducible). Only the bases keep a slot per row: every
//           (row, tree) adds to them. A sum epilogue that kept the ICE tile and reduced it over its rows gave the
//           same bits but needed more column chunks and fewer rows per tile; on an MI355X it took 1.41x, 1.74x
//           and 1.84x as long (20 000 records x 20 columns x 64 bins; XGBoost of 200 trees of depth 10, 200 of
//           depth 3, 50 of depth 6), so it is not kept.
//
// Bound of the scale: with S = sum_t |w_t| max |value_t|, a row's base stays within S and every partial sum of its
// differences within 2 S (each tree adds at most |w_t| (|v'| + |v|) to a grid point), a curve value within 3 S.
// ICE mode takes the plan's scale, the power of two with S * scale < 2^61: every value is below 3 * 2^61 < 2^63,
// and intermediate wrap-around of two's-complement sums is harmless while the result fits. The sum takes
// scale / 2^ceil(log2 n), so the sum over n rows obeys the same bound.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip/tmog_hip_abi.h"
#include "hip/row_tile.hpp"
#include "common/forest_walk.hpp"

namespace {

using tmog::kTileThreads;
using Node = tmog::WalkNode;

struct PdArgs : tmog::RowTile {
  const int32_t* slot_of_used;   // [U] index q of the used column among the requested ones, or -1
  int Q;
  int NB;                        // grid points, the missing bin (last) included
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
  int qc;                        // requested columns per chunk
};

__global__ void __launch_bounds__(kTileThreads) forest_pd_kernel(PdArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t blk0 = tmog::tile_first_row(a);
  if (blk0 >= a.n) return;
  const int nrow = tmog::tile_row_count(a, blk0);
  const int q0 = (int)blockIdx.y * a.qc;
  const int nq = min(a.qc, a.Q - q0);
  const int qstride = a.NB * a.C;                    // one requested column of one row
  const size_t rstride = (size_t)a.qc * qstride;     // one row of the tile
  const size_t nacc = (size_t)a.acc_rows * rstride;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);
  unsigned long long* base = acc + nacc;             // [tile_rows][C]
  int32_t* slot = reinterpret_cast<int32_t*>(base + (size_t)a.tile_rows * a.C);
  uint8_t* sbin = reinterpret_cast<uint8_t*>(slot + a.ustride);
  tmog::zero_tile(acc, nacc + (size_t)a.tile_rows * a.C);
  for (int k = threadIdx.x; k < a.U; k += kTileThreads) {
    const int q = a.slot_of_used[k] - q0;
    slot[k] = (q >= 0 && q < nq) ? q : -1;
  }
  tmog::stage_used_bins(a, blk0, nrow, sbin);
  __syncthreads();
  const int items = nrow * a.T;
  for (int it = threadIdx.x; it < items; it += kTileThreads) {
    const int t = it / nrow, r = it - t * nrow;
    const int root = (int)a.tree_off[t];
    if ((int)a.tree_off[t + 1] <= root) continue;
    const uint8_t* xr = sbin + (size_t)r * a.ustride;
    // 1. the base path
    int nreq = 0;
    const int leaf = tmog::walk_to_leaf(a.nodes, a.missing_bin, root, [&](const Node& nd, int) {
      nreq += slot[nd.u] >= 0;
      return (int)xr[nd.u];
    });
    const double w = (double)a.tree_weight[t];
    const float* v0 = a.value + (size_t)leaf * a.KV;
    const int col = a.tree_out[t];
    for (int c = 0; c < a.KV; ++c)
      atomicAdd(base + (size_t)r * a.C + col + c, (unsigned long long)tmog::fx_base(w, v0[c], a.scale));
    if (nreq == 0) continue;
    unsigned long long* tile = acc + (a.acc_rows > 1 ? (size_t)r * rstride : 0) + col;
    // 2. the step function of every requested column from its first node on the path
    int seen = 0, node = root;
    for (;;) {
      const Node nd = a.nodes[node];
      if (nd.leaf()) break;
      const int q = slot[nd.u];
      if (q >= 0) {
        const int u = nd.u;
        bool seen_u = false;
        if (seen > 0)                          // did the column occur higher up on the base path
          tmog::walk_prefix(a.nodes, a.missing_bin, root, node, [&](const Node& pd, int) {
            seen_u = seen_u || pd.u == u;
            return (int)xr[pd.u];
          });
        ++seen;
        if (!seen_u) {
          // the walk from `node` with column u at bin b; hi is lowered to the split bin of every node of that
          // column at which the walk turns left
          auto walk_at = [&](int b, int* hi) {
            return tmog::walk_to_leaf(a.nodes, a.missing_bin, node, [&](const Node& wd, int) {
              if (wd.u != u) return (int)xr[wd.u];
              if (tmog::node_goes_left(b, wd, a.missing_bin)) *hi = min(*hi, wd.split_bin());
              return b;
            });
          };
          unsigned long long* dq = tile + (size_t)q * qstride;
          int b = 0;
          while (b < a.NO) {
            int hi = a.NO - 1;
            const int other = walk_at(b, &hi);
            if (other != leaf) {
              const float* v1 = a.value + (size_t)other * a.KV;
              for (int c = 0; c < a.KV; ++c) {
                const long long d = tmog::fx_delta(w, v1[c], v0[c], a.scale);
                atomicAdd(dq + (size_t)b * a.C + c, (unsigned long long)d);
                if (hi + 1 < a.NO) atomicAdd(dq + (size_t)(hi + 1) * a.C + c, (unsigned long long)(-d));
              }
            }
            b = hi + 1;
          }
          if (a.NO < a.NB) {                   // the missing bin: one walk along the default directions
            int hi = 0;
            const int other = walk_at(a.missing_bin, &hi);
            if (other != leaf) {
              const float* v1 = a.value + (size_t)other * a.KV;
              for (int c = 0; c < a.KV; ++c)
                atomicAdd(dq + (size_t)a.NO * a.C + c, (unsigned long long)tmog::fx_delta(w, v1[c], v0[c], a.scale));
            }
          }
        }
        if (seen == nreq) break;               // no requested column below
      }
      node = tmog::node_goes_left(xr[nd.u], nd, a.missing_bin) ? nd.left : nd.right;
    }
  }
  __syncthreads();
  const int live = nq * qstride;               // the tile row's part this chunk uses
  const int nr = a.mode == 0 ? nrow : 1;
  if (a.mode != 0) {                           // the sum's tile is shared already; its rows' bases add up
    for (int c = threadIdx.x; c < a.C; c += kTileThreads) {
      unsigned long long s = 0ull;
      for (int r = 1; r < nrow; ++r) s += base[(size_t)r * a.C + c];
      base[c] += s;
    }
    __syncthreads();
  }
  // integer prefix sum over the ordinary bins, plus the base
  const int curves = nr * nq * a.C;
  for (int it = threadIdx.x; it < curves; it += kTileThreads) {
    const int r = it / (nq * a.C), rem = it - r * (nq * a.C);
    const int q = rem / a.C, c = rem - q * a.C;
    unsigned long long* p = acc + (size_t)r * rstride + (size_t)q * qstride + c;
    const unsigned long long b0 = base[(size_t)r * a.C + c];
    unsigned long long run = b0;
    for (int b = 0; b < a.NO; ++b) {
      run += p[(size_t)b * a.C];
      p[(size_t)b * a.C] = run;
    }
    if (a.NO < a.NB) p[(size_t)a.NO * a.C] += b0;
  }
  __syncthreads();
  if (a.mode == 0) {
    const double inv = 1.0 / a.scale;
    double* o = reinterpret_cast<double*>(a.out);
    const size_t total = (size_t)nrow * live;
    for (size_t i = threadIdx.x; i < total; i += kTileThreads) {
      const size_t r = i / live, k = i - r * live;
      o[((size_t)(blk0 + r) * a.Q + q0) * qstride + k] = tmog::tile_value(acc[r * rstride + k], inv);
    }
  } else {
    unsigned long long* o = reinterpret_cast<unsigned long long*>(a.out) + (size_t)q0 * qstride;
    for (int i = threadIdx.x; i < live; i += kTileThreads)
      if (acc[i] != 0ull) atomicAdd(o + i, acc[i]);
  }
}

size_t pd_lds_bytes(int rows, int acc_rows, int qc, int64_t qstride, int C, int ustride) {
  return ((size_t)acc_rows * qc * qstride + (size_t)rows * C) * 8 + (size_t)ustride * 4 + (size_t)rows * ustride;
}

}  // namespace

extern "C" {

// The device twin of tmog_forest_pd_cpu (common/tmog_abi.h has the contract), all arrays in device memory; nodes
// holds n_nodes records. mode 0: out is fp64 [n][Q][NB][C]; mode 1: out is a zero-initialised int64 [Q][NB][C] that
// the fixed-point sums at `scale` are added to. Returns -3 when one row x one column x NB x C x 8 bytes exceeds the
// LDS limit, -4 when the launch does not fit 32-bit indices.
int tmog_hip_forest_pd(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                       const int32_t* slot_of_used, int Q, int NB, int64_t T, const int64_t* tree_off,
                       const int32_t* nodes, int64_t n_nodes, const float* value, int KV, const float* tree_weight,
                       const int32_t* tree_out, int missing_bin, int C, double scale, int mode, void* out,
                       hipStream_t stream) {
  if (n == 0 || Q == 0) return 0;
  if (NB < 1 || NB > 256 || mode < 0 || mode > 1) return -1;
  if (missing_bin >= 0 && missing_bin < NB && missing_bin != NB - 1) return -1;
  const int NO = (missing_bin >= 0 && missing_bin < NB) ? NB - 1 : NB;
  const int ustride = tmog::ustride_of(U);
  const int64_t qstride = (int64_t)NB * C;
  if (qstride * 8 > (int64_t)tmog::kTileLdsLimit) return -3;
  if (pd_lds_bytes(1, 1, 1, qstride, C, ustride) > tmog::kTileLdsLimit) return -3;
  if (n_nodes > 0x7FFFFFFF || T * tmog::kTileMaxRows > 0x7FFFFFFF || (int64_t)Q * qstride > 0x7FFFFFFF) return -4;
  // two dimensions to size, rows and requested columns per chunk: down to 16 rows first, then fewer columns, while
  // the tile exceeds the two-workgroup share; then fewer rows while it exceeds the limit
  const bool shared = mode == 1;
  int rows = tmog::kTileMaxRows, qc = Q;
  auto bytes = [&] { return pd_lds_bytes(rows, shared ? 1 : rows, qc, qstride, C, ustride); };
  while (bytes() > tmog::kTileLdsShare && (rows > 16 || qc > 1)) {
    if (rows > 16) rows >>= 1;
    else qc = (qc + 1) >> 1;
  }
  while (rows > 1 && bytes() > tmog::kTileLdsLimit) rows >>= 1;
  if (bytes() > tmog::kTileLdsLimit) return -3;
  const int64_t blocks = (n + rows - 1) / rows;
  const int chunks = (Q + qc - 1) / qc;
  if (blocks > 0x7FFFFFFF || chunks > 65535) return -4;   // ahead of launch_lds' -3, as this entry always answered
  PdArgs a{{Xb, F, n, row_list, U, used, C, scale, missing_bin, rows, ustride}, slot_of_used, Q, NB, NO, (int)T,
           tree_off, reinterpret_cast<const Node*>(nodes), value, KV, tree_weight, tree_out, mode, out,
           shared ? 1 : rows, qc};
  return tmog::launch_lds<forest_pd_kernel>(blocks, chunks, bytes(), stream, a);
}

}  // extern "C"
