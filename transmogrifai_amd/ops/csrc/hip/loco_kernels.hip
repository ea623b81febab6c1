// Exact leave-one-column-out (LOCO) sums of the tree engine's flat forests by path perturbation, CDNA4 (gfx950).
//
// Replacing column c of a row by the bin of the value 0 can change tree t's answer only if c is tested on the path
// the row already takes through t. Per (row, tree) the kernel therefore
//   1. walks the base path (tmog::goes_left) and adds w_t v[leaf] to the base slot; a node of that path is FLIPPED
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
// tree (node records are 16-byte loads shared through L2 / L1, diverging only with depth). Nodes come as one packed
// record (slot u, bin | default_left << 16, left, right) prepared by models/tree_engine.py forest_loco_plan.
//
// Accumulation is order-independent, hence bitwise reproducible and equal to the host twin (host/loco_cpu.cpp):
// each contribution is formed in fp64 from the fp32 weight and leaf values without contraction, scaled by a power
// of two, rounded to int64 and added to the workgroup's LDS tile [rows][U + G + 1][C] with 64-bit LDS integer
// atomics; the tile is converted to fp64 and written with plain stores at the end.
// Bound of the scale: with S = sum_t |w_t| max |value_t|, the base slot's partial sums stay within S and a delta
// slot's within 2 S (each tree adds at most |w_t| (|v'| + |v|)); scale is the power of two with S * scale < 2^61,
// so every partial sum is below 2^62 in magnitude and the at most T roundings of 1/2 each cannot reach 2^63.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip/tmog_hip_abi.h"
#include "common/tree_rules.hpp"

namespace {

constexpr int LOCO_THREADS = 512;
constexpr int LOCO_MAX_ROWS = 64;
constexpr size_t LOCO_LDS_LIMIT = 160 * 1024;
constexpr size_t LOCO_LDS_SHARE = 80 * 1024;   // two workgroups per CU while the tile stays >= 16 rows

struct LocoArgs {
  const uint8_t* Xb;
  int F;
  int64_t n;
  const int32_t* row_list;
  int U;
  const int32_t* used;
  const int32_t* slot_meta;   // [U] zero bin | (group + 1) << 8
  int G;
  int T;
  const int64_t* tree_off;
  const int4* nodes;          // (u, bin | default_left << 16, left, right)
  const float* value;
  int KV;
  const float* tree_weight;
  const int32_t* tree_out;
  int missing_bin;
  int C;
  double scale;
  double* out;
  int tile_rows;
  int ustride;                // bytes per staged row (U rounded up to 4)
};

__device__ __forceinline__ bool loco_left(int bin, const int4& nd, int missing_bin) {
  return tmog::goes_left((uint8_t)bin, nd.y & 0xFFFF, [&] { return (nd.y >> 16) != 0; }, missing_bin);
}

// The walk from `node` to its leaf for one staged row; over(u) says whether slot u's column takes its zero bin.
template <class Over>
__device__ __forceinline__ int loco_walk(const LocoArgs& a, const uint8_t* xr, const int32_t* meta, int node,
                                         Over over) {
  for (;;) {
    const int4 nd = a.nodes[node];
    if (nd.z < 0) return node;
    const int b = over(nd.x) ? (meta[nd.x] & 0xFF) : (int)xr[nd.x];
    node = loco_left(b, nd, a.missing_bin) ? nd.z : nd.w;
  }
}

__device__ __forceinline__ void loco_add(unsigned long long* dst, const LocoArgs& a, double w, const float* v1,
                                         const float* v0) {
#pragma clang fp contract(off)
  for (int c = 0; c < a.KV; ++c) {
    const double d = v0 ? (double)v1[c] - (double)v0[c] : (double)v1[c];
    atomicAdd(dst + c, (unsigned long long)__double2ll_rn(w * d * a.scale));
  }
}

__global__ void __launch_bounds__(LOCO_THREADS) forest_loco_kernel(LocoArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t blk0 = (int64_t)blockIdx.x * a.tile_rows;
  if (blk0 >= a.n) return;
  const int nrow = (int)min((int64_t)a.tile_rows, a.n - blk0);
  const int slots = (a.U + a.G + 1) * a.C;
  const size_t nacc = (size_t)a.tile_rows * slots;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);
  int32_t* meta = reinterpret_cast<int32_t*>(smem + nacc * 8);
  uint8_t* sbin = smem + nacc * 8 + (size_t)a.ustride * 4;
  for (size_t i = threadIdx.x; i < nacc; i += LOCO_THREADS) acc[i] = 0ull;
  for (int k = threadIdx.x; k < a.U; k += LOCO_THREADS) meta[k] = a.slot_meta[k];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < nrow; r += LOCO_THREADS / 64) {
    const int64_t row = a.row_list ? a.row_list[blk0 + r] : (blk0 + r);
    const uint8_t* src = a.Xb + row * (int64_t)a.F;
    for (int k = lane; k < a.U; k += 64) sbin[(size_t)r * a.ustride + k] = src[a.used[k]];
  }
  __syncthreads();
  const int items = nrow * a.T;
  for (int it = threadIdx.x; it < items; it += LOCO_THREADS) {
    const int t = it / nrow, r = it - t * nrow;
    const int root = (int)a.tree_off[t];
    if ((int)a.tree_off[t + 1] <= root) continue;
    const uint8_t* xr = sbin + (size_t)r * a.ustride;
    // 1. the base path
    int node = root, nflip = 0;
    for (;;) {
      const int4 nd = a.nodes[node];
      if (nd.z < 0) break;
      const bool l = loco_left(xr[nd.x], nd, a.missing_bin);
      nflip += l != loco_left(meta[nd.x] & 0xFF, nd, a.missing_bin);
      node = l ? nd.z : nd.w;
    }
    const int leaf = node;
    const double w = (double)a.tree_weight[t];
    const float* v0 = a.value + (size_t)leaf * a.KV;
    unsigned long long* dst = acc + (size_t)r * slots + a.tree_out[t];
    loco_add(dst + (size_t)(a.U + a.G) * a.C, a, w, v0, nullptr);
    if (nflip == 0) continue;
    // 2. every candidate from its first flipped node
    int seen = 0;
    node = root;
    for (;;) {
      const int4 nd = a.nodes[node];
      if (nd.z < 0) break;
      const bool l = loco_left(xr[nd.x], nd, a.missing_bin);
      if (l != loco_left(meta[nd.x] & 0xFF, nd, a.missing_bin)) {
        const int u = nd.x, g = (meta[u] >> 8) - 1;
        bool seen_u = false, seen_g = false;
        if (seen > 0) {                        // was the candidate flipped higher up on the base path
          int p = root;
          while (p != node) {
            const int4 pd = a.nodes[p];
            const bool pl = loco_left(xr[pd.x], pd, a.missing_bin);
            if (pl != loco_left(meta[pd.x] & 0xFF, pd, a.missing_bin)) {
              seen_u = seen_u || pd.x == u;
              seen_g = seen_g || (g >= 0 && (meta[pd.x] >> 8) - 1 == g);
            }
            p = pl ? pd.z : pd.w;
          }
        }
        ++seen;
        if (!seen_u) {
          const int other = loco_walk(a, xr, meta, node, [&](int x) { return x == u; });
          if (other != leaf) loco_add(dst + (size_t)u * a.C, a, w, a.value + (size_t)other * a.KV, v0);
        }
        if (g >= 0 && !seen_g) {
          const int other = loco_walk(a, xr, meta, node, [&](int x) { return (meta[x] >> 8) - 1 == g; });
          if (other != leaf) loco_add(dst + (size_t)(a.U + g) * a.C, a, w, a.value + (size_t)other * a.KV, v0);
        }
        if (seen == nflip) break;              // nothing below can flip
      }
      node = l ? nd.z : nd.w;
    }
  }
  __syncthreads();
  const size_t nout = (size_t)nrow * slots;
  const double inv = 1.0 / a.scale;
  double* o = a.out + (size_t)blk0 * slots;
  for (size_t i = threadIdx.x; i < nout; i += LOCO_THREADS) o[i] = (double)(long long)acc[i] * inv;
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
  const int ustride = (U + 3) & ~3;
  const int64_t slots64 = ((int64_t)U + G + 1) * C;
  if (slots64 * 8 > (int64_t)LOCO_LDS_LIMIT) return -3;
  if (n_nodes > 0x7FFFFFFF || T * LOCO_MAX_ROWS > 0x7FFFFFFF) return -4;
  const int slots = (int)slots64;
  if (loco_lds_bytes(1, slots, ustride) > LOCO_LDS_LIMIT) return -3;
  int rows = LOCO_MAX_ROWS;
  while (rows > 16 && loco_lds_bytes(rows, slots, ustride) > LOCO_LDS_SHARE) rows >>= 1;
  while (rows > 1 && loco_lds_bytes(rows, slots, ustride) > LOCO_LDS_LIMIT) rows >>= 1;
  LocoArgs a{Xb, F, n, row_list, U, used, slot_meta, G, (int)T, tree_off, reinterpret_cast<const int4*>(nodes),
             value, KV, tree_weight, tree_out, missing_bin, C, scale, out, rows, ustride};
  const size_t lds = loco_lds_bytes(rows, slots, ustride);
  static const bool lds_attr = hipFuncSetAttribute((const void*)forest_loco_kernel,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)LOCO_LDS_LIMIT) == hipSuccess;   // once per process
  if (lds > 64 * 1024 && !lds_attr) return -3;
  const int64_t blocks = (n + rows - 1) / rows;
  if (blocks > 0x7FFFFFFF) return -4;
  hipLaunchKernelGGL(forest_loco_kernel, dim3((unsigned)blocks), dim3(LOCO_THREADS), lds, stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
