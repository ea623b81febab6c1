// Row partition and leaf collection of the histogram tree engine for CDNA4 (gfx950): what moves a level's row
// entries once tree_split_kernels.hip has decided the splits (layout contract: tree_hist_kernels.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common/tree_rules.hpp"
#include "hip/tmog_hip_abi.h"
#include "hip/tree_dev.hpp"

namespace {

using namespace tmog;   // common/tree_rules.hpp: the split / growth rules shared with the CPU twin

// ----------------------------------------------------------------------------------- partition
// (work items: PartItem, common/tmog_abi.h)
constexpr int PART_U = 4;

// One-pass partition (replaces count + scatter): every chunk of every node reads its split decision
// straight from split_find's device output (no host round trip before the partition), and each
// 256-row step reserves its left / right output slots with two atomics on the node's cursors: left
// entries fill the node's own range [begin, begin + nl) upward, right entries fill it downward from
// the end. The order inside a child is not stable, which changes nothing downstream: histograms are
// exact integer sums (order-independent) and leaf assignments are keyed by row id. Nodes that do not
// split (feat < 0) are skipped; their ranges are collected as leaves from the input buffer.
__global__ void __launch_bounds__(256) partition_fused_kernel(
    const uint8_t* __restrict__ Xb, int F, const uint32_t* __restrict__ rows_in, uint32_t* __restrict__ rows_out,
    const PartItem* __restrict__ items, const int64_t* __restrict__ node_begin, const int64_t* __restrict__ node_count,
    const int32_t* __restrict__ split_feat, const int32_t* __restrict__ split_bin, const uint8_t* __restrict__ dl,
    const float* __restrict__ node_params, const float* __restrict__ split_gain, int missing_bin,
    unsigned long long* __restrict__ cursors, const uint8_t* __restrict__ XbT, int64_t Nt,
    const int2* __restrict__ gh_in, int2* __restrict__ gh_out, const int* __restrict__ dcount, int wide) {
  if (dcount != nullptr && (int)blockIdx.x >= *dcount) return;
  const PartItem it = items[blockIdx.x];
  const int j = it.node;
  const int f = split_feat[j], sb = split_bin[j];
  // the host's split decision, evaluated identically: splittable node, a split found, gain above eps
  const float* P = node_params + (int64_t)j * kPrmStride;
  if (!split_accepted(P, f, split_gain + j)) return;
  const bool d = dl[j] != 0;
  const int64_t nb = node_begin[j], nend = nb + node_count[j];
  // PART_U rows per thread per pass: their row / bin loads are all in flight together and one pair
  // of cursor atomics reserves the slots of 256 * PART_U rows (the dependent load -> load -> atomic
  // chain runs once per pass instead of once per 256 rows)
  __shared__ int s_cnt[PART_U][4];
  __shared__ unsigned long long s_base[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t base = 0; base < it.count; base += (int64_t)blockDim.x * PART_U) {
    uint32_t e[PART_U];
    int2 q[PART_U];
    bool vd[PART_U], lf[PART_U];
#pragma unroll
    for (int u = 0; u < PART_U; ++u) {
      const int64_t i = base + (int64_t)u * blockDim.x + threadIdx.x;
      vd[u] = i < it.count;
      e[u] = rows_in[it.begin + (vd[u] ? i : 0)];     // unpredicated: row 0 of the item is valid
      if (gh_in) q[u] = gh_in[it.begin + (vd[u] ? i : 0)];   // the staged (g, h) move with their entry
    }
    uint8_t bn[PART_U];
#pragma unroll
    for (int u = 0; u < PART_U; ++u)
      bn[u] = XbT ? XbT[(int64_t)f * Nt + ent_row(e[u], wide)] : Xb[(int64_t)ent_row(e[u], wide) * F + f];
    int wpre[PART_U];
#pragma unroll
    for (int u = 0; u < PART_U; ++u) {
      lf[u] = vd[u] && goes_left(bn[u], sb, [&] { return d; }, missing_bin);
      const unsigned long long m = __ballot(lf[u]);
      wpre[u] = __popcll(m & below);
      if (lane == 0) s_cnt[u][wave] = __popcll(m);
    }
    __syncthreads();
    int tot = 0, before[PART_U];
#pragma unroll
    for (int u = 0; u < PART_U; ++u) {
      int b = tot;
      for (int w = 0; w < 4; ++w) {
        if (w < wave) b += s_cnt[u][w];
        tot += s_cnt[u][w];
      }
      before[u] = b;
    }
    const int nvalid = (int)min((int64_t)blockDim.x * PART_U, it.count - base);
    if (threadIdx.x == 0) {
      s_base[0] = atomicAdd(cursors + 2 * j, (unsigned long long)tot);
      s_base[1] = atomicAdd(cursors + 2 * j + 1, (unsigned long long)(nvalid - tot));
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PART_U; ++u) {
      if (!vd[u]) continue;
      const int lpos = before[u] + wpre[u];               // left rows before this one (row order)
      const int idx = u * (int)blockDim.x + (int)threadIdx.x;  // rows before this one
      // guarded: a slot outside the node's range (impossible unless the cursors were not reset) is
      // dropped; the host checks every node's left + right count against its size
      const int64_t pos = lf[u] ? nb + (int64_t)s_base[0] + lpos : nend - 1 - (int64_t)s_base[1] - (idx - lpos);
      if (pos >= nb && pos < nend) {
        rows_out[pos] = e[u];
        if (gh_in) gh_out[pos] = q[u];
      }
    }
    __syncthreads();
  }
}

// ----------------------------------------------------------------------------- leaf collection
// When a node stops splitting, its row entries (still contiguous in the level's row buffer) are
// copied out with the node id: after the last level every training entry sits in exactly one
// (entry, leaf) pair, so boosting updates its margins by a gather instead of re-walking the tree.
// (Work items: LeafItem, common/tmog_abi.h.)
__global__ void __launch_bounds__(256) leaf_collect_kernel(const uint32_t* __restrict__ rows,
                                                           const uint32_t* __restrict__ rows_alt,
                                                           const LeafItem* __restrict__ items,
                                                           uint32_t* __restrict__ out_rows,
                                                           int32_t* __restrict__ out_gid,
                                                           const int* __restrict__ dcount) {
  if (dcount != nullptr && (int)blockIdx.x >= *dcount) return;
  const LeafItem it = items[blockIdx.x];
  const uint32_t* src = (it.buf && rows_alt) ? rows_alt : rows;
  for (int64_t i = threadIdx.x; i < it.count; i += blockDim.x) {
    out_rows[it.out + i] = src[it.begin + i];
    out_gid[it.out + i] = it.gid;
  }
}

}  // namespace

int tmog::prime_tree_partition() { return prime_kernel(&leaf_collect_kernel); }

// ------------------------------------------------------------------------------------- C ABI
extern "C" {

int tmog_hip_partition_fused(const uint8_t* Xb, int F, const uint32_t* rows_in, uint32_t* rows_out, const void* items,
                             int n_items, const int64_t* node_begin, const int64_t* node_count, const int32_t* split_feat,
                             const int32_t* split_bin, const uint8_t* dl, const float* node_params,
                             const float* split_gain, int missing_bin, int64_t* cursors, const uint8_t* XbT,
                             int64_t N, hipStream_t stream, const int32_t* gh_in, int32_t* gh_out, const int* dcount,
                             int wide_rows) {
  if (n_items == 0) return 0;
  if ((gh_in != nullptr) != (gh_out != nullptr)) return -2;
  hipLaunchKernelGGL(partition_fused_kernel, dim3(n_items), dim3(256), 0, stream, Xb, F, rows_in, rows_out,
                     (const PartItem*)items, node_begin, node_count, split_feat, split_bin, dl, node_params,
                     split_gain, missing_bin, (unsigned long long*)cursors, XbT, N,
                     reinterpret_cast<const int2*>(gh_in), reinterpret_cast<int2*>(gh_out), dcount, wide_rows);
  return (int)hipGetLastError();
}

int tmog_hip_leaf_collect(const uint32_t* rows, const void* items, int n_items, uint32_t* out_rows,
                          int32_t* out_gid, hipStream_t stream, const uint32_t* rows_alt, const int* dcount) {
  if (n_items == 0) return 0;
  hipLaunchKernelGGL(leaf_collect_kernel, dim3(n_items), dim3(256), 0, stream, rows, rows_alt, (const LeafItem*)items,
                     out_rows, out_gid, dcount);
  return (int)hipGetLastError();
}

}  // extern "C"
