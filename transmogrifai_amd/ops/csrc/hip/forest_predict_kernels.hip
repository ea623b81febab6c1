// Forest scoring kernels for CDNA4 (gfx950): ensemble traversal over binned rows (SURVEY.md kernel K29) for the
// forests that the tree engine grows (tree_hist_kernels.hip and its siblings) -- Xb is uint8 [N][F] row-major bins.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <stdint.h>

#include "common/tree_rules.hpp"
#include "hip/tmog_hip_abi.h"
#include "hip/tree_dev.hpp"

namespace {

using namespace tmog;   // common/tree_rules.hpp: goes_left, the rule shared with the CPU twin

// Three kernel shapes score a forest, each written once over a node source (below): forest_predict_lds_kernel
// (rows staged in LDS, F <= 512), forest_predict_kernel (rows in global memory) and forest_predict_multi_kernel
// (a shared forest's pruned variants).
constexpr int PRED_ROWS = 128;
constexpr int PRED_TU = 8;
constexpr int PRED_TPR = 4;   // threads per row (tree slices), 512-thread workgroups sharing the staged rows

constexpr int PM_ROWS = 64;
constexpr int PM_TPR = 4;
constexpr int PM_TU = 4;
constexpr int PM_VK = TMOG_PM_VK;      // variants x classes accumulated per thread

// A node source is how a walk reads the forest: load(k) gives node k's record, is_leaf(record) whether every walk
// ends there, mask(record, k) the variants that stop there at any depth, and child(record, k, xr, missing_bin) the
// next node for the row whose bins are xr[] (the rule is goes_left's). Node indices are int: children are int32 in
// `nodes`, so no forest has more. The kernels do the same fp32 operations in the same order over either source, so
// the two give the same bits.
//
// ImageNodes reads a packed node image, one 16-byte record per node,
//   x = feat | bin << 16 | default_left << 24,  y = variant stop mask (0 for the plain kernels),  z / w = children,
// so a walk step is one dependent 16-byte load. forest_image_kernel builds the image once per forest (the caller
// keeps it for every later batch).
struct ImageNodes {
  using Rec = uint4;
  const uint4* __restrict__ img;
  __device__ __forceinline__ Rec load(int k) const { return img[k]; }
  __device__ __forceinline__ static bool is_leaf(const Rec& nd) { return (int)nd.z < 0; }
  __device__ __forceinline__ uint32_t mask(const Rec& nd, int) const { return nd.y; }
  __device__ __forceinline__ int child(const Rec& nd, int, const uint8_t* xr, int missing_bin) const {
    const uint8_t b = xr[nd.x & 0xFFFFu];
    const bool gl = goes_left(b, (int)((nd.x >> 16) & 0xFFu), [&] { return (nd.x >> 24) != 0u; }, missing_bin);
    return (int)(gl ? nd.z : nd.w);
  }
};

// DirectNodes reads `nodes` / `default_left` / `node_mask` as the growers leave them: feature and split bin keep
// their 32 bits, which is why it exists (a forest with feat >= 65536 or bin >= 256 does not fit the record). A step
// is a node load, in the variant kernel a mask load and, on a missing bin, a default_left load. TMOG_PREDICT_V1=1
// selects it for every forest (tmog_hip_predict_v1).
struct DirectNodes {
  using Rec = int4;
  const int4* __restrict__ nodes;
  const uint8_t* __restrict__ default_left;
  const uint32_t* __restrict__ node_mask;                   // null for the plain kernels, which never ask
  __device__ __forceinline__ Rec load(int k) const { return nodes[k]; }
  __device__ __forceinline__ static bool is_leaf(const Rec& nd) { return nd.z < 0; }
  __device__ __forceinline__ uint32_t mask(const Rec&, int k) const { return node_mask[k]; }
  __device__ __forceinline__ int child(const Rec& nd, int k, const uint8_t* xr, int missing_bin) const {
    const uint8_t b = xr[nd.x];
    const bool gl = goes_left(b, nd.y, [&] { return default_left[k] != 0; }, missing_bin);
    return gl ? nd.z : nd.w;
  }
};

__global__ void __launch_bounds__(256) forest_image_kernel(const int4* __restrict__ nodes,
                                                           const uint8_t* __restrict__ default_left,
                                                           const uint32_t* __restrict__ node_mask, int64_t n,
                                                           uint4* __restrict__ img) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int4 nd = nodes[i];
  img[i] = make_uint4((uint32_t)nd.x | (uint32_t)nd.y << 16 | (default_left[i] != 0 ? 1u << 24 : 0u),
                      node_mask ? node_mask[i] : 0u, (uint32_t)nd.z, (uint32_t)nd.w);
}

// Copies the workgroup's nrow rows (row r at srows + r * F) with the widest loads the row pitch and the base allow:
// 16 bytes, else 4, else the byte loop.
__device__ __forceinline__ void stage_rows(uint8_t* srows, const uint8_t* __restrict__ Xb, int F,
                                           const int32_t* __restrict__ row_list, int64_t blk0, int64_t r0, int nrow) {
  const uintptr_t base = reinterpret_cast<uintptr_t>(Xb);
  if (F % 16 == 0 && base % 16 == 0) {
    const int per = F >> 4;
    for (int i = threadIdx.x; i < nrow * per; i += blockDim.x) {
      const int r = i / per, b = i - r * per;
      const int64_t row = row_list ? row_list[blk0 + r] : (blk0 + r - r0);
      reinterpret_cast<uint4*>(srows)[i] = reinterpret_cast<const uint4*>(Xb + row * F)[b];
    }
  } else if (F % 4 == 0 && base % 4 == 0) {
    const int per = F >> 2;
    for (int i = threadIdx.x; i < nrow * per; i += blockDim.x) {
      const int r = i / per, b = i - r * per;
      const int64_t row = row_list ? row_list[blk0 + r] : (blk0 + r - r0);
      reinterpret_cast<uint32_t*>(srows)[i] = reinterpret_cast<const uint32_t*>(Xb + row * F)[b];
    }
  } else {
    // any other pitch (F = 329, the headline's): a wave per row, a byte per lane. Eight batched byte loads per lane
    // and 4-byte loads at any alignment were both measured and neither was faster (profiles/README.md, round 8).
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    for (int r = wave; r < nrow; r += nwaves) {
      const int64_t row = row_list ? row_list[blk0 + r] : (blk0 + r - r0);
      const uint8_t* src = Xb + row * F;
      for (int b = lane; b < F; b += 64) srows[r * F + b] = src[b];
    }
  }
}

// LDS-row kernel (F <= 512): the workgroup first stages its 128 rows' bins (row-major, F bytes each) in LDS, then
// four lanes per row each walk a quarter of the model's trees (chunks of eight interleaved) reading bins from LDS,
// and the four partial sums are folded in a fixed order. 512-thread workgroups keep 16 waves per CU busy on the
// dependent node-fetch chains (128-thread groups left 4 waves per CU with the 64 KB of staged rows). Without the
// staging each tree step paid a dependent L2/Infinity-cache round trip for a single byte (64 lanes = 64 different
// rows = 64 cache lines per step); now only the node fetch (shared by the wave near the root, L2/L1 resident)
// stays global. grid.y = model. The q-fold reuses the staged rows' LDS once the walks are done, so a
// workgroup holds max(PRED_ROWS * F, 16 KB): three workgroups (24 waves) per CU at F = 352, two at F = 512.
// Six waves per SIMD (80 VGPRs) are asked for so that the registers allow those three workgroups too; neither node
// source spills under it.
template <class NS>
__global__ void __launch_bounds__(PRED_ROWS * PRED_TPR) __attribute__((amdgpu_waves_per_eu(6)))
forest_predict_lds_kernel(
    const uint8_t* __restrict__ Xb, int F, const int64_t* __restrict__ model_row_off,
    const int32_t* __restrict__ row_list, const int64_t* __restrict__ model_tree_off,
    const int64_t* __restrict__ tree_off, const float* __restrict__ tree_weight, const NS ns,
    int missing_bin, const float* __restrict__ leaf_value, int K, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t srows[];
  const int m = blockIdx.y;
  const int64_t r0 = model_row_off[m], r1 = model_row_off[m + 1];
  const int64_t blk0 = r0 + (int64_t)blockIdx.x * PRED_ROWS;
  if (blk0 >= r1) return;                                   // whole workgroup out of range (uniform)
  const int nrow = (int)min((int64_t)PRED_ROWS, r1 - blk0);
  stage_rows(srows, Xb, F, row_list, blk0, r0, nrow);
  __syncthreads();
  const int rr = threadIdx.x % PRED_ROWS, q = threadIdx.x / PRED_ROWS;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (rr < nrow) {
    const uint8_t* xr = srows + rr * F;
    const int64_t t_end = model_tree_off[m + 1];
    for (int64_t t = model_tree_off[m] + (int64_t)q * PRED_TU; t < t_end; t += (int64_t)PRED_TU * PRED_TPR) {
      const int nu = (int)min((int64_t)PRED_TU, t_end - t);
      int k[PRED_TU];
      typename NS::Rec nd[PRED_TU];
#pragma unroll
      for (int u = 0; u < PRED_TU; ++u) {
        k[u] = (int)(u < nu ? tree_off[t + u] : tree_off[t]);   // an idle slot re-walks the first tree; not added
        nd[u] = ns.load(k[u]);
      }
      bool active = true;
      while (active) {
        active = false;
#pragma unroll
        for (int u = 0; u < PRED_TU; ++u) {
          if (!NS::is_leaf(nd[u])) {
            k[u] = ns.child(nd[u], k[u], xr, missing_bin);
            nd[u] = ns.load(k[u]);
            active = true;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < PRED_TU; ++u) {
        if (u < nu) {
#pragma clang fp contract(off)
          const float w = tree_weight[t + u];
          for (int c = 0; c < K && c < 8; ++c) acc[c] += w * leaf_value[(int64_t)k[u] * K + c];
        }
      }
    }
  }
  __syncthreads();                                          // the rows are read no more: the fold takes their LDS
  float* red = reinterpret_cast<float*>(srows);
  for (int c = 0; c < 8; ++c) red[(q * PRED_ROWS + rr) * 8 + c] = acc[c];
  __syncthreads();
  if (q == 0 && rr < nrow) {
    float* o = out + (blk0 + rr) * K;
    for (int c = 0; c < K && c < 8; ++c) {
      float v = red[rr * 8 + c];
      for (int qq = 1; qq < PRED_TPR; ++qq) v += red[(qq * PRED_ROWS + rr) * 8 + c];
      o[c] = v;
    }
  }
}

// Shared-forest prediction for pruned variants (models/trees.py: RF grid points that differ only in
// maxDepth / minInfoGain share one grown forest, tree_engine.prune_forest). Model m walks the grown
// trees once per (row, tree) and serves all of its variants v in [var_off[m], var_off[m+1]) on the way
// down: variant v stops at the first node that is a leaf of the grown tree, lies at depth >= var_depth[v]
// or has a split gain < the variant's min gain (exactly prune_forest's rule; the leaf / gain part comes
// precomputed as a per-node variant bitmask) and adds that node's value. One walk
// instead of one per variant (~5x fewer node visits for the default RF grid). Rows staged in LDS as in
// forest_predict_lds_kernel; 4 trees interleaved per thread; out[var_out_off[v] + (row - r0) * K + c].
// KT = classes; the thread's VKP >= V * KT sums stay in registers. A depth
// iteration first gathers the four walks' stop sets (the node's mask word | depth table), then, if any lane of
// the wave stops anywhere, loads the four nodes' values together and adds them in u order by selecting the sum
// (acc = bit ? acc + val : acc; an add of 0.0f would turn a -0.0f sum into +0.0f), then steps the four walks
// without a branch: four LDS reads, then four node loads in flight. LDS holds max(rows, the fold's three partial
// planes): 46.7 KB at F = 730 (three workgroups per CU), 24 KB at F = 352 and VKP = 32.
template <class NS, int KT, int VKP>
__global__ void __launch_bounds__(PM_ROWS * PM_TPR) forest_predict_multi_kernel(
    const uint8_t* __restrict__ Xb, int F, const int64_t* __restrict__ model_row_off,
    const int32_t* __restrict__ row_list, const int64_t* __restrict__ model_tree_off,
    const int64_t* __restrict__ tree_off, const float* __restrict__ tree_weight, const NS ns,
    int missing_bin, const float* __restrict__ leaf_value, const int32_t* __restrict__ var_off,
    const int32_t* __restrict__ var_depth, const int64_t* __restrict__ var_out_off, float* __restrict__ out) {
  constexpr int NV = VKP / KT;                              // variants the registers hold; host: V <= NV
  extern __shared__ __attribute__((aligned(16))) uint8_t srows[];
  const int m = blockIdx.y;
  const int64_t r0 = model_row_off[m], r1 = model_row_off[m + 1];
  const int64_t blk0 = r0 + (int64_t)blockIdx.x * PM_ROWS;
  if (blk0 >= r1) return;
  const int nrow = (int)min((int64_t)PM_ROWS, r1 - blk0);
  const int v0 = var_off[m], V = var_off[m + 1] - v0;
  stage_rows(srows, Xb, F, row_list, blk0, r0, nrow);
  // depth stop masks: s_dmask[d] = variants whose max depth is <= d (the gain / grown-leaf part of the rule is the
  // node's mask word, precomputed by the host: the variants that stop at the node regardless of depth). The table
  // ends at depth 32: a variant with var_depth > 32 is in no s_dmask entry, so for such a variant the host also
  // sets its mask bit at every node of depth >= var_depth (tree_engine.forest_predict_multi).
  __shared__ uint32_t s_dmask[33];
  if (threadIdx.x < 33) {
    uint32_t mk = 0u;
    for (int v = 0; v < V; ++v) mk |= (var_depth[v0 + v] <= (int)threadIdx.x ? 1u : 0u) << v;
    s_dmask[threadIdx.x] = mk;
  }
  __syncthreads();
  const int rr = threadIdx.x % PM_ROWS, q = threadIdx.x / PM_ROWS;
  float acc[VKP];
#pragma unroll
  for (int i = 0; i < VKP; ++i) acc[i] = 0.f;
  if (rr < nrow) {
    const uint8_t* xr = srows + rr * F;
    const int64_t t_end = model_tree_off[m + 1];
    const uint32_t all = V >= 32 ? 0xFFFFFFFFu : (1u << V) - 1u;
    for (int64_t t = model_tree_off[m] + (int64_t)q * PM_TU; t < t_end; t += (int64_t)PM_TU * PM_TPR) {
      const int nu = (int)min((int64_t)PM_TU, t_end - t);
      int k[PM_TU];
      typename NS::Rec nd[PM_TU];
      uint32_t live[PM_TU];
      float w[PM_TU];
#pragma unroll
      for (int u = 0; u < PM_TU; ++u) {
        k[u] = (int)(u < nu ? tree_off[t + u] : tree_off[t]);
        nd[u] = ns.load(k[u]);
        live[u] = u < nu ? all : 0u;
        w[u] = tree_weight[u < nu ? t + u : t];
      }
      int dep = 0;                                          // the chunk's walks step together: one depth for all
      while ((live[0] | live[1] | live[2] | live[3]) != 0u) {
        static_assert(PM_TU == 4, "the loop condition above names four walks");
        const uint32_t dm = s_dmask[min(dep, 32)];
        uint32_t stop[PM_TU], any = 0u;
#pragma unroll
        for (int u = 0; u < PM_TU; ++u) {
          stop[u] = (ns.mask(nd[u], k[u]) | dm) & live[u];
          any |= stop[u];
        }
        if (any != 0u) {
          float lv[PM_TU][KT];
#pragma unroll
          for (int u = 0; u < PM_TU; ++u)
#pragma unroll
            for (int c = 0; c < KT; ++c) lv[u][c] = leaf_value[(int64_t)k[u] * KT + c];
#pragma unroll
          for (int u = 0; u < PM_TU; ++u) {
            if (stop[u] != 0u) {
#pragma clang fp contract(off)
#pragma unroll
              for (int c = 0; c < KT; ++c) {
                const float val = w[u] * lv[u][c];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                  const float sum = acc[v * KT + c] + val;
                  acc[v * KT + c] = ((stop[u] >> v) & 1u) ? sum : acc[v * KT + c];
                }
              }
              live[u] &= ~stop[u];
            }
          }
        }
        // a finished walk steps too, for nothing: its record's feature is a column of the row (0 at a leaf)
        int kn[PM_TU];
#pragma unroll
        for (int u = 0; u < PM_TU; ++u) kn[u] = ns.child(nd[u], k[u], xr, missing_bin);
#pragma unroll
        for (int u = 0; u < PM_TU; ++u) {
          k[u] = live[u] != 0u ? kn[u] : k[u];              // a finished walk re-reads its own node
          nd[u] = ns.load(k[u]);
        }
        dep += 1;
      }
    }
  }
  __syncthreads();                                          // the rows are read no more: the fold takes their LDS
  float* red = reinterpret_cast<float*>(srows);             // [q - 1][i][rr]: lanes of a wave on distinct banks
  if (q > 0) {
#pragma unroll
    for (int i = 0; i < VKP; ++i) red[((q - 1) * VKP + i) * PM_ROWS + rr] = acc[i];
  }
  __syncthreads();
  if (q == 0 && rr < nrow) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (v < V) {
        float* o = out + var_out_off[v0 + v] + (blk0 + rr - r0) * KT;
#pragma unroll
        for (int c = 0; c < KT; ++c) {
          float x = acc[v * KT + c];
          for (int qq = 1; qq < PM_TPR; ++qq) x += red[((qq - 1) * VKP + v * KT + c) * PM_ROWS + rr];
          o[c] = x;
        }
      }
    }
  }
}

// F > 512: rows stay in global memory. grid.y = model; each thread walks every tree of its model for one of the
// model's rows, four trees together (four independent node-fetch -> bin-fetch chains in flight per lane).
template <class NS>
__global__ void __launch_bounds__(256) forest_predict_kernel(
    const uint8_t* __restrict__ Xb, int F, const int64_t* __restrict__ model_row_off,
    const int32_t* __restrict__ row_list, const int64_t* __restrict__ model_tree_off,
    const int64_t* __restrict__ tree_off, const float* __restrict__ tree_weight, const NS ns,
    int missing_bin, const float* __restrict__ leaf_value, int K, float* __restrict__ out) {
  const int m = blockIdx.y;
  const int64_t r0 = model_row_off[m], r1 = model_row_off[m + 1];
  const int64_t i = r0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r1) return;
  const int64_t row = row_list ? row_list[i] : (i - r0);
  const uint8_t* xr = Xb + row * F;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t t_end = model_tree_off[m + 1];
  int64_t t = model_tree_off[m];
  for (; t + 4 <= t_end; t += 4) {
    int k[4];
    typename NS::Rec nd[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      k[u] = (int)tree_off[t + u];
      nd[u] = ns.load(k[u]);
    }
    bool active = true;
    while (active) {
      active = false;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!NS::is_leaf(nd[u])) {
          k[u] = ns.child(nd[u], k[u], xr, missing_bin);
          nd[u] = ns.load(k[u]);
          active = true;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma clang fp contract(off)
      const float w = tree_weight[t + u];
      for (int c = 0; c < K && c < 8; ++c) acc[c] += w * leaf_value[(int64_t)k[u] * K + c];
    }
  }
  for (; t < t_end; ++t) {
#pragma clang fp contract(off)
    int k = (int)tree_off[t];
    typename NS::Rec nd = ns.load(k);
    while (!NS::is_leaf(nd)) {
      k = ns.child(nd, k, xr, missing_bin);
      nd = ns.load(k);
    }
    const float w = tree_weight[t];
    for (int c = 0; c < K && c < 8; ++c) acc[c] += w * leaf_value[(int64_t)k * K + c];
  }
  float* o = out + i * K;
  for (int c = 0; c < K && c < 8; ++c) o[c] = acc[c];
}

// Plain scoring over node source `ns`: the LDS kernel while 128 rows fit 64 KiB (F <= 512), else the global-row one.
template <class NS>
int launch_forest_predict(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                          const int32_t* row_list, int64_t max_rows, const int64_t* model_tree_off,
                          const int64_t* tree_off, const float* tree_weight, NS ns, int missing_bin,
                          const float* leaf_value, int K, float* out, hipStream_t stream) {
  if (n_models == 0 || max_rows == 0) return 0;
  if (K > 8) return -2;
  if ((size_t)PRED_ROWS * F <= 64 * 1024) {
    dim3 g2((unsigned)((max_rows + PRED_ROWS - 1) / PRED_ROWS), n_models);
    const size_t rows_b = ((size_t)PRED_ROWS * F + 15) & ~(size_t)15;
    const size_t fold_b = sizeof(float) * 8 * PRED_ROWS * PRED_TPR;
    hipLaunchKernelGGL(forest_predict_lds_kernel<NS>, g2, dim3(PRED_ROWS * PRED_TPR),
                       rows_b > fold_b ? rows_b : fold_b, stream, Xb, F, model_row_off, row_list, model_tree_off,
                       tree_off, tree_weight, ns, missing_bin, leaf_value, K, out);
    return (int)hipGetLastError();
  }
  dim3 grid((unsigned)((max_rows + 255) / 256), n_models);
  hipLaunchKernelGGL(forest_predict_kernel<NS>, grid, dim3(256), 0, stream, Xb, F, model_row_off, row_list,
                     model_tree_off, tree_off, tree_weight, ns, missing_bin, leaf_value, K, out);
  return (int)hipGetLastError();
}

// Dynamic LDS of a variant-scoring workgroup with vkp register sums per thread: the staged rows, which the fold's
// PM_TPR - 1 partial planes reuse (vkp = 0: the rows alone).
inline size_t pm_lds_bytes(int F, int vkp) {
  const size_t rows_b = ((size_t)PM_ROWS * F + 15) & ~(size_t)15;
  const size_t fold_b = sizeof(float) * (PM_TPR - 1) * vkp * PM_ROWS;
  return rows_b > fold_b ? rows_b : fold_b;
}

// Variant scoring over node source `ns` with VKP register sums per thread; the caller has checked K in {1, 2, 4, 8}
// and V * K <= VKP for every model.
template <class NS, int VKP>
int launch_forest_predict_multi(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                                const int32_t* row_list, int64_t max_rows, const int64_t* model_tree_off,
                                const int64_t* tree_off, const float* tree_weight, NS ns, int missing_bin,
                                const float* leaf_value, int K, const int32_t* var_off, const int32_t* var_depth,
                                const int64_t* var_out_off, float* out, hipStream_t stream) {
  const size_t lds = pm_lds_bytes(F, VKP);
  if (lds + sizeof(uint32_t) * 33 > 160 * 1024) return -3;   // dynamic LDS + the kernel's static s_dmask[33]
  dim3 g2((unsigned)((max_rows + PM_ROWS - 1) / PM_ROWS), n_models);
#define TM_PM(KV)                                                                                               \
  hipLaunchKernelGGL((forest_predict_multi_kernel<NS, KV, VKP>), g2, dim3(PM_ROWS * PM_TPR), lds, stream, Xb, F, \
                     model_row_off, row_list, model_tree_off, tree_off, tree_weight, ns, missing_bin, leaf_value, \
                     var_off, var_depth, var_out_off, out)
  if (K == 1) TM_PM(1);
  else if (K == 2) TM_PM(2);
  else if (K == 4) TM_PM(4);
  else TM_PM(8);
#undef TM_PM
  return (int)hipGetLastError();
}

}  // namespace

int tmog::prime_forest_predict() { return prime_kernel(&forest_image_kernel); }

// ------------------------------------------------------------------------------------- C ABI
extern "C" {

// Shared-forest multi-variant prediction over the direct node source. Every model's V x K <= 32 (V <= 32): the
// signature carries no variant count, so this entry always takes the 32-sum tile.
int tmog_hip_forest_predict_multi(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                                  const int32_t* row_list, int64_t max_rows, const int64_t* model_tree_off,
                                  const int64_t* tree_off, const float* tree_weight, const int32_t* nodes,
                                  const uint8_t* default_left, int missing_bin, const float* leaf_value, int K,
                                  const uint32_t* node_mask, const int32_t* var_off, const int32_t* var_depth,
                                  const int64_t* var_out_off, float* out, hipStream_t stream) {
  if (n_models == 0 || max_rows == 0) return 0;
  if (K != 1 && K != 2 && K != 4 && K != 8) return -2;
  // This refusal (F >= 2046) is the entry's contract with its callers, not the kernel's need, which is max(rows, fold)
  // below: tree_engine._pm_lds_bytes mirrors it, and the wrapper's by-value fallback for wide tables hangs on that.
  const size_t lds = pm_lds_bytes(F, 0) + sizeof(float) * PM_VK * PM_ROWS * PM_TPR;
  if (lds + sizeof(uint32_t) * 33 > 160 * 1024) return -3;
  return launch_forest_predict_multi<DirectNodes, PM_VK>(
      Xb, F, n_models, model_row_off, row_list, max_rows, model_tree_off, tree_off, tree_weight,
      DirectNodes{(const int4*)nodes, default_left, node_mask}, missing_bin, leaf_value, K, var_off, var_depth,
      var_out_off, out, stream);
}

int tmog_hip_forest_predict(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                            const int32_t* row_list, int64_t max_rows, const int64_t* model_tree_off,
                            const int64_t* tree_off, const float* tree_weight, const int32_t* nodes,
                            const uint8_t* default_left, int missing_bin, const float* leaf_value, int K, float* out,
                            hipStream_t stream) {
  return launch_forest_predict(Xb, F, n_models, model_row_off, row_list, max_rows, model_tree_off, tree_off,
                               tree_weight, DirectNodes{(const int4*)nodes, default_left, nullptr}, missing_bin,
                               leaf_value, K, out, stream);
}

// TMOG_PREDICT_V1=1 selects the direct node source for every forest (the A/B switch against the image). Read once
// per process.
int tmog_hip_predict_v1() {
  static const int v1 = [] { const char* e = std::getenv("TMOG_PREDICT_V1"); return e && e[0] == '1'; }() ? 1 : 0;
  return v1;
}

// image[4 * i ..] = the packed record of node i (forest_image_kernel); node_mask may be null (plain scoring).
// The caller has checked feat < 65536 and 0 <= bin < 256.
int tmog_hip_forest_image(const int32_t* nodes, const uint8_t* default_left, const uint32_t* node_mask, int64_t n,
                          int32_t* image, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(forest_image_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     (const int4*)nodes, default_left, node_mask, n, (uint4*)image);
  return (int)hipGetLastError();
}

// tmog_hip_forest_predict_multi over the image (whose mask words are the call's node_mask). max_variants = the
// largest variant count of a model: it picks the register tile, 8, 16 or 32 sums per thread.
int tmog_hip_forest_predict_multi_image(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                                        const int32_t* row_list, int64_t max_rows, const int64_t* model_tree_off,
                                        const int64_t* tree_off, const float* tree_weight, const int32_t* image,
                                        int missing_bin, const float* leaf_value, int K, const int32_t* var_off,
                                        const int32_t* var_depth, const int64_t* var_out_off, int max_variants,
                                        float* out, hipStream_t stream) {
  if (n_models == 0 || max_rows == 0) return 0;
  if (K != 1 && K != 2 && K != 4 && K != 8) return -2;
  if (max_variants < 0 || max_variants > 32 || max_variants * K > PM_VK) return -2;
  const int vk = max_variants * K;
  auto* launch = vk <= 8 ? launch_forest_predict_multi<ImageNodes, 8>
                 : vk <= 16 ? launch_forest_predict_multi<ImageNodes, 16> : launch_forest_predict_multi<ImageNodes, 32>;
  return launch(Xb, F, n_models, model_row_off, row_list, max_rows, model_tree_off, tree_off, tree_weight,
                ImageNodes{(const uint4*)image}, missing_bin, leaf_value, K, var_off, var_depth, var_out_off, out,
                stream);
}

// tmog_hip_forest_predict over the image.
int tmog_hip_forest_predict_image(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                                  const int32_t* row_list, int64_t max_rows, const int64_t* model_tree_off,
                                  const int64_t* tree_off, const float* tree_weight, const int32_t* image,
                                  int missing_bin, const float* leaf_value, int K, float* out, hipStream_t stream) {
  return launch_forest_predict(Xb, F, n_models, model_row_off, row_list, max_rows, model_tree_off, tree_off,
                               tree_weight, ImageNodes{(const uint4*)image}, missing_bin, leaf_value, K, out, stream);
}

}  // extern "C"
