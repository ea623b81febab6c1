// Staged evaluation of a boosted forest for CDNA4 (gfx950): the validation curve of a model in one pass.
//
// staged_eval_kernel -- one lane per row, 256-lane workgroups. A lane walks the trees in stage order, adds each
// leaf value into its fp64 margin(s) and, whenever a stage's last tree has been added, contributes the metric of the
// updated margins to that stage's output (common/boost_eval.hpp: the per-row terms shared with the host twin
// tmog_forest_staged_eval_cpu). A call covers S stages; models/tree_engine.py forest_staged_eval chunks longer models
// and carries the margins from call to call. Scoring every prefix with forest_predict would walk O(S^2) trees.
//
//   * Four independent tree walks are in flight per lane (as forest_predict_kernel), across stage boundaries: the
//     walks do not depend on the margins, only the adds and the metric are ordered.
//   * K == 1 (binary and regression metrics): the margin stays in a register for the whole call. K > 1: the lane's
//     margin row lives in the global margins buffer (read-modify-write by its own lane only); the K-class terms
//     stream over it, so K is not bounded by registers.
//   * Counted metrics: one wave ballot and one 64-bit integer atomic per wave and stage. aupr: integer atomics
//     into the stage's [2][bins] table after the wave-level aggregation of equal slots of boost_epilogue_kernel.
//     Floating sums: wave shuffle reduction, the four wave sums added in wave order into slab[block][stage], then
//     staged_reduce_kernel adds the slab rows of a stage in a fixed order. No floating-point atomics: the sums are
//     bitwise reproducible for the same inputs.
// Tree offsets, tree_col < K and row_list < N are validated once by the Python wrapper, not here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "hip/tmog_hip_abi.h"
#include "common/boost_eval.hpp"

namespace {

using namespace tmog;

constexpr int kBlock = TMOG_EVAL_BLOCK;
constexpr int kWaves = kBlock / 64;
constexpr int kWalks = 4;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;   // lane 0 holds the sum, added in a fixed tree order
}

template <int METRIC>
__global__ void __launch_bounds__(kBlock) staged_eval_kernel(
    const uint8_t* __restrict__ Xb, int F, const int32_t* __restrict__ row_list, int64_t n,
    const float* __restrict__ y, const int4* __restrict__ nodes, const uint8_t* __restrict__ default_left,
    const float* __restrict__ leaf_value, const int64_t* __restrict__ tree_off,
    const float* __restrict__ tree_weight, int missing_bin, const int64_t* __restrict__ stage_off, int S,
    const int32_t* __restrict__ tree_col, int K, double scale, int bins, double* __restrict__ margins,
    unsigned long long* __restrict__ counts, int32_t* __restrict__ tables, double* __restrict__ slab) {
  constexpr bool kMulti = METRIC == TMOG_EVAL_MLOGLOSS || METRIC == TMOG_EVAL_MERROR;
  constexpr bool kCounted = METRIC == TMOG_EVAL_ERROR || METRIC == TMOG_EVAL_MERROR;
  constexpr bool kTable = METRIC == TMOG_EVAL_AUPR;
  __shared__ double s_wave[2][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  // no early return: the ballots, shuffles and barriers below need every lane of the workgroup
  const bool ok = i < n;
  const int64_t row = ok ? (row_list ? (int64_t)row_list[i] : i) : 0;
  const uint8_t* xr = Xb + row * F;
  const float yr = ok ? y[row] : 0.f;
  double* mr = margins + i * K;              // dereferenced only when ok
  double m = (!kMulti && ok) ? mr[0] : 0.0;  // K == 1: the margin, in a register across the call

  int s = 0;
  // the metric of stage s over the workgroup's rows, from the margins as they stand
  auto emit = [&]() {
    if constexpr (kTable) {
      int slot = ok ? eval_aupr_slot(m, scale, yr, bins) : -1;
      int32_t* tb = tables + (int64_t)s * 2 * bins;
      // scores cluster in a few bins: the wave peels off up to 8 distinct slots (one atomic of the match count
      // each), the rest go per lane
      bool pend = slot >= 0;
      for (int it = 0; it < 8; ++it) {
        const unsigned long long act = __ballot(pend);
        if (act == 0ull) break;
        const int leader = __ffsll((long long)act) - 1;
        const int ls = __builtin_amdgcn_readlane(slot, leader);
        const bool mine = pend && slot == ls;
        const unsigned long long mm = __ballot(mine);
        if (lane == leader) atomicAdd(tb + ls, (int)__popcll(mm));
        pend = pend && !mine;
      }
      if (pend) atomicAdd(tb + slot, 1);
    } else if constexpr (kCounted) {
      int bad = 0;
      if (ok) {
        if constexpr (kMulti)
          bad = eval_merror([&](int c) { return mr[c]; }, K, (int)yr);
        else
          bad = eval_error(m, scale, (double)yr);
      }
      const unsigned long long mm = __ballot(bad != 0);
      if (lane == 0 && mm != 0ull) atomicAdd(counts + s, (unsigned long long)__popcll(mm));
    } else {
      double term = 0.0;
      if (ok) {
        if constexpr (METRIC == TMOG_EVAL_LOGLOSS) term = eval_logloss(m, scale, (double)yr);
        if constexpr (METRIC == TMOG_EVAL_SQERR) term = eval_sqerr(m, (double)yr);
        if constexpr (METRIC == TMOG_EVAL_ABSERR) term = eval_abserr(m, (double)yr);
        if constexpr (METRIC == TMOG_EVAL_MLOGLOSS)
          term = eval_mlogloss([&](int c) { return mr[c]; }, K, eval_label(yr, K));
      }
      const double ws = wave_sum(term);
      // double buffered by stage parity: thread 0 reads stage s while the waves may already write stage s + 1
      if (lane == 0) s_wave[s & 1][wave] = ws;
      __syncthreads();
      if (threadIdx.x == 0) {
        double b = s_wave[s & 1][0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) b += s_wave[s & 1][w];
        slab[(int64_t)blockIdx.x * S + s] = b;
      }
    }
  };

  int64_t t = stage_off[0];
  const int64_t t_end = stage_off[S];
  while (s < S && stage_off[s + 1] == t) {   // leading stages without trees
    emit();
    ++s;
  }
  while (t < t_end) {
    const int nb = (int)((t_end - t) < kWalks ? (t_end - t) : kWalks);
    int k[kWalks];
    int4 nd[kWalks];
#pragma unroll
    for (int u = 0; u < kWalks; ++u) {
      k[u] = 0;
      nd[u] = make_int4(0, 0, -1, -1);
      if (ok && u < nb) {
        k[u] = (int)tree_off[t + u];
        nd[u] = nodes[k[u]];
      }
    }
    bool active = ok;
    while (active) {
      active = false;
#pragma unroll
      for (int u = 0; u < kWalks; ++u) {
        if (nd[u].z >= 0) {
          const uint8_t b = xr[nd[u].x];
          const bool gl = goes_left(b, nd[u].y, [&] { return default_left[k[u]] != 0; }, missing_bin);
          k[u] = gl ? nd[u].z : nd[u].w;
          nd[u] = nodes[k[u]];
          active = true;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kWalks; ++u) {
      if (u < nb) {
        if (ok) {
          const double add = (double)tree_weight[t + u] * (double)leaf_value[k[u]];
          if constexpr (kMulti)
            mr[tree_col ? tree_col[t + u] : 0] += add;
          else
            m += add;
        }
        while (s < S && stage_off[s + 1] == t + u + 1) {
          emit();
          ++s;
        }
      }
    }
    t += nb;
  }
  if constexpr (!kMulti)
    if (ok) mr[0] = m;
}

// values[s] = the slab column of stage s added in a fixed order: lane j takes blocks j, j + 256, ... in order, then
// a shared-memory tree over the 256 lanes. One workgroup per stage.
__global__ void __launch_bounds__(kBlock) staged_reduce_kernel(const double* __restrict__ slab, int64_t nblk, int S,
                                                               double* __restrict__ values) {
  __shared__ double s_part[kBlock];
  const int s = blockIdx.x;
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < nblk; b += kBlock) acc += slab[b * S + s];
  s_part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_part[threadIdx.x] += s_part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) values[s] = s_part[0];
}

}  // namespace

extern "C" {

int tmog_hip_forest_staged_eval(const uint8_t* Xb, int F, const int32_t* row_list, int64_t n, const float* y,
                                const int32_t* nodes, const uint8_t* default_left, const float* leaf_value,
                                const int64_t* tree_off, const float* tree_weight, int missing_bin,
                                const int64_t* stage_off, int S, const int32_t* tree_col, int K, int metric,
                                double scale, int bins, double* margins, double* values, int64_t* counts,
                                int32_t* tables, double* slab, hipStream_t stream) {
  if (!eval_metric_known(metric) || K < 1 || (!eval_metric_multi(metric) && K != 1)) return 1;
  if (n <= 0 || S <= 0) return 0;
  const int64_t nblk = (n + kBlock - 1) / kBlock;
  if (nblk > 0x7fffffff) return 2;
#define TM_STAGED(M)                                                                                               \
  case M:                                                                                                          \
    hipLaunchKernelGGL(staged_eval_kernel<M>, dim3((unsigned)nblk), dim3(kBlock), 0, stream, Xb, F, row_list, n, y, \
                       (const int4*)nodes, default_left, leaf_value, tree_off, tree_weight, missing_bin, stage_off, \
                       S, tree_col, K, scale, bins, margins, (unsigned long long*)counts, tables, slab);            \
    break;
  switch (metric) {
    TM_STAGED(TMOG_EVAL_LOGLOSS)
    TM_STAGED(TMOG_EVAL_ERROR)
    TM_STAGED(TMOG_EVAL_AUPR)
    TM_STAGED(TMOG_EVAL_SQERR)
    TM_STAGED(TMOG_EVAL_ABSERR)
    TM_STAGED(TMOG_EVAL_MLOGLOSS)
    TM_STAGED(TMOG_EVAL_MERROR)
  }
#undef TM_STAGED
  if (!eval_metric_counted(metric) && metric != TMOG_EVAL_AUPR)
    hipLaunchKernelGGL(staged_reduce_kernel, dim3(S), dim3(kBlock), 0, stream, slab, nblk, S, values);
  return (int)hipGetLastError();
}

}  // extern "C"
