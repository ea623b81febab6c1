// Round epilogue of multiclass (multi:softprob / multi:softmax) XGBoost boosting for CDNA4 (gfx950).
//
// A K-class model is K Newton trees per round, one per class: pseudo-job q = p * K + k of the tree grower
// (models/trees.py). What couples the K trees is the softmax over a row's K margins, which gives the next
// round's (g, h) of all of them. Two launches per round replace the torch ops of that step:
//
// boost_margin_add_kernel -- for every training entry of the round's trees (the leaf assignment the grower
// returns): F[q, r] += value[gid] in fp64, q = tree_job[gid_tree[gid]]. Every (pseudo-job, row) pair occurs
// once among a round's entries, so the stores need no atomics.
//
// softmax_grad_kernel -- one thread per (model p, index i into the model's training-row list): reads the K
// margins F[(p K + k) N + r] (class stride N; consecutive lanes read consecutive entries of the row list, so a
// sorted list gives coalesced loads), p = softmax in fp64 and writes, for every class,
//     g_k = p_k - [y == k],   h_k = max(2 p_k (1 - p_k), 1e-16)                              (fp32)
// K is a runtime argument and no per-class register array is kept: the first pass over k carries the running
// maximum (with its first index: the argmax, ties to the lowest class) and the sum of exponentials rescaled
// whenever the maximum moves; the second pass re-reads F (L2 hits) and writes (g, h). It also produces
//   * the per-pseudo-job maxima of |g| and h (tree_engine._quant_scales of the next round) in the
//     [kAmaxCopies][P K][2] float-bits table of boost_kernels.hip: wave-level max on DPP, one atomicMax per
//     wave, class and statistic (a wave belongs to one model: blockIdx.y), and
//   * with a counter table, the per-model count of training rows whose argmax differs from the label
//     (eval_metric merror): one ballot and one integer atomicAdd per wave -- exact, order independent.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "hip/tmog_hip_abi.h"
#include "hip/tree_dev.hpp"

namespace {

constexpr int kAmaxCopies = 64;   // as boost_kernels.hip: the maxima table is [kAmaxCopies][P * K][2]

// Wave64 max of non-negative floats (their bit patterns order like int32) on DPP -- row_shr 1/2/4/8 inside the
// 16-lane rows, row_bcast 15/31 across them -- wave-uniform result. Whole wave active (boost_kernels.hip).
__device__ __forceinline__ float wave_max_nonneg(float f) {
  int v = __float_as_int(f);
#define TM_DPP_MAX(CTRL, ROWS) v = max(v, __builtin_amdgcn_update_dpp(0, v, CTRL, ROWS, 0xF, false));
  TM_DPP_MAX(0x111, 0xF) TM_DPP_MAX(0x112, 0xF) TM_DPP_MAX(0x114, 0xF) TM_DPP_MAX(0x118, 0xF)
  TM_DPP_MAX(0x142, 0xA) TM_DPP_MAX(0x143, 0xC)
#undef TM_DPP_MAX
  return __int_as_float(__builtin_amdgcn_readlane(v, 63));
}

__global__ void __launch_bounds__(256) boost_margin_add_kernel(
    const uint32_t* __restrict__ entries, const int32_t* __restrict__ gid, int64_t n_entries,
    const float* __restrict__ gid_value, const int64_t* __restrict__ gid_tree, const int64_t* __restrict__ tree_job,
    int64_t N, double* __restrict__ F, int64_t n_gid, int64_t n_trees, int64_t Q, int wide) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_entries) return;
  const int64_t r = (int64_t)tmog::ent_row(entries[e], wide);
  const int32_t g_id = gid[e];
  if (g_id < 0 || g_id >= n_gid || r >= N) return;   // defensive: never index out of range
  const int64_t t = gid_tree[g_id];
  if (t < 0 || t >= n_trees) return;
  const int64_t q = tree_job[t];
  if (q < 0 || q >= Q) return;
  F[q * N + r] += (double)gid_value[g_id];
}

__global__ void __launch_bounds__(256) softmax_grad_kernel(
    const int64_t* __restrict__ rows, const int64_t* __restrict__ row_off, const int64_t* __restrict__ models,
    int K, int64_t N, int64_t P, const double* __restrict__ F, const float* __restrict__ y,
    float* __restrict__ G, float* __restrict__ H, uint32_t* __restrict__ amax, int32_t* __restrict__ err) {
  const int64_t p = models[blockIdx.y];
  if (p < 0 || p >= P) return;                                   // block-uniform
  const int64_t lo = row_off[blockIdx.y], n = row_off[blockIdx.y + 1] - lo;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i - (threadIdx.x & 63) >= n) return;                       // wave-uniform: a wave past the list's end
  // no early returns from here on: the wave reductions below need every lane of the wave
  bool ok = i < n;
  int64_t r = 0;
  if (ok) {
    r = rows[lo + i];
    ok = r >= 0 && r < N;                                        // defensive: never index out of range
  }
  const int64_t base = p * K * N + r;
  int label = -1, arg = 0;
  double mx = 0.0, sum = 1.0;
  if (ok) {
    label = (int)y[r];
    mx = F[base];
    for (int k = 1; k < K; ++k) {
      const double f = F[base + (int64_t)k * N];
      if (f > mx) {                                              // strict: ties keep the lowest class
        sum = sum * exp(mx - f) + 1.0;
        mx = f;
        arg = k;
      } else {
        sum += exp(f - mx);
      }
    }
  }
  const int lane = threadIdx.x & 63;
  const int64_t copy = (int64_t)((blockIdx.x + blockIdx.y) % kAmaxCopies) * P * K + p * K;
  for (int k = 0; k < K; ++k) {
    float ag = 0.f, ah = 0.f;
    if (ok) {
      const int64_t a = base + (int64_t)k * N;
      const double pr = exp(F[a] - mx) / sum;
      const float gk = (float)(pr - (k == label ? 1.0 : 0.0));
      const float hk = (float)fmax(2.0 * pr * (1.0 - pr), 1e-16);
      G[a] = gk;
      H[a] = hk;
      ag = gk == gk ? fabsf(gk) : 0.f;                           // NaN lanes contribute nothing
      ah = hk == hk ? hk : 0.f;
    }
    if (amax) {
      const float mg = wave_max_nonneg(ag), mh = wave_max_nonneg(ah);
      if (lane == 0) {
        uint32_t* dst = amax + (copy + k) * 2;
        atomicMax(dst, __float_as_uint(mg));
        atomicMax(dst + 1, __float_as_uint(mh));
      }
    }
  }
  if (err) {
    const unsigned long long wrong = __ballot(ok && arg != label);
    if (lane == 0 && wrong) atomicAdd(err + p, (int)__popcll(wrong));
  }
}

}  // namespace

extern "C" {

// Q = number of pseudo-jobs (rows of F).
int tmog_hip_boost_margin_add(const uint32_t* entries, const int32_t* gid, int64_t n_entries, const float* gid_value,
                              const int64_t* gid_tree, const int64_t* tree_job, int64_t N, double* F, int64_t n_gid,
                              int64_t n_trees, int64_t Q, int wide_rows, hipStream_t stream) {
  if (n_entries == 0) return 0;
  if (N >= (1 << 24) && !wide_rows) return -2;
  hipLaunchKernelGGL(boost_margin_add_kernel, dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, stream,
                     entries, gid, n_entries, gid_value, gid_tree, tree_job, N, F, n_gid, n_trees, Q, wide_rows);
  return (int)hipGetLastError();
}

// rows: the M models' training-row lists back to back, row_off [M + 1] their offsets, models [M] their indices
// in [0, P); max_rows = the longest list. F is [P * K][N] fp64, G / H [P * K][N] fp32, y [N] class ids as
// floats, amax (optional) [kAmaxCopies][P * K][2] float bits, err (optional) [P] counters.
int tmog_hip_softmax_grad(const int64_t* rows, const int64_t* row_off, const int64_t* models, int M, int64_t max_rows,
                          int K, int64_t N, int64_t P, const double* F, const float* y, float* G, float* H,
                          uint32_t* amax, int32_t* err, hipStream_t stream) {
  if (M <= 0 || max_rows <= 0) return 0;
  if (K < 2 || K > 64 || M > 65535 || P <= 0 || N <= 0) return -2;
  const int64_t bx = (max_rows + 255) / 256;
  if (bx > 0x7FFFFFFF) return -2;
  hipLaunchKernelGGL(softmax_grad_kernel, dim3((unsigned)bx, (unsigned)M), dim3(256), 0, stream, rows, row_off,
                     models, K, N, P, F, y, G, H, amax, err);
  return (int)hipGetLastError();
}

}  // extern "C"
