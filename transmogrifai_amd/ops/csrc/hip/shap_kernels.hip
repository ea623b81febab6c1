// Exact path-dependent TreeSHAP for the flat forests of the tree engine, CDNA4 (gfx950).
//
// The host (models/tree_engine.py forest_paths) unrolls every tree into one path per leaf. A feature that
// repeats on a path is merged into one element: compact "used feature" index u, inclusive bin interval
// [lo, hi], whether the missing bin satisfies it, and the zero fraction z (product of the cover ratios of
// the merged nodes). For one (row, path) the element's one fraction o is 1 when the row's bin satisfies
// the element and 0 otherwise, the path's game is g(S) = v * prod_{e in S} o_e * prod_{e not in S} z_e,
// and the Shapley value of element e is v * (o_e - z_e) * UNWOUND_e(w) with w the permutation weights
// built by EXTEND over the path's elements (Lundberg et al. 2018, Algorithm 2). The bias, sum v * prod z over
// the paths, does not depend on the row: the host sums it once and the kernel stores it into slot U.
//
// Mapping: a workgroup owns a tile of rows, stages the used features' bins of its rows in LDS and loops
// over all paths (shared by every workgroup, L2 resident). One sub-wave lane group of W = 16 / 32 / 64
// lanes (template parameter, one instantiation per path-length bin) serves one (row, path), one lane per
// path element: lane e keeps w[e] in a register, EXTEND shifts the weights one lane up (DPP / __shfl_up; the
// new element's zero fraction is a wave-uniform load, its one fraction a bit of a ballot), UNWOUND broadcasts
// w[j] with __shfl and keeps each element's running sum in its own lane. The top weight w[m] is
// prod o / (m + 1) in closed form, so m <= W lanes hold the m + 1 weights. All groups of a wave work on the
// same path (different rows): element loads are wave-uniform broadcasts and the loop trip counts are
// uniform. Everything is fp64.
//
// Accumulation is order-independent, hence bitwise reproducible: each contribution is rounded to int64
// fixed point (scale = the power of two with S * scale < 2^62, S = sum_t |w_t| max |value_t|; a row's
// partial sums stay below 2 S) and added to the workgroup's LDS tile [rows][U + 1][C] with 64-bit LDS
// integer atomics; the tile is converted to fp64 and stored with plain stores at the end.
//
// The second kernel of this file computes the SHAP interaction values on the same mapping (see below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hip/tmog_hip_abi.h"

namespace {

constexpr int SHAP_THREADS = 512;
constexpr int SHAP_MAX_ROWS = 64;
constexpr int SHAP_MAX_M = 64;
constexpr size_t SHAP_LDS_LIMIT = 160 * 1024;
constexpr size_t SHAP_LDS_SHARE = 80 * 1024;   // two workgroups per CU while the tile stays >= 16 rows
constexpr int SHAP_RCP = SHAP_MAX_M + 2;       // rcp[k] = 1 / k, k = 1 .. 65

struct ShapArgs {
  const uint8_t* Xb;
  int F;
  int64_t n;
  const int32_t* row_list;
  int U;
  const int32_t* used;
  const int64_t* p_off;
  const int32_t* p_out;
  const double* p_val;
  int KV;
  const double* bias;       // [C] sum over paths of value * prod z (row-independent)
  const int32_t* e_feat;
  const int32_t* e_rng;     // lo | hi << 12 | missing-satisfies << 24
  const double* e_z;
  int missing_bin;
  int C;
  double scale;
  double* out;
  int tile_rows;
  int ustride;              // bytes per staged row (U rounded up to 4)
};

__device__ __forceinline__ size_t shap_acc_elems(int rows, int U, int C) { return (size_t)rows * (U + 1) * C; }

// w of the lane below in the group (0 for the group's first lane). W = 16: a DPP row shift (row_shr:1, rows are
// the 16-lane groups, lanes shifted in from outside the row read 0), else a shuffle through the LDS crossbar.
template <int W>
__device__ __forceinline__ double shap_shift_up(double w, int e) {
  if constexpr (W == 16) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(w), 0x111, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(w), 0x111, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
  } else {
    const double wp = __shfl_up(w, 1, W);
    return e == 0 ? 0.0 : wp;
  }
}

template <int W>
__device__ __forceinline__ void shap_paths(const ShapArgs& a, int64_t p0, int64_t p1, int nrow,
                                           unsigned long long* acc, const double* rcp, const uint8_t* sbin) {
  constexpr int G = 64 / W;
  const int lane = threadIdx.x & 63;
  const int e = lane & (W - 1), g = lane / W;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = SHAP_THREADS / 64;
  const unsigned long long gmask = (W == 64 ? ~0ull : ((1ull << W) - 1ull)) << (g * W);
  const int slots = (a.U + 1) * a.C;
  for (int64_t p = p0 + wave; p < p1; p += nwaves) {
    const int64_t eo = a.p_off[p];
    const int m = (int)(a.p_off[p + 1] - eo);            // wave-uniform, <= W
    const bool el = e < m;
    const int u = el ? a.e_feat[eo + e] : 0;
    const int rng = el ? a.e_rng[eo + e] : 0;
    const double z = el ? a.e_z[eo + e] : 1.0;
    const double invz = z != 0.0 ? 1.0 / z : 0.0;
    const int lo = rng & 0xFFF, hi = (rng >> 12) & 0xFFF, miss_ok = (rng >> 24) & 1;
    const int col = a.p_out[p];
    const double* val = a.p_val + p * a.KV;
    const double rtop = rcp[m + 1];
    for (int r0 = 0; r0 < nrow; r0 += G) {
      const int r = r0 + g;
      const bool valid = r < nrow;
      const int b = (valid && el) ? (int)sbin[(size_t)r * a.ustride + u] : 0;
      const bool sat = (a.missing_bin >= 0 && b == a.missing_bin) ? (miss_ok != 0) : (lo <= b && b <= hi);
      const bool o = !el || sat;
      // an unsatisfied element of zero fraction 0 makes the path's game identically 0 for this row
      const bool dead = (__ballot(el && !sat && z == 0.0) & gmask) != 0;
      const unsigned long long ones = __ballot(o);
      const bool all_one = (~ones & gmask) == 0;
      // EXTEND: lane e holds w[e], e < m; step l adds element l (held by lane l - 1)
      double w = e == 0 ? 1.0 : 0.0;
      for (int l = 1; l <= m; ++l) {
        const double zl = a.e_z[eo + l - 1];
        const bool ol = (ones >> (g * W + l - 1)) & 1ull;
        const double wp = shap_shift_up<W>(w, e);
        w = (zl * w * (double)(l - e) + (ol ? wp * (double)e : 0.0)) * rcp[l + 1];
      }
      // UNWOUND sum of this lane's element (scaled by 1 / (m + 1) until the end)
      double next = all_one ? rtop : 0.0, total = 0.0;
      auto unwind = [&](int j, double wj) {
        if (o) {
          const double tmp = next * rcp[j + 1];
          total += tmp;
          next = wj - tmp * z * (double)(m - j);
        } else {
          total += wj * invz * rcp[m - j];
        }
      };
      int j = m - 1;
      for (; j >= 3; j -= 4) {      // the broadcasts do not depend on the running sums: four in flight
        const double w0 = __shfl(w, j, W), w1 = __shfl(w, j - 1, W), w2 = __shfl(w, j - 2, W),
                     w3 = __shfl(w, j - 3, W);
        unwind(j, w0);
        unwind(j - 1, w1);
        unwind(j - 2, w2);
        unwind(j - 3, w3);
      }
      for (; j >= 0; --j) unwind(j, __shfl(w, j, W));
      const double phi = total * (double)(m + 1) * ((o ? 1.0 : 0.0) - z);
      if (valid && !dead && el) {
        unsigned long long* dst = acc + (size_t)r * slots;
        for (int c = 0; c < a.KV; ++c)
          atomicAdd(dst + (size_t)u * a.C + col + c, (unsigned long long)__double2ll_rn(phi * val[c] * a.scale));
      }
    }
  }
}

__global__ void __launch_bounds__(SHAP_THREADS) forest_shap_kernel(ShapArgs a, int64_t b0, int64_t b1, int64_t b2,
                                                                   int64_t b3) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t blk0 = (int64_t)blockIdx.x * a.tile_rows;
  if (blk0 >= a.n) return;
  const int nrow = (int)min((int64_t)a.tile_rows, a.n - blk0);
  const size_t nacc = shap_acc_elems(a.tile_rows, a.U, a.C);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);
  double* rcp = reinterpret_cast<double*>(smem + nacc * 8);
  uint8_t* sbin = smem + nacc * 8 + SHAP_RCP * 8;
  for (size_t i = threadIdx.x; i < nacc; i += SHAP_THREADS) acc[i] = 0ull;
  if (threadIdx.x < SHAP_RCP) rcp[threadIdx.x] = threadIdx.x ? 1.0 / (double)threadIdx.x : 0.0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < nrow; r += SHAP_THREADS / 64) {
    const int64_t row = a.row_list ? a.row_list[blk0 + r] : (blk0 + r);
    const uint8_t* src = a.Xb + row * (int64_t)a.F;
    for (int k = lane; k < a.U; k += 64) sbin[(size_t)r * a.ustride + k] = src[a.used[k]];
  }
  __syncthreads();
  shap_paths<16>(a, b0, b1, nrow, acc, rcp, sbin);
  shap_paths<32>(a, b1, b2, nrow, acc, rcp, sbin);
  shap_paths<64>(a, b2, b3, nrow, acc, rcp, sbin);
  __syncthreads();
  const size_t nout = shap_acc_elems(nrow, a.U, a.C);
  const double inv = 1.0 / a.scale;
  double* o = a.out + (size_t)blk0 * (a.U + 1) * a.C;
  const size_t slots = (size_t)(a.U + 1) * a.C, first_bias = (size_t)a.U * a.C;
  for (size_t i = threadIdx.x; i < nout; i += SHAP_THREADS) {
    const size_t k = i % slots;
    o[i] = k >= first_bias ? a.bias[k - first_bias] : (double)(long long)acc[i] * inv;
  }
}

size_t shap_lds_bytes(int rows, int U, int C, int ustride) {
  return (size_t)rows * (U + 1) * C * 8 + SHAP_RCP * 8 + (size_t)rows * ustride;
}

// ------------------------------------------------------------------------------------ interaction values
// SHAP interaction values on the same paths and the same lane mapping. For two elements i != j of a path the
// Shapley interaction index of the path's game is
//   Phi_ij = 1/2 * (o_i - z_i) * phi_j(path \ {i}),
// phi_j(path \ {i}) the TreeSHAP value of element j on the path without element i (same value vector): the
// game is a product over the elements, so fixing i in or out factors (o_i - z_i) out of every difference the
// index averages, and what is left is the Shapley value of j among the other m - 1 elements. For every
// conditioning position i the group runs EXTEND over the other m - 1 elements (top weight prod_{e != i} o_e / m
// in closed form) and UNWOUND with sub-path length m - 1 in every lane e != i; i, z_i and the trip counts are
// wave-uniform, o_i is a bit of the group's ballot. Each unordered pair is stored once, by the lane of the
// larger compact feature index: cell (u_i, u_e) with u_i < u_e of tri [n][U][U][C]; the host adds the
// transpose, the diagonal (phi_i minus the row's pair sums) and the bias.
//
// A [U][U][C] tile per row does not fit the LDS for real models, so the conditioning feature is tiled too:
// gridDim.y runs over chunks of UB consecutive compact feature indices, the workgroup's tile is int64
// [rows][UB][U][C] (plus the staged bins) and it runs only the conditioning positions whose u_i lies in its chunk. Every workgroup
// still walks all paths; to find the few that have an element in its chunk a wave scans 64 paths at a time,
// one path per lane, and then serves the hits one by one.
//
// Fixed point: the scale of forest_shap serves. Any partial sum of a cell over a set Q of paths is the
// interaction index of the game sum_{p in Q} g_p, a weighted mean (weights summing to 1/2) of the four-term
// differences g(S + ij) - g(S + i) - g(S + j) + g(S) with |g| <= S: below 2 S, as for forest_shap.
__device__ __forceinline__ size_t shap_pair_elems(int rows, int UB, int U, int C) {
  return (size_t)rows * UB * U * C;
}

// v of lane `lane` of the wave (wave-uniform index): a register read, no memory access
__device__ __forceinline__ double shap_lane(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                          __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// The inner loops touch no memory: every group holds the same path, so the zero fraction and the feature of a
// wave-uniform position are read from that lane of group 0, and 1 / k from lane k - 1 of a reciprocal register.
template <int W>
__device__ __forceinline__ void shap_pair_paths(const ShapArgs& a, int UB, int c0, int c1, int64_t p0, int64_t p1,
                                                int nrow, unsigned long long* acc, const uint8_t* sbin) {
  constexpr int G = 64 / W;
  const int lane = threadIdx.x & 63;
  const int e = lane & (W - 1), g = lane / W;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = SHAP_THREADS / 64;
  const unsigned long long wmask = W == 64 ? ~0ull : ((1ull << W) - 1ull);
  const unsigned long long gmask = wmask << (g * W);
  const size_t rstride = (size_t)UB * a.U * a.C;
  const double rl = 1.0 / (double)(lane + 1);            // shap_lane(rl, k - 1) = 1 / k, k = 1 .. 64
  for (int64_t pb = p0 + (int64_t)wave * 64; pb < p1; pb += (int64_t)nwaves * 64) {
    // scan: lane k looks for an element of path pb + k inside the chunk
    bool hit = false;
    if (pb + lane < p1) {
      const int64_t so = a.p_off[pb + lane];
      const int sm = (int)(a.p_off[pb + lane + 1] - so);
      if (sm >= 2)
        for (int t = 0; t < sm; ++t) {
          const int f = a.e_feat[so + t];
          hit = hit || (f >= c0 && f < c1);
        }
    }
    for (unsigned long long hits = __ballot(hit); hits; hits &= hits - 1ull) {
      const int64_t p = pb + __builtin_ctzll(hits);
      const int64_t eo = a.p_off[p];
      const int m = (int)(a.p_off[p + 1] - eo);            // wave-uniform, 2 <= m <= W
      const bool el = e < m;
      const int u = el ? a.e_feat[eo + e] : 0;
      const int rng = el ? a.e_rng[eo + e] : 0;
      const double z = el ? a.e_z[eo + e] : 1.0;
      const double invz = z != 0.0 ? 1.0 / z : 0.0;
      const int lo = rng & 0xFFF, hi = (rng >> 12) & 0xFFF, miss_ok = (rng >> 24) & 1;
      // the conditioning positions of this chunk: every group holds the same path, group 0's bits serve
      const unsigned long long cond = __ballot(el && u >= c0 && u < c1) & wmask;
      const int col = a.p_out[p];
      const double* val = a.p_val + p * a.KV;
      const double rtop = shap_lane(rl, m - 1);
      for (int r0 = 0; r0 < nrow; r0 += G) {
        const int r = r0 + g;
        const bool valid = r < nrow;
        const int b = (valid && el) ? (int)sbin[(size_t)r * a.ustride + u] : 0;
        const bool sat = (a.missing_bin >= 0 && b == a.missing_bin) ? (miss_ok != 0) : (lo <= b && b <= hi);
        const bool o = !el || sat;
        const bool dead = (__ballot(el && !sat && z == 0.0) & gmask) != 0;
        const unsigned long long ones = __ballot(o);
        const double oz = (o ? 1.0 : 0.0) - z;
        for (unsigned long long cm = cond; cm; cm &= cm - 1ull) {
          const int i = __builtin_ctzll(cm);               // wave-uniform
          const int ui = __builtin_amdgcn_readlane(u, i);
          const double zi = shap_lane(z, i);
          const unsigned long long ibit = 1ull << (g * W + i);
          const double oi = (ones & ibit) ? 1.0 : 0.0;
          const bool all_one = (~ones & gmask & ~ibit) == 0;
          // EXTEND over the elements other than i: step s adds element s - 1 (s <= i) or s (s > i)
          double w = e == 0 ? 1.0 : 0.0;
          for (int s = 1; s < m; ++s) {
            const int l = s <= i ? s - 1 : s;
            const double zl = shap_lane(z, l);
            const bool ol = (ones >> (g * W + l)) & 1ull;
            const double wp = shap_shift_up<W>(w, e);
            w = (zl * w * (double)(s - e) + (ol ? wp * (double)e : 0.0)) * shap_lane(rl, s);
          }
          // UNWOUND of this lane's element on the sub-path of m - 1 elements
          double next = all_one ? rtop : 0.0, total = 0.0;
          auto unwind = [&](int j, double wj) {
            const double rj = shap_lane(rl, j), rmj = shap_lane(rl, m - 2 - j);   // 1 / (j + 1), 1 / (m - 1 - j)
            if (o) {
              const double tmp = next * rj;
              total += tmp;
              next = wj - tmp * z * (double)(m - 1 - j);
            } else {
              total += wj * invz * rmj;
            }
          };
          int j = m - 2;
          for (; j >= 3; j -= 4) {
            const double w0 = __shfl(w, j, W), w1 = __shfl(w, j - 1, W), w2 = __shfl(w, j - 2, W),
                         w3 = __shfl(w, j - 3, W);
            unwind(j, w0);
            unwind(j - 1, w1);
            unwind(j - 2, w2);
            unwind(j - 3, w3);
          }
          for (; j >= 0; --j) unwind(j, __shfl(w, j, W));
          const double pair = total * (double)m * oz * 0.5 * (oi - zi);
          if (valid && !dead && el && u > ui) {            // u > ui: each pair once, and never e == i
            unsigned long long* dst = acc + (size_t)r * rstride + ((size_t)(ui - c0) * a.U + u) * a.C + col;
            for (int c = 0; c < a.KV; ++c)
              atomicAdd(dst + c, (unsigned long long)__double2ll_rn(pair * val[c] * a.scale));
          }
        }
      }
    }
  }
}

// a.out is tri [n][U][U][C]; blockIdx.x: row tile, blockIdx.y: chunk of UB conditioning features
__global__ void __launch_bounds__(SHAP_THREADS) forest_shap_pair_kernel(ShapArgs a, int UB, int64_t b0, int64_t b1,
                                                                        int64_t b2, int64_t b3) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t blk0 = (int64_t)blockIdx.x * a.tile_rows;
  const int c0 = (int)blockIdx.y * UB;
  if (blk0 >= a.n || c0 >= a.U) return;
  const int nrow = (int)min((int64_t)a.tile_rows, a.n - blk0);
  const int c1 = min(c0 + UB, a.U);
  const size_t nacc = shap_pair_elems(a.tile_rows, UB, a.U, a.C);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);
  uint8_t* sbin = smem + nacc * 8;
  for (size_t i = threadIdx.x; i < nacc; i += SHAP_THREADS) acc[i] = 0ull;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < nrow; r += SHAP_THREADS / 64) {
    const int64_t row = a.row_list ? a.row_list[blk0 + r] : (blk0 + r);
    const uint8_t* src = a.Xb + row * (int64_t)a.F;
    for (int k = lane; k < a.U; k += 64) sbin[(size_t)r * a.ustride + k] = src[a.used[k]];
  }
  __syncthreads();
  shap_pair_paths<16>(a, UB, c0, c1, b0, b1, nrow, acc, sbin);
  shap_pair_paths<32>(a, UB, c0, c1, b1, b2, nrow, acc, sbin);
  shap_pair_paths<64>(a, UB, c0, c1, b2, b3, nrow, acc, sbin);
  __syncthreads();
  const double inv = 1.0 / a.scale;
  const size_t per = (size_t)(c1 - c0) * a.U * a.C, rstride = (size_t)UB * a.U * a.C;
  for (int r = 0; r < nrow; ++r) {
    double* o = a.out + ((size_t)(blk0 + r) * a.U + c0) * a.U * a.C;
    const unsigned long long* src = acc + (size_t)r * rstride;
    for (size_t k = threadIdx.x; k < per; k += SHAP_THREADS) o[k] = (double)(long long)src[k] * inv;
  }
}

size_t shap_pair_lds_bytes(int rows, int UB, int U, int C, int ustride) {
  return (size_t)rows * UB * U * C * 8 + (size_t)rows * ustride;
}

}  // namespace

extern "C" {

// out[i][U + 1][C] (fp64) for rows row_list[0 .. n) (row_list == nullptr: rows 0 .. n-1) of Xb [.][F].
// Paths p in [0, P): elements [p_off[p], p_off[p+1]), value p_val[p][KV] added to columns p_out[p] + c;
// bias[C] is the row-independent bias (slot U); bin_off is host memory:
// bin_off[0..3] bounds the paths of length <= 16, <= 32, <= 64 (bin_off[3] = P once no path is longer).
// Returns -2 when a path has more than 64 elements, -3 when one row's tile exceeds the LDS limit.
int tmog_hip_forest_shap(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                         int64_t P, const int64_t* p_off, const int32_t* p_out, const double* p_val, int KV,
                         const double* bias, const int32_t* e_feat, const int32_t* e_rng, const double* e_z,
                         const int64_t* bin_off, int missing_bin, int C, double scale, double* out,
                         hipStream_t stream) {
  if (n == 0) return 0;
  if (bin_off[3] != P) return -2;
  const int ustride = (U + 3) & ~3;
  if (shap_lds_bytes(1, U, C, ustride) > SHAP_LDS_LIMIT) return -3;
  int rows = SHAP_MAX_ROWS;
  while (rows > 16 && shap_lds_bytes(rows, U, C, ustride) > SHAP_LDS_SHARE) rows >>= 1;
  while (rows > 1 && shap_lds_bytes(rows, U, C, ustride) > SHAP_LDS_LIMIT) rows >>= 1;
  ShapArgs a{Xb, F, n, row_list, U, used, p_off, p_out, p_val, KV, bias, e_feat, e_rng, e_z, missing_bin, C,
             scale, out, rows, ustride};
  const size_t lds = shap_lds_bytes(rows, U, C, ustride);
  static const bool lds_attr = hipFuncSetAttribute((const void*)forest_shap_kernel,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)SHAP_LDS_LIMIT) == hipSuccess;   // once per process
  if (lds > 64 * 1024 && !lds_attr) return -3;
  const int64_t blocks = (n + rows - 1) / rows;
  if (blocks > 0x7FFFFFFF) return -4;
  hipLaunchKernelGGL(forest_shap_kernel, dim3((unsigned)blocks), dim3(SHAP_THREADS), lds, stream, a, bin_off[0],
                     bin_off[1], bin_off[2], bin_off[3]);
  return (int)hipGetLastError();
}

// Pair sums of the SHAP interaction values: tri[i][U][U][C] (fp64, every cell written), the unordered pair of
// compact features u < v counted once, in cell (u, v); everything else as tmog_hip_forest_shap (bias is not read).
// The tile is rows x UB conditioning features, sized from the LDS budget: 8 rows and as many features as fit the
// two-workgroup share; when all U fit, more rows; when not even one does, fewer rows, and at one row the whole
// limit. Returns -2 when a path has more than 64 elements, -3 when one row x one feature exceeds the LDS limit.
int tmog_hip_forest_shap_interactions(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U,
                                      const int32_t* used, int64_t P, const int64_t* p_off, const int32_t* p_out,
                                      const double* p_val, int KV, const double* bias, const int32_t* e_feat,
                                      const int32_t* e_rng, const double* e_z, const int64_t* bin_off,
                                      int missing_bin, int C, double scale, double* tri, hipStream_t stream) {
  if (n == 0 || U == 0) return 0;
  if (bin_off[3] != P) return -2;
  const int ustride = (U + 3) & ~3;
  if (shap_pair_lds_bytes(1, 1, U, C, ustride) > SHAP_LDS_LIMIT) return -3;
  size_t budget = SHAP_LDS_SHARE;
  int rows = 8;
  while (rows > 1 && shap_pair_lds_bytes(rows, 1, U, C, ustride) > budget) rows >>= 1;
  if (shap_pair_lds_bytes(rows, 1, U, C, ustride) > budget) budget = SHAP_LDS_LIMIT;   // rows == 1
  const size_t unit = (size_t)rows * U * C * 8;
  int UB = (int)std::min<size_t>((size_t)U, (budget - (size_t)rows * ustride) / unit);
  if (UB == U)
    while (rows < SHAP_MAX_ROWS && shap_pair_lds_bytes(rows * 2, U, U, C, ustride) <= SHAP_LDS_SHARE) rows <<= 1;
  ShapArgs a{Xb, F, n, row_list, U, used, p_off, p_out, p_val, KV, bias, e_feat, e_rng, e_z, missing_bin, C,
             scale, tri, rows, ustride};
  const size_t lds = shap_pair_lds_bytes(rows, UB, U, C, ustride);
  static const bool lds_attr = hipFuncSetAttribute((const void*)forest_shap_pair_kernel,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)SHAP_LDS_LIMIT) == hipSuccess;   // once per process
  if (lds > 64 * 1024 && !lds_attr) return -3;
  const int64_t blocks = (n + rows - 1) / rows;
  const int chunks = (U + UB - 1) / UB;
  if (blocks > 0x7FFFFFFF || chunks > 65535) return -4;
  hipLaunchKernelGGL(forest_shap_pair_kernel, dim3((unsigned)blocks, (unsigned)chunks), dim3(SHAP_THREADS), lds,
                     stream, a, UB, bin_off[0], bin_off[1], bin_off[2], bin_off[3]);
  return (int)hipGetLastError();
}

}  // extern "C"
