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
#include "hip/row_tile.hpp"
#include "common/forest_walk.hpp"

namespace {

using tmog::kTileThreads;

constexpr int SHAP_MAX_M = 64;
constexpr int SHAP_RCP = SHAP_MAX_M + 2;       // rcp[k] = 1 / k, k = 1 .. 65

struct ShapArgs : tmog::RowTile {
  const int64_t* p_off;
  const int32_t* p_out;
  const double* p_val;
  int KV;
  const double* bias;       // [C] sum over paths of value * prod z (row-independent)
  const int32_t* e_feat;
  const int32_t* e_rng;     // tmog::element_satisfied has the layout
  const double* e_z;
  double* out;
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

// What lane e of group g knows of its element for the group's row r (valid: r is a row of the tile; el: the lane
// holds an element, of slot u, range word rng and zero fraction z).
struct ShapRow {
  bool o;                     // the one fraction: the row satisfies the element (true for lanes without one)
  bool dead;                  // an unsatisfied element of zero fraction 0 makes the path's game identically 0
  unsigned long long ones;    // ballot of o over the wave
};
__device__ __forceinline__ ShapRow shap_row(const ShapArgs& a, const uint8_t* sbin, int r, bool valid, bool el,
                                            int u, int rng, double z, unsigned long long gmask) {
  const int b = (valid && el) ? (int)sbin[(size_t)r * a.ustride + u] : 0;
  const bool sat = tmog::element_satisfied(rng, b, a.missing_bin);
  const bool o = !el || sat;
  const bool dead = (__ballot(el && !sat && z == 0.0) & gmask) != 0;
  return ShapRow{o, dead, __ballot(o)};
}

// One EXTEND step: lane e holds w[e]; step s adds an element of zero fraction zl and one fraction ol, rs = 1 / (s + 1).
template <int W>
__device__ __forceinline__ double shap_extend(double w, int e, int s, double zl, bool ol, double rs) {
  const double wp = shap_shift_up<W>(w, e);
  return (zl * w * (double)(s - e) + (ol ? wp * (double)e : 0.0)) * rs;
}

// The UNWOUND sum of this lane's element (one fraction o, zero fraction z, invz = 1 / z or 0) over a path of len
// elements whose weights w[j] sit in lane j of the group; top = w[len], scaled by 1 / (len + 1) as the result is.
// rcp(k) gives 1 / k from wherever the caller keeps it. The broadcasts do not depend on the running sums: four are
// kept in flight.
template <int W, class Rcp>
__device__ __forceinline__ double shap_unwound(double w, int len, bool o, double z, double invz, double top,
                                               Rcp rcp) {
  double next = top, total = 0.0;
  auto unwind = [&](int j, double wj) {
    const double rj = rcp(j + 1), rmj = rcp(len - j);
    if (o) {
      const double tmp = next * rj;
      total += tmp;
      next = wj - tmp * z * (double)(len - j);
    } else {
      total += wj * invz * rmj;
    }
  };
  int j = len - 1;
  for (; j >= 3; j -= 4) {
    const double w0 = __shfl(w, j, W), w1 = __shfl(w, j - 1, W), w2 = __shfl(w, j - 2, W), w3 = __shfl(w, j - 3, W);
    unwind(j, w0);
    unwind(j - 1, w1);
    unwind(j - 2, w2);
    unwind(j - 3, w3);
  }
  for (; j >= 0; --j) unwind(j, __shfl(w, j, W));
  return total;
}

template <int W>
__device__ __forceinline__ void shap_paths(const ShapArgs& a, int64_t p0, int64_t p1, int nrow,
                                           unsigned long long* acc, const double* rcp, const uint8_t* sbin) {
  constexpr int G = 64 / W;
  const int lane = threadIdx.x & 63;
  const int e = lane & (W - 1), g = lane / W;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = kTileThreads / 64;
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
    const int col = a.p_out[p];
    const double* val = a.p_val + p * a.KV;
    const double rtop = rcp[m + 1];
    for (int r0 = 0; r0 < nrow; r0 += G) {
      const int r = r0 + g;
      const bool valid = r < nrow;
      const ShapRow row = shap_row(a, sbin, r, valid, el, u, rng, z, gmask);
      const bool o = row.o, dead = row.dead;
      const bool all_one = (~row.ones & gmask) == 0;
      // EXTEND: lane e holds w[e], e < m; step l adds element l - 1; its zero fraction is a wave-uniform load
      double w = e == 0 ? 1.0 : 0.0;
      for (int l = 1; l <= m; ++l)
        w = shap_extend<W>(w, e, l, a.e_z[eo + l - 1], (row.ones >> (g * W + l - 1)) & 1ull, rcp[l + 1]);
      const double total = shap_unwound<W>(w, m, o, z, invz, all_one ? rtop : 0.0, [&](int k) { return rcp[k]; });
      const double phi = total * (double)(m + 1) * ((o ? 1.0 : 0.0) - z);
      if (valid && !dead && el) {
        unsigned long long* dst = acc + (size_t)r * slots;
        for (int c = 0; c < a.KV; ++c)
          atomicAdd(dst + (size_t)u * a.C + col + c, (unsigned long long)__double2ll_rn(phi * val[c] * a.scale));
      }
    }
  }
}

__global__ void __launch_bounds__(kTileThreads) forest_shap_kernel(ShapArgs a, int64_t b0, int64_t b1, int64_t b2,
                                                                   int64_t b3) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t blk0 = tmog::tile_first_row(a);
  if (blk0 >= a.n) return;
  const int nrow = tmog::tile_row_count(a, blk0);
  const size_t nacc = shap_acc_elems(a.tile_rows, a.U, a.C);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);
  double* rcp = reinterpret_cast<double*>(smem + nacc * 8);
  uint8_t* sbin = smem + nacc * 8 + SHAP_RCP * 8;
  tmog::zero_tile(acc, nacc);
  if (threadIdx.x < SHAP_RCP) rcp[threadIdx.x] = threadIdx.x ? 1.0 / (double)threadIdx.x : 0.0;
  tmog::stage_used_bins(a, blk0, nrow, sbin);
  __syncthreads();
  shap_paths<16>(a, b0, b1, nrow, acc, rcp, sbin);
  shap_paths<32>(a, b1, b2, nrow, acc, rcp, sbin);
  shap_paths<64>(a, b2, b3, nrow, acc, rcp, sbin);
  __syncthreads();
  const size_t nout = shap_acc_elems(nrow, a.U, a.C);
  const double inv = 1.0 / a.scale;
  double* o = a.out + (size_t)blk0 * (a.U + 1) * a.C;
  const size_t slots = (size_t)(a.U + 1) * a.C, first_bias = (size_t)a.U * a.C;
  for (size_t i = threadIdx.x; i < nout; i += kTileThreads) {
    const size_t k = i % slots;
    o[i] = k >= first_bias ? a.bias[k - first_bias] : tmog::tile_value(acc[i], inv);
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
  const int nwaves = kTileThreads / 64;
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
      // the conditioning positions of this chunk: every group holds the same path, group 0's bits serve
      const unsigned long long cond = __ballot(el && u >= c0 && u < c1) & wmask;
      const int col = a.p_out[p];
      const double* val = a.p_val + p * a.KV;
      const double rtop = shap_lane(rl, m - 1);
      for (int r0 = 0; r0 < nrow; r0 += G) {
        const int r = r0 + g;
        const bool valid = r < nrow;
        const ShapRow row = shap_row(a, sbin, r, valid, el, u, rng, z, gmask);
        const bool o = row.o, dead = row.dead;
        const unsigned long long ones = row.ones;
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
            w = shap_extend<W>(w, e, s, shap_lane(z, l), (ones >> (g * W + l)) & 1ull, shap_lane(rl, s));
          }
          // UNWOUND of this lane's element on the sub-path of m - 1 elements
          const double total = shap_unwound<W>(w, m - 1, o, z, invz, all_one ? rtop : 0.0,
                                               [&](int k) { return shap_lane(rl, k - 1); });
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
__global__ void __launch_bounds__(kTileThreads) forest_shap_pair_kernel(ShapArgs a, int UB, int64_t b0, int64_t b1,
                                                                        int64_t b2, int64_t b3) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t blk0 = tmog::tile_first_row(a);
  const int c0 = (int)blockIdx.y * UB;
  if (blk0 >= a.n || c0 >= a.U) return;
  const int nrow = tmog::tile_row_count(a, blk0);
  const int c1 = min(c0 + UB, a.U);
  const size_t nacc = shap_pair_elems(a.tile_rows, UB, a.U, a.C);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);
  uint8_t* sbin = smem + nacc * 8;
  tmog::zero_tile(acc, nacc);
  tmog::stage_used_bins(a, blk0, nrow, sbin);
  __syncthreads();
  shap_pair_paths<16>(a, UB, c0, c1, b0, b1, nrow, acc, sbin);
  shap_pair_paths<32>(a, UB, c0, c1, b1, b2, nrow, acc, sbin);
  shap_pair_paths<64>(a, UB, c0, c1, b2, b3, nrow, acc, sbin);
  __syncthreads();
  const double inv = 1.0 / a.scale;
  const size_t per = (size_t)(c1 - c0) * a.U * a.C, rstride = (size_t)UB * a.U * a.C;
  for (int r = 0; r < nrow; ++r)
    tmog::store_tile_fp64(a.out + ((size_t)(blk0 + r) * a.U + c0) * a.U * a.C, acc + (size_t)r * rstride, per, inv);
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
  const int ustride = tmog::ustride_of(U);
  auto bytes = [&](int rows) { return shap_lds_bytes(rows, U, C, ustride); };
  if (bytes(1) > tmog::kTileLdsLimit) return -3;
  const int rows = tmog::pick_tile_rows(bytes);
  ShapArgs a{{Xb, F, n, row_list, U, used, C, scale, missing_bin, rows, ustride}, p_off, p_out, p_val, KV, bias,
             e_feat, e_rng, e_z, out};
  return tmog::launch_lds<forest_shap_kernel>((n + rows - 1) / rows, 1, bytes(rows), stream, a, bin_off[0],
                                              bin_off[1], bin_off[2], bin_off[3]);
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
  const int ustride = tmog::ustride_of(U);
  auto bytes = [&](int rows, int UB) { return shap_pair_lds_bytes(rows, UB, U, C, ustride); };
  if (bytes(1, 1) > tmog::kTileLdsLimit) return -3;
  size_t budget = tmog::kTileLdsShare;
  int rows = 8;
  while (rows > 1 && bytes(rows, 1) > budget) rows >>= 1;
  if (bytes(rows, 1) > budget) budget = tmog::kTileLdsLimit;   // rows == 1
  const size_t unit = (size_t)rows * U * C * 8;
  const int UB = (int)std::min<size_t>((size_t)U, (budget - (size_t)rows * ustride) / unit);
  if (UB == U)
    while (rows < tmog::kTileMaxRows && bytes(rows * 2, U) <= tmog::kTileLdsShare) rows <<= 1;
  ShapArgs a{{Xb, F, n, row_list, U, used, C, scale, missing_bin, rows, ustride}, p_off, p_out, p_val, KV, bias,
             e_feat, e_rng, e_z, tri};
  return tmog::launch_lds<forest_shap_pair_kernel>((n + rows - 1) / rows, (U + UB - 1) / UB, bytes(rows, UB), stream,
                                                   a, UB, bin_off[0], bin_off[1], bin_off[2], bin_off[3]);
}

}  // extern "C"
