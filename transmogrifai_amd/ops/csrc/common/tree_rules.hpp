// The arithmetic and decision rules of the tree engine that have a host and a device twin, written once. The CPU
// grower (host/tree_cpu.cpp), the host-planned HIP grower (common/tree_grow.hpp + hip/tree_*_kernels.hip) and the
// device-planned grower (hip/tree_resident.hip) promise the same trees bit for bit: all of them evaluate the functions
// below, so a rule cannot change on one backend only. Stateless free functions of scalar arguments.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define TMOG_HD __host__ __device__ __forceinline__
#else
#define TMOG_HD inline
#endif
// Opens every body that does floating-point arithmetic or compares: no FMA contraction, so both sides run the same IEEE
// operation sequence and near-tied candidates resolve identically (hipcc contracts by default; g++ is built with
// -ffp-contract=off). Function-local: includers keep their setting. (Plumbing, as for_stats and fp_put / fp_get.)
#ifdef __clang__
#define TMOG_FP_EXACT _Pragma("clang fp contract(off)")
#else
#define TMOG_FP_EXACT
#endif

namespace tmog {

// Eight floats per histogram node, written by the level planners (grow_group, level_plan_kernel), read by the
// split scans, the partition and the host's decisions.
enum : int {
  kPrmMinInst,        // min_instances: smallest child count (impurity kinds)
  kPrmMinGain,        // min_info_gain (impurity kinds)
  kPrmMcw,            // min_child_weight: smallest child hessian sum (Newton)
  kPrmLambda,         // L2 regularisation of the Newton gain
  kPrmPaired,         // 1: scanned with its subtraction partner by pair_scan_kernel, the node-wise scan skips it
  kPrmAllowMissing,   // 1: search the default direction of the missing bin (XGBoost)
  kPrmEps,            // a recorded split is accepted only with gain > eps
  kPrmMaySplit,       // 0: built only as a subtraction partner (or unsplittable): not scanned, never splits
  kPrmStride = 8
};

struct SplitCand {
  double gain;
  int f;    // local feature index; in a feature-parallel record the position in the full feature list (tie-break)
  int b;
  int dl;
  static constexpr int kNoFeature = 0x7fffffff;
  static TMOG_HD SplitCand none() { return SplitCand{-INFINITY, kNoFeature, 0, 0}; }
  TMOG_HD bool found() const { return f != kNoFeature; }
};
static_assert(sizeof(SplitCand) == 24, "candidate record: three 8-byte words (store_best_sc1 / load_best_sc1)");

// The candidate order: gain descending, then feature, dl and bin ascending -- the first maximum of the CPU
// twin's (feature, dl, bin) scan order.
TMOG_HD bool better(const SplitCand& a, const SplitCand& b) {
  TMOG_FP_EXACT
  if (a.gain != b.gain) return a.gain > b.gain;
  if (a.f != b.f) return a.f < b.f;
  if (a.dl != b.dl) return a.dl < b.dl;
  return a.b < b.b;
}

// body(s) for every statistic s < S: tree_split_kernels.hip's TM_FOR_S as a function (the macro stays there for the
// scans' statement bodies). SM > 0: unrolled to the compile-time bound with a run-time guard, so arrays indexed by s stay in
// registers (a loop to the run-time S indexes them dynamically: scratch memory). SM == 0: the plain run-time loop.
template <int SM, class Body>
TMOG_HD void for_stats(int S, Body body) {
  if constexpr (SM > 0) {
#ifdef __clang__
#pragma unroll
#endif
    for (int s = 0; s < SM; ++s) if (s < S) body(s);
  } else {
    for (int s = 0; s < S; ++s) body(s);
  }
}

// Impurity of a node whose scaled statistic s is get(s); *count receives its row weight (Newton: hessian sum).
// Kinds: 0 gini, 1 entropy (S class weights), 2 variance (w, w t, w t t), 3 newton (no impurity: gain below).
template <int SM, class Get>
TMOG_HD double impurity(Get get, int S, int kind, double* count) {
  TMOG_FP_EXACT
  if (kind == 0 || kind == 1) {
    double n = 0;
    for_stats<SM>(S, [&](int s) { TMOG_FP_EXACT n += get(s); });
    *count = n;
    if (n <= 0) return 0.0;
    double imp = kind == 0 ? 1.0 : 0.0;
    for_stats<SM>(S, [&](int s) {
      TMOG_FP_EXACT
      const double p = get(s) / n;
      if (kind == 0) imp -= p * p;
      else if (p > 0) imp -= p * ::log2(p);
    });
    return imp;
  }
  if (kind == 2) {
    const double n = get(0);
    *count = n;
    if (n <= 0) return 0.0;
    const double m = get(1) / n;
    return get(2) / n - m * m;
  }
  *count = get(1);
  return 0.0;
}
// Kinds 0..2: the gain of (left, right) under a parent of impurity pimp and count tcount; false: not a candidate
// (a child below min_instances or empty, or the gain below min_info_gain).
TMOG_HD bool impurity_split_gain(double pimp, double tcount, double lc, double li, double rc, double ri,
                                 double min_inst, double min_gain, double* gain) {
  TMOG_FP_EXACT
  *gain = pimp - (lc / tcount) * li - (rc / tcount) * ri;
  return !(lc < min_inst || rc < min_inst || lc <= 0 || rc <= 0) && !(*gain < min_gain);
}
// Kind 3 (XGBoost): statistics (gradient sum, hessian sum). newton_invalid: a child below min_child_weight. It has
// this polarity because the narrow scans' early exit `if (newton_invalid(..)) return;` compiles as the literal test
// did; `!newton_valid(..)` costs the tuned Newton scan a VGPR and nine SGPR spills.
TMOG_HD double newton_parent(double t0, double t1, double lambda) { TMOG_FP_EXACT return t0 * t0 / (t1 + lambda); }
TMOG_HD double newton_gain(double l0, double l1, double r0, double r1, double lambda, double parent_gain) {
  TMOG_FP_EXACT
  return l0 * l0 / (l1 + lambda) + r0 * r0 / (r1 + lambda) - parent_gain;
}
TMOG_HD bool newton_invalid(double l1, double r1, double mcw) { TMOG_FP_EXACT return l1 < mcw || r1 < mcw; }

// One per node and rank: gain f64 | pos i32 (position in the full growth-order feature list, the tie-break) |
// bin i32 | dl i32 | col i32 (Xb column) | left f32[S], padded to 8 bytes.
enum : int { kFpGain = 0, kFpPos = 8, kFpBin = 12, kFpDl = 16, kFpCol = 20, kFpLeft = 24 };
TMOG_HD size_t fp_rec_bytes(int S) { return (kFpLeft + 4 * (size_t)S + 7) & ~size_t(7); }
// local feature f of this rank's list (multi-bin columns first, then its one-present-bin columns) -> position
TMOG_HD int fp_pos(int f, int fp_mlo, int fp_nml, int fp_obase) {
  return f < fp_nml ? fp_mlo + f : fp_obase + (f - fp_nml);
}
template <class T> TMOG_HD void fp_put(uint8_t* p, T v) {
#ifdef __HIP_DEVICE_COMPILE__
  *reinterpret_cast<T*>(p) = v;
#else
  std::memcpy(p, &v, sizeof(T));
#endif
}
template <class T> TMOG_HD T fp_get(const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
  return *reinterpret_cast<const T*>(p);
#else
  T v;
  std::memcpy(&v, p, sizeof(T));
  return v;
#endif
}
// The fixed fields; c.f is the rank's local feature, col() its Xb column, called only for a found split (on the
// device a load). No split: the "no candidate" gain and position, bin and column -1. Two arms, not selects: the
// narrow scans inline this, and their register figures depend on it.
template <class Col>
TMOG_HD void fp_rec_store(uint8_t* r, bool found, const SplitCand& c, int fp_mlo, int fp_nml, int fp_obase, Col col) {
  if (found) {
    fp_put<double>(r + kFpGain, c.gain);
    fp_put<int32_t>(r + kFpPos, fp_pos(c.f, fp_mlo, fp_nml, fp_obase));
    fp_put<int32_t>(r + kFpBin, c.b);
    fp_put<int32_t>(r + kFpDl, c.dl);
    fp_put<int32_t>(r + kFpCol, col());
  } else {
    fp_put<double>(r + kFpGain, -INFINITY);
    fp_put<int32_t>(r + kFpPos, SplitCand::kNoFeature);
    fp_put<int32_t>(r + kFpBin, -1);
    fp_put<int32_t>(r + kFpDl, 0);
    fp_put<int32_t>(r + kFpCol, -1);
  }
}
TMOG_HD SplitCand fp_rec_load(const uint8_t* r, int32_t* col) {
  *col = fp_get<int32_t>(r + kFpCol);
  return SplitCand{fp_get<double>(r + kFpGain), fp_get<int32_t>(r + kFpPos), fp_get<int32_t>(r + kFpBin),
                   fp_get<int32_t>(r + kFpDl)};
}
// Node j's decision from the R ranks' records (m_stride per rank, rb bytes each): the best under better() with the
// position as the feature -- the candidate a single rank scanning every feature would pick; "no split" if none has one.
TMOG_HD void fp_merge_node(const uint8_t* recv, int R, int64_t m_stride, int64_t j, int64_t rb, int S, int32_t* feat,
                           int32_t* bin, float* gain, uint8_t* dl, float* left) {
  int w = -1;
  int32_t col = -1;
  SplitCand best = SplitCand::none();
  for (int r = 0; r < R; ++r) {
    int32_t c_col;
    const SplitCand c = fp_rec_load(recv + (r * m_stride + j) * rb, &c_col);
    if (!c.found() || !(w < 0 || better(c, best))) continue;
    w = r;
    best = c;
    col = c_col;
  }
  feat[j] = col;
  bin[j] = w < 0 ? -1 : best.b;
  gain[j] = (float)best.gain;
  dl[j] = (uint8_t)best.dl;
  const uint8_t* p = recv + ((w < 0 ? 0 : w) * m_stride + j) * rb + kFpLeft;
  for (int s = 0; s < S; ++s) left[j * S + s] = w < 0 ? 0.f : fp_get<float>(p + 4 * s);
}

// Can a node of `count` entries at `depth` split at all. Newton trees: both children of a split need a hessian
// sum >= min_child_weight, so a node whose hessian (from its parent's split statistics, fp32) is clearly below
// 2 mcw has no valid split -- no histogram, no scan (the 1e-6 margin keeps every node that could split).
TMOG_HD bool can_split(int depth, int max_depth, int64_t count, double min_inst, bool newton, double mcw,
                       double hess) {
  TMOG_FP_EXACT
  if (!(depth < max_depth && count >= 2 && (double)count >= 2 * min_inst - 1e-9)) return false;
  return !(newton && depth > 0 && mcw > 0 && hess < 2.0 * mcw * (1.0 - 1e-6));
}
// Is the split recorded for a node (parameter block prm) taken; each of the three reads only if the ones before hold.
TMOG_HD bool split_accepted(const float* prm, int feat, const float* gain) {
  TMOG_FP_EXACT
  return !(feat < 0 || !(prm[kPrmMaySplit] > 0.5f) || !(*gain > prm[kPrmEps]));
}
// Which child of a sibling pair is derived as parent - sibling (the other one is built from its rows).
TMOG_HD bool left_is_big(int64_t lc, int64_t rc) { return lc >= rc; }
// Siblings of which exactly one needs a histogram: true when the other is built too, so that the needed one can
// be derived by subtraction from the parent's -- that is when the other is the smaller (built) one.
TMOG_HD bool build_sibling(bool can_l, bool need_l, int64_t lc, bool need_r, int64_t rc) {
  return need_l != need_r && lc >= 1 && rc >= 1 && (can_l ? rc <= lc : lc <= rc);
}

// mode 1 (variance statistics): the mean t1 / t0, guarded against a denormal t0 -- also the CPU's class frequency
// t[c] / sum (no device twin), which keeps the guard in one place; mode 2 (gradient, hessian): the Newton step.
TMOG_HD double leaf_value(int mode, double t0, double t1, double lambda, double eta) {
  TMOG_FP_EXACT
  if (mode == 1) return t0 > 0 ? t1 / ::fmax(t0, 1e-300) : 0.0;
  return -t0 / (t1 + lambda) * eta;
}

// Words of a node's live histogram region: with dense >= 0 the first `dense` words (the multi-bin columns, every
// bin) followed by bin 0 (S words of `per`) of each one-present-bin column.
TMOG_HD int64_t live_words(int64_t sz, int64_t dense, int per, int S) {
  return (dense < 0 || sz <= dense) ? sz : dense + (sz - dense) / per * S;
}
// Does a row whose split feature has bin `bin` go left; dl() gives the node's default direction and is called only
// for a missing value (the predict kernels load it then, not at every tree step).
template <class DL> TMOG_HD bool goes_left(uint8_t bin, int sb, DL dl, int missing_bin) {
  return (missing_bin >= 0 && bin == missing_bin) ? dl() : ((int)bin <= sb);
}

}  // namespace tmog
