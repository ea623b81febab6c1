// Device-planned tree growth ("resident" level loop) for one job group on the caller's stream.
//
// The host-planned grower (common/tree_grow.hpp grow_group) reads every level's split decisions back to the
// host, plans the next level there (node bookkeeping, histogram / partition / leaf work items, sibling
// pairs, zero segments) and ships the plan in one staged copy: one blocking round trip per level and
// group, 66-170 us of stream idle per level on the XGBoost headline (profiles/r4_levels_base.txt). Here the
// same plan is computed ON THE DEVICE by one 1024-thread workgroup (level_plan_kernel) between the level
// kernels, and every level kernel is launched with a host upper bound of its grid and reads the real item
// count from device memory (the `dcount` arguments of tree_*_kernels.hip): the host enqueues a whole tree -- every
// level, the leaf collection and the tree finalisation (leaf values, gamma pruning; tree_finalize_kernel) --
// without a single synchronisation, and boosting (models/trees.py) enqueues round after round. The host
// reads the created-node records once per fit.
//
// The device plan reproduces grow_group's decisions exactly: both evaluate common/tree_rules.hpp (can / need rules,
// Newton hessian gate) and common/tree_plan.hpp (subtraction pairing, work counts, items, zero segments, parameter
// slots) over the feature groups of group_layout, so the trees are bit-identical to the host-planned grower
// (tests/test_tree_resident_gpu.py; the layout alone: tests/test_level_items_cpu.py). Partition order inside a
// child is not stable on either path.
//
// Reference behaviour: XGBoost4J's hist updater as wrapped by OpXGBoostClassifier.scala:47-403.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "common/tree_grow.hpp"
#include "hip/dev_alloc.hpp"
#include "hip/tmog_hip_abi.h"

// plan / finalisation arithmetic with the host twins' IEEE operation sequence (no FMA contraction)
#pragma clang fp contract(off)

namespace {

using tmog::HistItemH;
using tmog::LeafItemH;
using tmog::PartItemH;

// device counters of the current level (int32 each)
enum : int {
  C_N = 0,     // nodes of the current level
  C_M,         // histogram (scanned) nodes
  C_NP,        // sibling pairs
  C_NH,        // histogram items
  C_NC,        // partition items
  C_NZ,        // zero segments (C_NZ, C_NZD adjacent: zero_segments_kernel reads both)
  C_NZD,       // ... of which whole-node segments (listed first)
  C_NL,        // leaf items
  C_NCREATED,  // created nodes of the tree
  C_ERR,       // bit 0: partition cursor mismatch, bit 1: capacity overflow
  C_COUNT = 16
};

constexpr int kRecFixed = TMOG_REC_FIXED;   // record words before the S totals: tree feat bin dl gain left right

struct PlanArgs {
  int d, T, S, chunk_rows, n_groups, n_sc, newton, subtract, pair_fuse, F_use, has_missing;
  int64_t hsz, live_dense;
  const tmog::FeatGroup* groups;   // GroupLayout.full_groups as they are
  const int32_t* j_depth;
  const int32_t* j_model;
  const int64_t* j_count;
  const double* j_inst;
  const double* j_gain;
  const double* j_mcw;
  const double* j_lam;
  const double* j_eps;
  int32_t* lv_tree[2];
  int32_t* lv_gid[2];
  int64_t* lv_begin[2];
  int64_t* lv_count[2];
  int32_t* hn[2];              // histogram node j -> level node i
  int32_t* nmd[2];
  int64_t* nho[2];
  float* par[2];
  int64_t* nb[2];
  int64_t* nc[2];
  int32_t* nfo;
  int32_t* nnf;
  int32_t* sj;
  int32_t* bj;
  int64_t* poff;
  int64_t* zoff;
  int64_t* zsize;
  int64_t* ppo;                // parent histogram offset of the previous level's q-th split
  HistItemH* hitems;
  PartItemH* citems;
  LeafItemH* litems;
  const int32_t* r_feat;
  const int32_t* r_bin;
  const float* r_gain;
  const float* r_left;
  const float* r_tot;
  const uint8_t* r_dl;
  const int64_t* r_cur;
  int64_t* rec;
  int W;
  int32_t* level_off;
  int* cnt;
  int64_t* leaf_pos;
  int64_t* sa;
  int64_t* sb;
  int64_t* sc;
  int64_t* sd;
  int64_t* se;
  int64_t* sf;
  int64_t* sg;
  int32_t* flag;
  int32_t* loc;
  int64_t cap_nl, cap_m, cap_nodes, cap_h, cap_c, cap_l;
  int profile;                 // TMOG_PLAN_PROFILE: per-phase wall-clock ticks into g_plan_prof
  int64_t lds_cap;             // > 0: scratch arrays in dynamic LDS with this many entries each
};

// TMOG_PLAN_PROFILE diagnostics: wall-clock ticks (100 MHz) spent in each phase of level_plan_kernel, summed
// over calls (entry 31: calls); read with tmog_hip_plan_profile.
__device__ unsigned long long g_plan_prof[32];

__device__ __forceinline__ int64_t dbits(double v) { return __double_as_longlong(v); }
__device__ __forceinline__ double bitsd(int64_t v) { return __longlong_as_double(v); }

// Exclusive prefix sums of K arrays v[k][0, n) in place at once; every thread of the block calls it and gets the
// totals. Each thread sums a contiguous run of ceil(n / 1024) entries, the runs are scanned inside each wave on
// the lane network (6 shuffle steps, no barrier), the 16 wave totals go through LDS: two barriers per call
// whatever K, instead of 2 log2(1024) per array.
__device__ __forceinline__ int64_t wave_incl_scan(int64_t x, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  return x;
}

template <int K>
__device__ void block_scan_multi(int64_t* const (&v)[K], int64_t n, int64_t (&total)[K], int64_t* sh) {
  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
  const int64_t per = (n + nt - 1) / nt;
  const int64_t lo = min(n, (int64_t)t * per), hi = min(n, lo + per);
  int64_t s[K], incl[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    s[k] = 0;
    for (int64_t i = lo; i < hi; ++i) s[k] += v[k][i];
    incl[k] = wave_incl_scan(s[k], lane);
    if (lane == 63) sh[k * 16 + wave] = incl[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int64_t before = 0, all = 0;
    for (int w = 0; w < nw; ++w) {
      const int64_t x = sh[k * 16 + w];
      before += w < wave ? x : 0;
      all += x;
    }
    total[k] = all;
    int64_t run = before + incl[k] - s[k];
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t x = v[k][i];
      v[k][i] = run;
      run += x;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ int64_t block_scan(int64_t* v, int64_t n, int64_t* sh) {
  int64_t* const a[1] = {v};
  int64_t tot[1];
  block_scan_multi<1>(a, n, tot, sh);
  return tot[0];
}

// last i in [0, n) with pre[i] <= k (pre: exclusive prefix sums, k < total): the owner of item k
__device__ __forceinline__ int64_t owner(const int64_t* pre, int64_t n, int64_t k) {
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= k) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void init_node(int64_t* r, int64_t tree, int S) {
  r[0] = tree;
  r[1] = -1;
  r[2] = -1;
  r[3] = 0;
  r[4] = dbits(0.0);
  r[5] = -1;
  r[6] = -1;
  for (int s = 0; s < S; ++s) r[kRecFixed + s] = dbits(0.0);
}

// Leaf items of the nodes i in [0, n) whose sa-flag is 0 (sa == nullptr: all nodes), reading buffer `buf`.
// Appends to litems at C_NL and advances the leaf cursor (host twin: the collect lambda of grow_group).
// The planner's per-node scratch arrays (global memory, or dynamic LDS when the level capacity fits).
struct PlanScratch {
  int64_t *sa, *sb, *sc, *sd, *se, *sf, *sg;
  int32_t* flag;
};

__device__ void emit_leaves(const PlanArgs& A, const PlanScratch& Z, int lvl, int n, const int32_t* split, int buf,
                            int64_t* sh) {
  const int t = threadIdx.x, nt = blockDim.x;
  const int64_t* cnt_ = A.lv_count[lvl];
  for (int i = t; i < n; i += nt) {
    const bool leaf = split == nullptr || split[i] == 0;
    const int64_t c = cnt_[i];
    Z.sd[i] = leaf && c > 0 ? c : 0;
    Z.se[i] = leaf ? tmog::leaf_items(c, A.chunk_rows) : 0;
  }
  __syncthreads();
  const int64_t lbase = *A.leaf_pos;
  const int64_t nl0 = A.cnt[C_NL];
  __syncthreads();
  int64_t* const arr[2] = {Z.sd, Z.se};
  int64_t tots[2];
  block_scan_multi<2>(arr, n, tots, sh);
  const int64_t tot_rows = tots[0], tot_items = tots[1];
  const int64_t n_emit = min(tot_items, A.cap_l - nl0);
  for (int64_t k = t; k < n_emit; k += nt) {
    const int64_t i = owner(Z.se, n, k);
    A.litems[nl0 + k] = tmog::leaf_item_at(k - Z.se[i], A.lv_begin[lvl][i], cnt_[i], A.chunk_rows, lbase + Z.sd[i],
                                           A.lv_gid[lvl][i], buf);
  }
  __syncthreads();
  if (t == 0) {
    *A.leaf_pos = lbase + tot_rows;
    A.cnt[C_NL] = (int)(nl0 + n_emit);
    if (n_emit < tot_items) A.cnt[C_ERR] |= 2;
  }
  __syncthreads();
}

// One level of planning. d > 0 first turns level d - 1's device decisions (split_find + partition) into
// the tree records, the leaf items of its non-splitting nodes and the children (level d); then level d's
// work lists are built. Host twin: common/tree_grow.hpp grow_group (GPU backend, no feature subsets).
constexpr int kPlanScratch = 7;     // int64 per-node scratch arrays of the planner (sa .. sg) + one int32 (flag)

__global__ void __launch_bounds__(1024) level_plan_kernel(PlanArgs A) {
  __shared__ int64_t sh[1024];
  // the per-node scratch arrays live in LDS when the level capacity fits (A.lds_cap > 0): every scan, owner
  // search and flag read of the plan is then an LDS access instead of an L2 round trip
  extern __shared__ int64_t dyn_scratch[];
  // the plan is the serial link between two levels of this tree while its CU usually also runs other boosting
  // parts' histogram waves: issue priority over them
  __builtin_amdgcn_s_setprio(3);
  PlanScratch Z{A.sa, A.sb, A.sc, A.sd, A.se, A.sf, A.sg, A.flag};
  if (A.lds_cap > 0) {
    int64_t* base = dyn_scratch;
    Z = PlanScratch{base, base + A.lds_cap, base + 2 * A.lds_cap, base + 3 * A.lds_cap, base + 4 * A.lds_cap,
                    base + 5 * A.lds_cap, base + 6 * A.lds_cap, reinterpret_cast<int32_t*>(base + 7 * A.lds_cap)};
  }
  __shared__ int s_n_prev, s_m_prev, s_created;
  const int t = threadIdx.x, nt = blockDim.x;
  const int d = A.d, S = A.S, T = A.T;
  auto R = [&](int64_t g) { return A.rec + (g + 1) * (int64_t)A.W; };
  uint64_t t_prev = 0;
  if (A.profile && t == 0) {
    t_prev = wall_clock64();
    atomicAdd(&g_plan_prof[31], 1ull);
  }
  auto mark = [&](int k) {
    if (A.profile && t == 0) {
      const uint64_t now = wall_clock64();
      atomicAdd(&g_plan_prof[k], (unsigned long long)(now - t_prev));
      t_prev = now;
    }
  };
  if (t == 0) {
    s_n_prev = d > 0 ? A.cnt[C_N] : 0;
    s_m_prev = d > 0 ? A.cnt[C_M] : 0;
    s_created = d > 0 ? A.cnt[C_NCREATED] : 0;
  }
  __syncthreads();
  if (t == 0) {
    A.cnt[C_NL] = 0;
    if (d == 0) {
      A.cnt[C_ERR] = 0;
      *A.leaf_pos = 0;
    }
  }
  __syncthreads();
  int n = 0;
  const int C = d & 1;
  if (d == 0) {
    if (t == 0) {
      int64_t b = 0;
      for (int j = 0; j < T; ++j) {
        A.lv_tree[0][j] = j;
        A.lv_gid[0][j] = j;
        A.lv_begin[0][j] = b;
        A.lv_count[0][j] = A.j_count[j];
        b += A.j_count[j];
      }
      A.cnt[C_NCREATED] = T;
      A.level_off[0] = 0;
    }
    for (int j = t; j < T; j += nt) init_node(R(j), j, S);
    n = T;
    __syncthreads();
    mark(0);
  } else {
    const int P = (d - 1) & 1;
    const int n_prev = s_n_prev;
    if (t == 0) A.level_off[d] = s_created;
    if (n_prev == 0) {
      if (t == 0) {
        for (int k = C_N; k <= C_NZD; ++k) A.cnt[k] = 0;
      }
      return;
    }
    // (a) per node of level d - 1 (loc[i] = its histogram node j, or -1): node totals, split flag, leaf work
    const int64_t* pcnt = A.lv_count[P];
    for (int i = t; i < n_prev; i += nt) {
      const int j = A.loc[i];
      bool split = false;
      if (j >= 0) {
        int64_t* r = R(A.lv_gid[P][i]);
        for (int s = 0; s < S; ++s) r[kRecFixed + s] = dbits((double)A.r_tot[(int64_t)j * S + s]);
        const float* Pp = A.par[P] + (int64_t)j * tmog::kPrmStride;
        split = tmog::split_accepted(Pp, A.r_feat[j], A.r_gain + j);
      }
      const int64_t c = pcnt[i];
      const bool leaf = !split && c > 0;
      Z.sd[i] = leaf ? c : 0;
      Z.se[i] = split ? 0 : tmog::leaf_items(c, A.chunk_rows);
      Z.sf[i] = split ? 1 : 0;
      Z.flag[i] = split ? 1 : 0;
    }
    __syncthreads();
    mark(1);
    const int64_t lbase = *A.leaf_pos;
    const int64_t nl0 = A.cnt[C_NL];
    int64_t* const arr3[3] = {Z.sd, Z.se, Z.sf};
    int64_t tot3[3];
    block_scan_multi<3>(arr3, n_prev, tot3, sh);
    const int64_t tot_rows = tot3[0], tot_items = tot3[1], ns = tot3[2];
    mark(2);
    const int base = s_created;
    if (2 * ns > A.cap_nl || base + 2 * ns > A.cap_nodes) {   // (cannot happen: caps bound every level)
      if (t == 0) {
        A.cnt[C_ERR] |= 2;
        A.cnt[C_N] = 0;
        for (int k = C_M; k <= C_NZD; ++k) A.cnt[k] = 0;
      }
      return;
    }
    // (b) leaf items of the nodes that do not split (read from the buffer level d - 1 read)
    const int64_t n_emit = min(tot_items, A.cap_l - nl0);
    for (int64_t k = t; k < n_emit; k += nt) {
      const int64_t i = owner(Z.se, n_prev, k);
      A.litems[nl0 + k] = tmog::leaf_item_at(k - Z.se[i], A.lv_begin[P][i], pcnt[i], A.chunk_rows, lbase + Z.sd[i],
                                             A.lv_gid[P][i], P);
    }
    // (c) splits -> records + children (level d), in split order
    for (int i = t; i < n_prev; i += nt) {
      if (!Z.flag[i]) continue;
      const int j = A.loc[i];
      const int64_t q = Z.sf[i];
      int64_t* r = R(A.lv_gid[P][i]);
      r[1] = A.r_feat[j];
      r[2] = A.r_bin[j];
      r[3] = A.r_dl[j];
      r[4] = dbits((double)A.r_gain[j]);
      const int64_t ncnt = pcnt[i];
      const int64_t nl = A.r_cur[2 * j];
      if (nl < 0 || nl + A.r_cur[2 * j + 1] != ncnt) A.cnt[C_ERR] |= 1;
      const int64_t gl = base + 2 * q, gr = gl + 1;
      r[5] = gl;
      r[6] = gr;
      const int tree = A.lv_tree[P][i];
      int64_t* rl = R(gl);
      int64_t* rr = R(gr);
      init_node(rl, tree, S);
      init_node(rr, tree, S);
      for (int s = 0; s < S; ++s) {
        const double lt = (double)A.r_left[(int64_t)j * S + s];
        const double tt = (double)A.r_tot[(int64_t)j * S + s];
        rl[kRecFixed + s] = dbits(lt);
        rr[kRecFixed + s] = dbits(tt - lt);
      }
      const int64_t b0 = A.lv_begin[P][i];
      A.lv_tree[C][2 * q] = tree;
      A.lv_gid[C][2 * q] = (int32_t)gl;
      A.lv_begin[C][2 * q] = b0;
      A.lv_count[C][2 * q] = nl;
      A.lv_tree[C][2 * q + 1] = tree;
      A.lv_gid[C][2 * q + 1] = (int32_t)gr;
      A.lv_begin[C][2 * q + 1] = b0 + nl;
      A.lv_count[C][2 * q + 1] = ncnt - nl;
      A.ppo[q] = A.nho[P][j];
    }
    n = (int)(2 * ns);
    if (t == 0) {
      *A.leaf_pos = lbase + tot_rows;
      A.cnt[C_NL] = (int)(nl0 + n_emit);
      if (n_emit < tot_items) A.cnt[C_ERR] |= 2;
      A.cnt[C_NCREATED] = base + n;
    }
    __syncthreads();
    mark(3);
  }
  if (n == 0) {
    if (t == 0) {
      A.cnt[C_N] = 0;
      for (int k = C_M; k <= C_NZD; ++k) A.cnt[k] = 0;
    }
    return;
  }
  // ---- plan level d, one pass over sibling pairs (level 0: over the roots). Per node i: the kNode* flag bits
  // and work counts of common/tree_plan.hpp, the counts for one multi-scan: sa need, sb wide-load hist items,
  // sc other hist items, sd partition items, se whole-node zero segments, sf CSR-region zero segments, sg pairs (at
  // the left node)
  const int32_t* ltree = A.lv_tree[C];
  const int64_t* lcnt = A.lv_count[C];
  auto can_split = [&](int i) {
    const int jt = ltree[i];
    const bool gate = A.newton && d > 0;       // the hessian: the node's second total, recorded by its parent's split
    return tmog::can_split(d, A.j_depth[jt], lcnt[i], A.j_inst[jt], gate, A.j_mcw[jt],
                           gate ? bitsd(R(A.lv_gid[C][i])[kRecFixed + 1]) : 0.0);
  };
  auto counts = [&](int i, int fl) {
    const tmog::NodeWork w = tmog::node_work(fl, lcnt[i], A.chunk_rows, A.groups, A.n_groups, A.n_sc, A.live_dense,
                                             A.hsz);
    Z.flag[i] = fl;
    Z.sa[i] = (fl & tmog::kNodeNeed) ? 1 : 0;
    Z.sb[i] = w.n_wide;
    Z.sc[i] = w.n_other;
    Z.sd[i] = w.n_part;
    Z.se[i] = w.zero == tmog::kZeroNode ? 1 : 0;
    Z.sf[i] = w.zero == tmog::kZeroCsr ? 1 : 0;
    Z.sg[i] = (fl & tmog::kNodePairLeft) ? 1 : 0;
  };
  if (d == 0) {
    for (int i = t; i < n; i += nt) counts(i, tmog::root_flags(can_split(i)));
  } else {
    for (int q = t; 2 * q + 1 < n; q += nt) {
      const int li = 2 * q, ri = li + 1;
      int fl, fr;
      tmog::sibling_flags(can_split(li), can_split(ri), lcnt[li], lcnt[ri], A.subtract != 0, &fl, &fr);
      counts(li, fl);
      counts(ri, fr);
    }
  }
  __syncthreads();
  mark(4);
  int64_t* const arr7[7] = {Z.sa, Z.sb, Z.sc, Z.sd, Z.se, Z.sf, Z.sg};
  int64_t tot7[7];
  block_scan_multi<7>(arr7, n, tot7, sh);
  const int m = (int)tot7[0];
  const int64_t n_wide = tot7[1], n_other = tot7[2], n_part = tot7[3], n_zw = tot7[4], n_zc = tot7[5];
  const int n_pairs = (int)tot7[6];
  mark(5);
  if (m > A.cap_m) {                       // (cannot happen: caps bound every level)
    if (t == 0) {
      A.cnt[C_ERR] |= 2;
      A.cnt[C_N] = 0;
      for (int k = C_M; k <= C_NZD; ++k) A.cnt[k] = 0;
    }
    return;
  }
  if (m == 0) {                            // nothing to scan: every node of level d is a leaf
    for (int i = t; i < n; i += nt) A.loc[i] = -1;
    emit_leaves(A, Z, C, n, nullptr, C, sh);
    if (t == 0) {
      A.cnt[C_N] = 0;
      for (int k = C_M; k <= C_NZD; ++k) A.cnt[k] = 0;
    }
    return;
  }
  // ---- emission: per-node tables (histogram node j = need prefix, in node order), pairs, zero segments
  for (int i = t; i < n; i += nt) {
    const int fl = Z.flag[i];
    if (!(fl & tmog::kNodeNeed)) {
      A.loc[i] = -1;
      continue;
    }
    const int j = (int)Z.sa[i];
    const int jt = ltree[i];
    A.hn[C][j] = i;
    A.loc[i] = j;
    A.nmd[C][j] = A.j_model[jt];
    A.nho[C][j] = (int64_t)j * A.hsz;
    A.nb[C][j] = A.lv_begin[C][i];
    A.nc[C][j] = lcnt[i];
    A.nfo[j] = 0;
    A.nnf[j] = A.F_use;
    // pair_fuse: the pair scan derives / scans both siblings
    const bool paired = d > 0 && (((i & 1) == 0 && (fl & tmog::kNodePairLeft)) ||
                                  ((i & 1) == 1 && (Z.flag[i - 1] & tmog::kNodePairLeft)));
    tmog::fill_node_params(A.par[C] + (int64_t)j * tmog::kPrmStride, A.j_inst[jt], A.j_gain[jt], A.j_mcw[jt],
                           A.j_lam[jt], paired, A.has_missing != 0, A.j_eps[jt], (fl & tmog::kNodeCan) != 0);
    if (fl & tmog::kNodePairLeft) {        // left node of a pair: (small, big) histogram nodes, parent offset
      const int jr = (int)Z.sa[i + 1];
      const bool left_big = fl & tmog::kNodeDerived;
      const int64_t k = Z.sg[i];
      A.sj[k] = left_big ? jr : j;
      A.bj[k] = left_big ? j : jr;
      A.poff[k] = A.ppo[i >> 1];
    }
    const bool zw = (i + 1 < n ? Z.se[i + 1] : n_zw) != Z.se[i];
    const bool zc = (i + 1 < n ? Z.sf[i + 1] : n_zc) != Z.sf[i];
    const int64_t hoff = (int64_t)j * A.hsz;
    if (zw) tmog::zero_segment(tmog::kZeroNode, hoff, A.hsz, A.live_dense, &A.zoff[Z.se[i]], &A.zsize[Z.se[i]]);
    if (zc)
      tmog::zero_segment(tmog::kZeroCsr, hoff, A.hsz, A.live_dense, &A.zoff[n_zw + Z.sf[i]], &A.zsize[n_zw + Z.sf[i]]);
  }
  mark(6);
  const int64_t n_hist = n_wide + n_other;
  const int64_t h_emit = min(n_hist, A.cap_h), c_emit = min(n_part, A.cap_c);
  // histogram items, wide-load items first (a kernel of their own), then the others
  for (int64_t k = t; k < h_emit; k += nt) {
    const bool wsec = k < n_wide;
    const int64_t* pre = wsec ? Z.sb : Z.sc;
    const int64_t kk = wsec ? k : k - n_wide;
    const int64_t i = owner(pre, n, kk);
    A.hitems[k] = tmog::hist_item_at(wsec, (int32_t)Z.sa[i], kk - pre[i], A.lv_begin[C][i], lcnt[i], A.chunk_rows,
                                     A.groups, A.n_groups, A.n_sc, A.live_dense);
  }
  // partition items of every scanned node (kPartRows-row slices)
  for (int64_t k = t; k < c_emit; k += nt) {
    const int64_t i = owner(Z.sd, n, k);
    A.citems[k] = tmog::part_item_at((int32_t)Z.sa[i], k - Z.sd[i], A.lv_begin[C][i], lcnt[i]);
  }
  if (t == 0) {
    A.cnt[C_N] = n;
    A.cnt[C_M] = m;
    A.cnt[C_NP] = n_pairs;
    A.cnt[C_NH] = (int)h_emit;
    A.cnt[C_NC] = (int)c_emit;
    A.cnt[C_NZ] = (int)(n_zw + n_zc);
    A.cnt[C_NZD] = (int)n_zw;
    if (h_emit < n_hist || c_emit < n_part) A.cnt[C_ERR] |= 2;
  }
  mark(7);
}

struct FinArgs {
  int T, S, mode, kind, n_levels;
  int prune;                   // some job has gamma > 0 (Newton): pruning can happen
  int64_t* rec;
  int W;
  const int32_t* level_off;
  const int* cnt;
  const int64_t* leaf_pos;
  const double* j_lam;
  const double* j_eta;
  const double* j_gamma;
  float* gid_value;
  int64_t* gid_tree;
  int64_t* left_w;
  int64_t* right_w;
  int64_t* parent;
  int32_t* reach;
  double* value;
};

// Device twin of tmog_tree_finalize_cpu's values / gamma pruning / gid values (ops/csrc/host/tree_cpu.cpp):
// the leaf output of every created node id for the boosting epilogue, a pruned node's descendants taking
// their kept ancestor's value. The host rebuilds the Forest from the same records with tree_cpu.cpp.
// Pruning bottom-up level by level is the sequential reverse-id loop (children have higher ids than parents).
__global__ void __launch_bounds__(1024) tree_finalize_kernel(FinArgs A) {
  __builtin_amdgcn_s_setprio(3);            // serial link between two boosting rounds (see level_plan_kernel)
  const int t = threadIdx.x, nt = blockDim.x;
  const int64_t n = A.cnt[C_NCREATED];
  auto R = [&](int64_t g) { return A.rec + (g + 1) * (int64_t)A.W; };
  if (!(A.kind == 3 && A.prune)) {
    // nothing can be pruned (no gamma > 0: a recorded split's gain exceeds split_eps > 0), so every created
    // node is reachable and keeps its own value: one pass, no level loops
    for (int64_t i = t; i < n; i += nt) {
      const int64_t* r = R(i);
      const int64_t jt = r[0];
      const double t0 = bitsd(r[kRecFixed]);
      const double t1 = A.S > 1 ? bitsd(r[kRecFixed + 1]) : 0.0;
      A.gid_value[i] = (float)tmog::leaf_value(A.mode, t0, t1, A.j_lam[jt], A.j_eta[jt]);
      A.gid_tree[i] = jt;
    }
    if (t == 0) {
      A.rec[0] = n;
      A.rec[1] = *A.leaf_pos;
      A.rec[2] = A.cnt[C_ERR];
    }
    return;
  }
  for (int64_t i = t; i < n; i += nt) {
    const int64_t* r = R(i);
    const int64_t jt = r[0];
    const double t0 = bitsd(r[kRecFixed]);
    const double t1 = A.S > 1 ? bitsd(r[kRecFixed + 1]) : 0.0;
    A.value[i] = tmog::leaf_value(A.mode, t0, t1, A.j_lam[jt], A.j_eta[jt]);
    A.left_w[i] = r[5];
    A.right_w[i] = r[6];
    A.parent[i] = -1;
    A.reach[i] = i < A.T ? 1 : 0;
  }
  __syncthreads();
  for (int64_t i = t; i < n; i += nt) {
    const int64_t* r = R(i);
    if (r[5] >= 0) {
      A.parent[r[5]] = i;
      A.parent[r[6]] = i;
    }
  }
  __syncthreads();
  auto lvl_lo = [&](int L) { return (int64_t)A.level_off[L]; };
  auto lvl_hi = [&](int L) { return L + 1 < A.n_levels ? (int64_t)A.level_off[L + 1] : n; };
  if (A.kind == 3) {
    for (int L = A.n_levels - 1; L >= 0; --L) {
      for (int64_t i = lvl_lo(L) + t; i < lvl_hi(L); i += nt) {
        const int64_t l = A.left_w[i];
        if (l < 0) continue;
        const int64_t r = A.right_w[i];
        const int64_t* rr = R(i);
        if (A.left_w[l] < 0 && A.left_w[r] < 0 && bitsd(rr[4]) < A.j_gamma[rr[0]]) {
          A.left_w[i] = -1;
          A.right_w[i] = -1;
        }
      }
      __syncthreads();
    }
  }
  for (int L = 0; L < A.n_levels; ++L) {
    for (int64_t i = lvl_lo(L) + t; i < lvl_hi(L); i += nt)
      if (A.reach[i] && A.left_w[i] >= 0) {
        A.reach[A.left_w[i]] = 1;
        A.reach[A.right_w[i]] = 1;
      }
    __syncthreads();
  }
  for (int L = 0; L < A.n_levels; ++L) {
    for (int64_t i = lvl_lo(L) + t; i < lvl_hi(L); i += nt) {
      const int64_t p = A.parent[i];
      A.gid_value[i] = (A.reach[i] || p < 0) ? (float)A.value[i] : A.gid_value[p];
      A.gid_tree[i] = R(i)[0];
    }
    __syncthreads();
  }
  if (t == 0) {
    A.rec[0] = n;
    A.rec[1] = *A.leaf_pos;
    A.rec[2] = A.cnt[C_ERR];
  }
}

using tmog::hchk;
using tmog::kchk;

// Per-slot device resources of the resident grower (hip/dev_alloc.hpp; stream-ordered allocations on the
// caller's stream, which every use of the slot is ordered on).
struct ResSlot {
  tmog::DevBuf arena, hist[2], cand;
  tmog::Tickets done;
  // Feature-parallel split records, this rank's and the all-gathered ones. Stream-ordered blocks here, plain
  // hipMalloc ones in the host-planned loop (tree_grow_hip.hip GpuSlot): the two loops differ, and neither has
  // run at world > 1 on hardware.
  tmog::DevBuf fp_send, fp_recv;
  tmog::StagedCopy consts;     // the per-call constants
  std::vector<uint8_t> last;   // constants last shipped (skipped when unchanged)
  int device = -1;
};

inline size_t slack(size_t bytes) { return bytes + bytes / 4 + 4096; }   // this loop's growth policy

std::vector<ResSlot>& res_slots() {
  static std::vector<ResSlot> s(32);
  return s;
}

thread_local std::string g_err;

struct Carve {
  uint8_t* base;
  size_t off = 0;
  template <class T>
  T* take(int64_t n) {
    off = (off + 255) & ~size_t(255);
    T* p = reinterpret_cast<T*>(base + off);
    off += sizeof(T) * (size_t)std::max<int64_t>(n, 1);
    return p;
  }
};

struct Caps {
  int D = 0;
  std::vector<int64_t> nmax;   // nodes per level bound, d = 0..D + 1 (level D + 1 is empty)
  int64_t cap_nl = 0, cap_m = 0, cap_nodes = 0, cap_h = 0, cap_c = 0, cap_l = 0;
  int64_t total = 0;           // row entries of the group
};

Caps caps_of(const tmog::GrowArgs& a, const tmog::GroupLayout& L, int n_sc) {
  Caps c;
  const int T = a.T;
  int64_t total = 0;
  for (int j = 0; j < T; ++j) {
    total += a.job_count[j];
    c.D = std::max(c.D, (int)a.job_depth[j]);
  }
  c.nmax.assign(c.D + 2, 0);
  for (int d = 0; d <= c.D; ++d) {
    int64_t s = 0;
    for (int j = 0; j < T; ++j)
      if (d <= a.job_depth[j]) s += std::min(d >= 40 ? a.job_count[j] : ((int64_t)1 << d), std::max<int64_t>(a.job_count[j], 1));
    c.nmax[d] = std::max<int64_t>(1, std::min<int64_t>(s, std::max<int64_t>(total, T)));
    c.cap_nl = std::max(c.cap_nl, c.nmax[d]);
    if (d < c.D || d == 0) c.cap_m = std::max(c.cap_m, c.nmax[d]);   // levels that build histograms
    c.cap_nodes += c.nmax[d];
  }
  c.cap_m = std::max<int64_t>(c.cap_m, 1);
  c.total = total;
  c.cap_h = tmog::hist_items_bound(L.full_groups.data(), (int)L.full_groups.size(), a.chunk_rows, n_sc, total, c.cap_m);
  c.cap_c = tmog::part_items_bound(total, c.cap_m);
  c.cap_l = 2 * tmog::leaf_items_bound(a.chunk_rows, total, c.cap_nl);   // a plan collects two levels' leaves
  return c;
}

// Configurations the device plan covers (everything else stays on the host-planned grower): one job group,
// no per-node feature subsets, subtraction + fused pair scan, narrow split scan with the fused reduction,
// statistics in one histogram chunk, leaves collected, Newton (MODE 2) or variance (MODE 1) values.
// Feature-parallel growth is covered: the level's split records are all-gathered and merged on the stream
// (RCCL, or the local answer of a projected rank group) between split-find and partition, so a spread job's
// levels need no host round trip either. Returns an empty string when supported.
std::string unsupported(const tmog::GrowArgs& a) {
  if (a.n_groups != 1) return "more than one job group";
  if (a.fp_world > 0 && a.fp_comm == nullptr) return "feature-parallel without a communicator array";
  if (!a.collect_leaves) return "leaves not collected";
  if (!a.subtract) return "no subtraction";
  if (a.mode == 0) return "class-count histograms";
  if (a.S > 16 || a.B > 64) return "wide statistics";
  for (int j = 0; j < a.T; ++j) {
    const int k = a.job_fsub[j];
    if (k > 0 && k < a.F) return "per-node feature subsets";
  }
  if (!tmog::pair_scan_enabled()) return "pair scan disabled";
  if (!tmog::fused_reduce_enabled()) return "fused reduction disabled";
  if (tmog::hist_wide_split()) return "split wide-load launches";
  if (tmog_hip_hist_stat_chunk(a.B, a.S) < a.S) return "chunked statistics";
  return "";
}

constexpr int kNsc = 1;   // statistic chunks per histogram item (unsupported(): one chunk holds all S)

// ---- the steps of one call (tmog_hip_grow_resident), in the order they run

// Everything carved out of the slot's arena: the planner's arrays (set in `plan`, whose other members
// plan_args() fills), split_find's outputs (which the planner reads) and the finalisation's scratch (in `fin`).
struct Arena {
  PlanArgs plan{};
  FinArgs fin{};
  int32_t *r_feat, *r_bin;
  float *r_gain, *r_left, *r_tot;
  uint8_t* r_dl;
  int64_t* r_cur;
};

// Called with a null base for the arena's size (cv.off afterwards), then with the real base.
Arena lay_out(Carve& cv, const Caps& cp, int S) {
  Arena A;
  PlanArgs& P = A.plan;
  for (int k = 0; k < 2; ++k) {
    P.lv_tree[k] = cv.take<int32_t>(cp.cap_nl);
    P.lv_gid[k] = cv.take<int32_t>(cp.cap_nl);
    P.lv_begin[k] = cv.take<int64_t>(cp.cap_nl);
    P.lv_count[k] = cv.take<int64_t>(cp.cap_nl);
    P.hn[k] = cv.take<int32_t>(cp.cap_m);
    P.nmd[k] = cv.take<int32_t>(cp.cap_m);
    P.nho[k] = cv.take<int64_t>(cp.cap_m);
    P.par[k] = cv.take<float>(8 * cp.cap_m);
    P.nb[k] = cv.take<int64_t>(cp.cap_m);
    P.nc[k] = cv.take<int64_t>(cp.cap_m);
  }
  P.nfo = cv.take<int32_t>(cp.cap_m);
  P.nnf = cv.take<int32_t>(cp.cap_m);
  P.sj = cv.take<int32_t>(cp.cap_m);
  P.bj = cv.take<int32_t>(cp.cap_m);
  P.poff = cv.take<int64_t>(cp.cap_m);
  P.zoff = cv.take<int64_t>(cp.cap_m);
  P.zsize = cv.take<int64_t>(cp.cap_m);
  P.ppo = cv.take<int64_t>(cp.cap_nl);
  P.hitems = cv.take<HistItemH>(cp.cap_h);
  P.citems = cv.take<PartItemH>(cp.cap_c);
  P.litems = cv.take<LeafItemH>(cp.cap_l);
  P.sa = cv.take<int64_t>(cp.cap_nl);
  P.sb = cv.take<int64_t>(cp.cap_nl);
  P.sc = cv.take<int64_t>(cp.cap_nl);
  P.sd = cv.take<int64_t>(cp.cap_nl);
  P.se = cv.take<int64_t>(cp.cap_nl);
  P.sf = cv.take<int64_t>(cp.cap_nl);
  P.sg = cv.take<int64_t>(cp.cap_nl);
  P.flag = cv.take<int32_t>(cp.cap_nl);
  P.loc = cv.take<int32_t>(cp.cap_nl);
  P.cnt = cv.take<int>(C_COUNT);
  P.leaf_pos = cv.take<int64_t>(1);
  P.level_off = cv.take<int32_t>(cp.D + 2);
  P.r_feat = A.r_feat = cv.take<int32_t>(cp.cap_m);
  P.r_bin = A.r_bin = cv.take<int32_t>(cp.cap_m);
  P.r_gain = A.r_gain = cv.take<float>(cp.cap_m);
  P.r_left = A.r_left = cv.take<float>((int64_t)S * cp.cap_m);
  P.r_tot = A.r_tot = cv.take<float>((int64_t)S * cp.cap_m);
  P.r_dl = A.r_dl = cv.take<uint8_t>(cp.cap_m);
  P.r_cur = A.r_cur = cv.take<int64_t>(2 * cp.cap_m);
  A.fin.left_w = cv.take<int64_t>(cp.cap_nodes);
  A.fin.right_w = cv.take<int64_t>(cp.cap_nodes);
  A.fin.parent = cv.take<int64_t>(cp.cap_nodes);
  A.fin.reach = cv.take<int32_t>(cp.cap_nodes);
  A.fin.value = cv.take<double>(cp.cap_nodes);
  return A;
}

// The per-call constants on the device: the block and the byte offset of each array in it.
struct Consts {
  const uint8_t* dev;
  size_t groups, flist, depth, model, count, inst, gain, mcw, lam, eps, eta, gamma;
  template <class T>
  const T* at(size_t off) const { return reinterpret_cast<const T*>(dev + off); }
};

// What the steps of one call share.
struct Ctx {
  const tmog::GrowArgs& a;
  const ResidentIO& io;
  ResSlot& sl;
  hipStream_t st;
  tmog::GroupLayout L;
  Caps cp;
  int64_t hsz;                 // histogram words per node
  bool need_general;           // any item on the byte-gather path: that of a built node
  Consts K;
  Arena A;
  PlanArgs plan;
  int64_t* hist[2];            // reserve()
  uint8_t* cand;
  unsigned* done;
  uint8_t *fp_send, *fp_recv;  // feature-parallel only, else null
};

// Feature groups, feature list and job table, shipped only when they differ from the last shipped block.
Consts ship_constants(Ctx& c) {
  const tmog::GrowArgs& a = c.a;
  const size_t T = (size_t)a.T;
  std::vector<int32_t> flist(c.L.F_use);
  for (int f = 0; f < c.L.F_use; ++f) flist[f] = c.L.perm_feats.empty() ? f : c.L.perm_feats[f];
  tmog::Staging cs;
  Consts K{nullptr,   // (braced initialisers are evaluated in order: the offsets are those of the members)
           cs.add(c.L.full_groups), cs.add(flist),
           cs.add(a.job_depth, 4 * T), cs.add(a.job_model, 4 * T),
           cs.add(a.job_count, 8 * T), cs.add(a.job_min_inst, 8 * T),
           cs.add(a.job_min_gain, 8 * T), cs.add(a.job_mcw, 8 * T),
           cs.add(a.job_lambda, 8 * T), cs.add(a.job_eps, 8 * T),
           cs.add(c.io.job_eta, 8 * T), cs.add(c.io.job_gamma, 8 * T)};
  const size_t n = cs.buf.size();
  if (c.sl.consts.dev.need(n, slack(n), c.st)) c.sl.last.clear();   // a new block holds nothing yet
  if (cs.buf != c.sl.last) {
    c.sl.consts.ship(cs.buf.data(), n, n + 4096, slack(n), c.st);
    c.sl.last = cs.buf;
  }
  K.dev = c.sl.consts.dev.as();
  return K;
}

// Histograms of two levels, split candidates, ticket counters; feature-parallel: the split records of this rank
// and of every rank of the group.
void reserve(Ctx& c) {
  ResSlot& sl = c.sl;
  auto grown = [&](tmog::DevBuf& b, size_t bytes) {
    b.need(bytes, slack(bytes), c.st);
    return b.as();
  };
  const size_t m = (size_t)c.cp.cap_m;
  for (int k = 0; k < 2; ++k) c.hist[k] = (int64_t*)grown(sl.hist[k], sizeof(int64_t) * (size_t)c.hsz * m);
  c.cand = grown(sl.cand, tmog_hip_split_cand_bytes((int)m, c.L.F_use, c.a.B, c.a.S));
  c.done = sl.done.need(m, slack(sizeof(unsigned) * m), c.st);
  const bool fp = c.a.fp_world > 0;
  const size_t rec = tmog::fp_rec_bytes(c.a.S) * m;
  c.fp_send = fp ? grown(sl.fp_send, rec) : nullptr;
  c.fp_recv = fp ? grown(sl.fp_recv, rec * (size_t)c.a.fp_world) : nullptr;
}

// TMOG_PLAN_PROFILE, TMOG_PLAN_LDS, TMOG_PLAN_THREADS and the planner's LDS attribute: once per process.
struct PlanLaunch {
  bool profile;
  bool lds;      // planner scratch in LDS when the per-level node capacity fits (TMOG_PLAN_LDS=0: global memory)
  int threads;   // of the two single-workgroup kernels (plan, finalisation); TMOG_PLAN_THREADS = 256 / 512 / 1024:
                 // a smaller workgroup finds a CU sooner while the other boosting parts' histogram waves occupy the chip
};
constexpr size_t kPlanLdsMax = 148 * 1024;

const PlanLaunch& plan_launch_config() {
  static const PlanLaunch cfg = [] {
    const char* e = std::getenv("TMOG_PLAN_THREADS");
    const int v = e ? std::atoi(e) : 1024;
    const bool attr = hipFuncSetAttribute((const void*)level_plan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)kPlanLdsMax) == hipSuccess;
    return PlanLaunch{tmog::env_is("TMOG_PLAN_PROFILE", '1'), attr && !tmog::env_is("TMOG_PLAN_LDS", '0'),
                      (v == 256 || v == 512) ? v : 1024};
  }();   // (thread-safe static initialisation)
  return cfg;
}

inline size_t plan_lds_bytes(int64_t cap_nl) {
  return ((size_t)kPlanScratch * sizeof(int64_t) + sizeof(int32_t)) * (size_t)cap_nl + 64;
}

PlanArgs plan_args(const Ctx& c) {
  const tmog::GrowArgs& a = c.a;
  const Caps& cp = c.cp;
  const Consts& K = c.K;
  PlanArgs P = c.A.plan;
  P.T = a.T;
  P.S = a.S;
  P.chunk_rows = (int)a.chunk_rows;
  P.n_groups = (int)c.L.full_groups.size();
  P.n_sc = kNsc;
  P.newton = tmog::hess_gate(a) ? 1 : 0;
  P.subtract = 1;
  P.pair_fuse = 1;
  P.F_use = c.L.F_use;
  P.has_missing = a.missing_bin >= 0 ? 1 : 0;
  P.hsz = c.hsz;
  P.live_dense = c.L.live_dense;
  P.groups = K.at<tmog::FeatGroup>(K.groups);
  P.j_depth = K.at<int32_t>(K.depth);
  P.j_model = K.at<int32_t>(K.model);
  P.j_count = K.at<int64_t>(K.count);
  P.j_inst = K.at<double>(K.inst);
  P.j_gain = K.at<double>(K.gain);
  P.j_mcw = K.at<double>(K.mcw);
  P.j_lam = K.at<double>(K.lam);
  P.j_eps = K.at<double>(K.eps);
  P.rec = c.io.rec;
  P.W = kRecFixed + a.S;
  P.cap_nl = cp.cap_nl;
  P.cap_m = cp.cap_m;
  P.cap_nodes = cp.cap_nodes;
  P.cap_h = cp.cap_h;
  P.cap_c = cp.cap_c;
  P.cap_l = cp.cap_l;
  const PlanLaunch& cfg = plan_launch_config();
  P.profile = cfg.profile ? 1 : 0;
  P.lds_cap = cfg.lds && cp.cap_nl > 0 && plan_lds_bytes(cp.cap_nl) <= kPlanLdsMax ? cp.cap_nl : 0;
  return P;
}

FinArgs fin_args(const Ctx& c) {
  FinArgs Fa = c.A.fin;
  Fa.T = c.a.T;
  Fa.S = c.a.S;
  Fa.mode = c.a.mode;
  Fa.kind = c.a.kind;
  Fa.n_levels = c.cp.D + 1;
  Fa.prune = 0;
  for (int j = 0; j < c.a.T; ++j) Fa.prune |= c.io.job_gamma[j] > 0.0 ? 1 : 0;
  Fa.rec = c.io.rec;
  Fa.W = c.plan.W;
  Fa.level_off = c.plan.level_off;
  Fa.cnt = c.plan.cnt;
  Fa.leaf_pos = c.plan.leaf_pos;
  Fa.j_lam = c.plan.j_lam;
  Fa.j_eta = c.K.at<double>(c.K.eta);
  Fa.j_gamma = c.K.at<double>(c.K.gamma);
  Fa.gid_value = c.io.gid_value;
  Fa.gid_tree = c.io.gid_tree;
  return Fa;
}

// Level d: plan -> leaf_collect -> zero -> hist_build -> pair_scan -> split_find -> [all-gather + merge] ->
// partition. Every launch gets a host upper bound of its grid and reads the real count from c.plan.cnt.
// Levels 0..D build histograms (level D only when D == 0: deeper, no node of level D may split); plan D + 1
// only turns the last decisions into leaves.
void enqueue_level(Ctx& c, int d) {
  const tmog::GrowArgs& a = c.a;
  const Caps& cp = c.cp;
  const tmog::GroupLayout& L = c.L;
  const Arena& A = c.A;
  PlanArgs& P = c.plan;
  hipStream_t st = c.st;
  const int B = a.B, S = a.S, F_use = L.F_use, n_groups = (int)L.full_groups.size();
  const int64_t total = cp.total;
  int* cnt = P.cnt;
  const int32_t* flist = c.K.at<int32_t>(c.K.flist);
  uint32_t* const rows[2] = {a.rows, a.rows_alt};
  int32_t* const gh[2] = {a.gh, a.gh_alt};
  const bool use_gh = a.gh != nullptr && a.gh_alt != nullptr && a.mode == 2;
  const bool fp = a.fp_world > 0;
  const size_t fp_rb = tmog::fp_rec_bytes(S);

  P.d = d;
  hipLaunchKernelGGL(level_plan_kernel, dim3(1), dim3(plan_launch_config().threads),
                     P.lds_cap > 0 ? plan_lds_bytes(P.lds_cap) : 0, st, P);
  kchk((int)hipGetLastError(), "level_plan");
  const int64_t nprev = d > 0 ? cp.nmax[d - 1] : 0;
  const int64_t lbound = tmog::leaf_items_bound(a.chunk_rows, total, nprev) +
                         tmog::leaf_items_bound(a.chunk_rows, total, cp.nmax[d]);
  kchk(tmog_hip_leaf_collect(rows[0], P.litems, (int)std::min(lbound, cp.cap_l), a.leaf_rows, a.leaf_gid, st,
                             rows[1], cnt + C_NL),
       "leaf_collect");
  if (d > cp.D || (d == cp.D && d > 0)) return;
  const int k = d & 1;
  const int64_t mb = cp.nmax[d];
  kchk(tmog_hip_zero_segments(c.hist[k], P.zoff, P.zsize, (int)mb, c.hsz, L.live_dense, B * S, S, st, 0, cnt + C_NZ),
       "zero_segments");
  const int64_t hb = tmog::hist_items_bound(L.full_groups.data(), n_groups, a.chunk_rows, kNsc, total, mb);
  kchk(tmog_hip_hist_build(a.Xb, a.F, rows[k], P.hitems, (int)std::min(hb, cp.cap_h), P.nfo, flist, P.nmd[k],
                           P.nho[k], c.hist[k], B, a.mode, S, a.y, a.t1, a.t2, a.stride, a.qscale,
                           a.mode == 2 ? a.missing_bin : -1, a.csr_ptr, a.csr_col, S, 0, c.need_general ? 1 : 0, st,
                           use_gh ? gh[k] : nullptr, cnt + C_NH, a.wide_rows, a.Xh, a.Fh),
       "hist_build");
  if (d > 0)
    kchk(tmog_hip_pair_scan(c.hist[k], c.hist[k ^ 1], P.poff, P.sj, P.bj, (int)std::max<int64_t>(1, mb / 2), P.nho[k],
                            P.nnf, P.nfo, flist, a.n_bins, B, S, a.kind, P.par[k], a.missing_bin, P.nmd[k], a.qinv,
                            F_use, c.cand, L.split_n_multi, st, cnt + C_NP),
         "pair_scan");
  kchk(tmog_hip_split_find(c.hist[k], (int)mb, P.nho[k], P.nnf, P.nfo, flist, a.n_bins, B, S, a.kind, P.par[k],
                           a.missing_bin, P.nmd[k], a.qinv, F_use, c.cand, A.r_feat, A.r_bin, A.r_gain, A.r_dl,
                           A.r_left, A.r_tot, A.r_cur, L.split_n_multi, c.fp_send, fp ? (int64_t)fp_rb : 0,
                           fp ? a.fp_mlo : 0, fp ? L.fp_nml : 0, fp ? L.fp_obase : 0, st, c.done, cnt + C_M),
       "split_find");
  if (fp) {
    // the ranks' best split per node: all-gather the level's records (the host bound mb of them; the
    // merge reads the device count) and merge them into this level's decisions, all on the stream
    kchk(tmog_hip_fp_allgather(c.fp_send, c.fp_recv, (int64_t)(fp_rb * (size_t)mb), a.fp_comm[0], a.fp_world, st),
         "fp_allgather");
    kchk(tmog_hip_fp_merge_dev(c.fp_recv, a.fp_world, (int)mb, (int64_t)fp_rb, S, A.r_feat, A.r_bin, A.r_gain,
                               A.r_dl, A.r_left, cnt + C_M, st),
         "fp_merge");
  }
  kchk(tmog_hip_partition_fused(a.Xb, a.F, rows[k], rows[k ^ 1], P.citems,
                                (int)std::min(tmog::part_items_bound(total, mb), cp.cap_c), P.nb[k], P.nc[k],
                                A.r_feat, A.r_bin, A.r_dl, P.par[k], A.r_gain, a.missing_bin, A.r_cur, a.XbT, a.N, st,
                                use_gh ? gh[k] : nullptr, use_gh ? gh[k ^ 1] : nullptr, cnt + C_NC, a.wide_rows),
       "partition_fused");
}

// Leaf values, gamma pruning and the created-node header, after the last level.
void enqueue_finalize(const Ctx& c) {
  hipLaunchKernelGGL(tree_finalize_kernel, dim3(1), dim3(plan_launch_config().threads), 0, c.st, fin_args(c));
  kchk((int)hipGetLastError(), "tree_finalize");
}

}  // namespace

extern "C" {

int64_t tmog_hip_resident_cap_nodes(const tmog::GrowArgs* args) {
  const tmog::GrowArgs& a = *args;
  if (!unsupported(a).empty()) return -1;
  const tmog::GroupLayout L = tmog::group_layout<true>(a, false, a.fp_world > 0);
  return caps_of(a, L, kNsc).cap_nodes;
}

// TMOG_PLAN_PROFILE: copy the planner's per-phase tick sums (32 entries, 100 MHz wall clock; [31] = calls).
int tmog_hip_plan_profile(uint64_t* out, int reset) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_plan_prof), sizeof(unsigned long long) * 32, 0,
                                     hipMemcpyDeviceToHost);
  if (e != hipSuccess) return (int)e;
  if (reset) {
    static const unsigned long long zero[32] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_plan_prof), zero, sizeof(zero), 0, hipMemcpyHostToDevice);
  }
  return (int)e;
}

int tmog_hip_resident_error(char* msg, int cap) {
  if (msg && cap > 0) {
    std::strncpy(msg, g_err.c_str(), cap - 1);
    msg[cap - 1] = 0;
  }
  return (int)g_err.size();
}

// Enqueue the growth of one tree per job of the (single) group on a.stream. Returns 0 when enqueued,
// 1 when the configuration is not covered (nothing enqueued; use tmog_hip_grow_forest), -1 on error
// (tmog_hip_resident_error). No host synchronisation with the device.
int tmog_hip_grow_resident(const tmog::GrowArgs* args, const ResidentIO* io) {
  g_err.clear();
  try {
    const tmog::GrowArgs& a = *args;
    const std::string why = unsupported(a);
    if (!why.empty()) {
      g_err = why;
      return 1;
    }
    if (a.slot_base < 0 || a.slot_base >= (int)res_slots().size()) throw std::runtime_error("bad slot");
    int dev = 0;
    hchk(hipGetDevice(&dev), "hipGetDevice");
    (void)tmog_hip_tree_prime();
    ResSlot& sl = res_slots()[a.slot_base];
    if (sl.device != dev) {
      sl = ResSlot();
      sl.device = dev;
    }
    Ctx c{a, *io, sl, (hipStream_t)a.stream, tmog::group_layout<true>(a, false, a.fp_world > 0)};
    c.cp = caps_of(a, c.L, kNsc);
    if (io->cap_nodes < c.cp.cap_nodes) throw std::runtime_error("record buffer too small");
    c.hsz = (int64_t)c.L.F_use * a.B * a.S;
    c.need_general = tmog::node_work(tmog::kNodeNeed, 1, a.chunk_rows, c.L.full_groups.data(),
                                     (int)c.L.full_groups.size(), kNsc, c.L.live_dense, c.hsz).n_general > 0;
    c.K = ship_constants(c);
    Carve probe{nullptr};
    lay_out(probe, c.cp, a.S);
    sl.arena.need(probe.off + 256, slack(probe.off + 256), c.st);
    Carve cv{sl.arena.as()};
    c.A = lay_out(cv, c.cp, a.S);
    reserve(c);
    c.plan = plan_args(c);
    for (int d = 0; d <= c.cp.D + 1; ++d) enqueue_level(c, d);
    enqueue_finalize(c);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

}  // extern "C"
