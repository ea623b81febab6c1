// Native level-synchronous tree grower (host orchestration), shared by the HIP and CPU backends.
//
// This is the runtime half of the histogram tree engine (replaces Spark MLlib's
// per-level RandomForest.findBestSplits driver loop and XGBoost4J's hist updater, e.g.
// OpRandomForestClassifier.scala:59-154, OpGBTClassifier.scala:47-142, OpXGBoostClassifier.scala:47-403).
// One call grows one tree per job, all jobs of a group level by level. Per level the grower plans the
// work items on the host, ships every host array in ONE staged copy, launches the level's kernels
// (histogram, subtraction trick, split scan, partition count), reads every decision back with ONE
// device->host copy, then launches the stable partition and the leaf collection. Job groups run on
// their own host threads and HIP streams, so one group's planning overlaps the other's kernels.
//
// Backends (template parameter BK) provide memory, staging and the kernels:
//   GPU  (hip/tree_grow_hip.hip)   : pinned staging + hipMemcpyAsync, tmog_hip_* launchers
//   CPU  (host/tree_grow_cpu.cpp)  : host memory, tmog_*_cpu functions (bit-identical results)
// Layout contracts are those of hip/tree_hist_kernels.hip (packed rows, int64 fixed-point histograms); how a level's
// nodes become work items is common/tree_plan.hpp, shared with the device planner (hip/tree_resident.hip).
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "common/tmog_abi.h"
#include "common/tree_plan.hpp"
#include "common/tree_rules.hpp"

namespace tmog {

// Deterministic cross-group order of the feature-parallel split exchanges. Every job group grows on its
// own host thread and issues one all-gather per level on its own communicator; left to the threads'
// timing, rank A could enqueue (g0 level L, g1 level L) while rank B enqueues (g1, g0) -- collectives of
// two communicators queued in different orders on different ranks is the classic RCCL/NCCL deadlock once
// two streams share a hardware queue. The turn passes round-robin over the groups that are still
// growing: g0 L0, g1 L0, g0 L1, g1 L1, ..., a finished group drops out. Each group's exchange count is
// identical on every rank (all ranks merge the same decisions), so the global enqueue order is too.
struct FpTurns {
  std::mutex m;
  std::condition_variable cv;
  int turn = 0;
  std::vector<char> done;
  std::vector<int64_t> issued;          // exchanges issued per group (checked against the other ranks' in tests)
  explicit FpTurns(int n) : done(std::max(1, n), 0), issued(std::max(1, n), 0) {}
  void advance_locked() {
    const int n = (int)done.size();
    for (int k = 1; k <= n; ++k) {
      const int c = (turn + k) % n;
      if (!done[c]) {
        turn = c;
        return;
      }
    }
  }
  template <class Fn>
  void run(int g, Fn&& fn) {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return turn == g || done[g]; });
    try {
      fn();
    } catch (...) {
      ++issued[g];
      advance_locked();
      cv.notify_all();
      throw;
    }
    ++issued[g];
    advance_locked();
    cv.notify_all();
  }
  void finish(int g) {
    std::lock_guard<std::mutex> lk(m);
    done[g] = 1;
    if (turn == g) advance_locked();
    cv.notify_all();
  }
};

// Test hook: TMOG_FP_DELAY="rank:group:ms" sleeps before every exchange of that (rank, group), so a
// multi-rank test can skew the groups' timing on one rank and check the order (and the trees) hold.
inline int fp_delay_ms(int rank, int group) {
  const char* e = std::getenv("TMOG_FP_DELAY");
  int r = -1, gg = -1, ms = 0;
  if (e == nullptr || std::sscanf(e, "%d:%d:%d", &r, &gg, &ms) != 3) return 0;
  return (r == rank && gg == group) ? ms : 0;
}

using ::GrowArgs;   // common/tmog_abi.h

// Diagnostic switches of the level loops, each with one reader: the host-planned loop and the device-planned
// loop's support check (hip/tree_resident.hip unsupported()) cannot disagree. Read per call: tests toggle
// them within a process.
inline bool env_is(const char* name, char c) {
  const char* e = std::getenv(name);
  return e && e[0] == c;
}
inline bool pair_scan_enabled() { return !env_is("TMOG_PAIR_SCAN", '0'); }
inline bool fused_reduce_enabled() { return !env_is("TMOG_FUSED_REDUCE", '0'); }
// (the launcher in hip/tree_hist_kernels.hip that acts on this one keeps its own once-per-process read)
inline bool hist_wide_split() { return env_is("TMOG_HIST_WIDE_SPLIT", '1'); }
// Newton growth gates a split on the children's hessian sums: (g, h) statistics, second-order gain.
// TMOG_TREE_HESS_GATE=0: off (A/B and the equality test).
inline bool hess_gate(const GrowArgs& a) {
  return a.mode == 2 && a.kind == 3 && a.S >= 2 && !env_is("TMOG_TREE_HESS_GATE", '0');
}

// Merge of the ranks' records of node j (host twin of tree_split_kernels.hip fp_merge_kernel).
inline void fp_merge_host(const uint8_t* recv, int R, int m, size_t rb, int S, int32_t* feat, int32_t* bin,
                          float* gain, uint8_t* dl, float* left) {
  for (int j = 0; j < m; ++j) fp_merge_node(recv, R, m, j, (int64_t)rb, S, feat, bin, gain, dl, left);
}

struct GroupResult {
  std::vector<int64_t> tree, feat, bin, left, right;
  std::vector<uint8_t> dl;
  std::vector<double> gain, tot;   // tot: n * S
  int64_t leaf_count = 0;
  int S = 1;

  std::vector<int64_t> add(const std::vector<int64_t>& trees) {
    std::vector<int64_t> ids(trees.size());
    for (size_t i = 0; i < trees.size(); ++i) {
      ids[i] = (int64_t)tree.size();
      tree.push_back(trees[i]);
      feat.push_back(-1);
      bin.push_back(-1);
      left.push_back(-1);
      right.push_back(-1);
      dl.push_back(0);
      gain.push_back(0.0);
      for (int s = 0; s < S; ++s) tot.push_back(0.0);
    }
    return ids;
  }
};

struct GrowResult {
  std::vector<GroupResult> groups;
  int status = 0;
  std::string error;
};

// work items of the level kernels (common/tmog_abi.h)
using HistItemH = ::HistItem;
using PartItemH = ::PartItem;
using LeafItemH = ::LeafItem;

// splitmix64 stream for the per-node feature subsets (identical on both backends)
struct SplitMix {
  uint64_t s;
  explicit SplitMix(uint64_t seed) : s(seed) {}
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return next() % n; }
};

// Host staging: arrays appended at 16-byte aligned offsets, shipped as one block by the backend.
struct Staging {
  std::vector<uint8_t> buf;
  size_t add(const void* p, size_t bytes) {
    const size_t off = (buf.size() + 15) & ~size_t(15);
    buf.resize(off + ((bytes + 15) & ~size_t(15)));
    if (bytes) std::memcpy(buf.data() + off, p, bytes);
    return off;
  }
  template <class T>
  size_t add(const std::vector<T>& v) { return add(v.data(), v.size() * sizeof(T)); }
  void clear() { buf.clear(); }
};

// Where split_find writes the feature-parallel split records (rec == nullptr: not feature-parallel).
struct FpSlice {
  uint8_t* rec;
  int64_t rec_bytes;
  int32_t mlo, nml, obase;   // local feature f -> position f < nml ? mlo + f : obase + (f - nml)
};

// n features in near-equal groups of at most 64
inline std::vector<FeatGroup> equal_groups(int n) {
  std::vector<FeatGroup> out;
  if (n <= 0) return out;
  const int ng = std::max(1, (n + 63) / 64);
  const int fg = (n + ng - 1) / ng;
  for (int gi = 0; gi * fg < n; ++gi) out.push_back(FeatGroup{gi * fg, std::min(fg, n - gi * fg), 0});
  return out;
}

// Groups whose sizes are multiples of 4 (<= 64): with a dword-aligned first column every group of the
// wide-load histogram path starts on a dword boundary of the row.
inline std::vector<FeatGroup> equal_groups4(int n) {
  std::vector<FeatGroup> out;
  if (n <= 0) return out;
  const int ng = std::max(1, (n + 63) / 64);
  const int fg = std::min(64, ((n + ng - 1) / ng + 3) / 4 * 4);
  for (int gi = 0; gi * fg < n; ++gi) out.push_back(FeatGroup{gi * fg, std::min(fg, n - gi * fg), 0});
  return out;
}

// TMOG_GROW_TIMING=1: host nanoseconds per level spent planning (building the level's work lists and
// reading the previous level's decisions), issuing (staging copy + kernel launches) and waiting for the
// level's result read-back, summed over every group and call (diagnostics; read by the C ABI)
struct GrowTiming {
  std::atomic<int64_t> plan{0}, issue{0}, wait{0}, levels{0};
};
inline GrowTiming& grow_timing() {
  static GrowTiming t;
  return t;
}

// Histogram feature groups of a job group without per-node feature subsets (or the per-node default),
// shared by the host-planned level loop (grow_group) and the device-planned one (hip/tree_resident.hip).
struct GroupLayout {
  std::vector<FeatGroup> full_groups;
  std::vector<int32_t> perm_feats;
  int split_n_multi = -1;   // GPU split scan: local features [n_multi, F) have one present bin
  int64_t live_dense = -1;  // GPU zero / subtract: words past this prefix are live only at bin 0
  int fp_nml = 0, fp_obase = 0;   // split records: local feature -> position in the full feature list
  int F_use = 0;
};

template <bool GPU>
GroupLayout group_layout(const GrowArgs& a, bool use_subset, bool fp) {
  // Feature groups of the histogram kernel (<= 64 features each). Without per-node subsets the
  // grouping is fixed: with a sparse missing bin (GPU, MODE 2) the one-present-bin columns (one-hot /
  // null indicators) go last; given their row-wise CSR they form one group whose items walk only the
  // present entries of each row (a few per row instead of one byte per column), otherwise groups of
  // their own that the kernel accumulates in registers.
  // The feature order is the same on both backends (stable: multi-bin columns first, then the
  // one-present-bin columns), so split tie-breaks by local feature index stay identical GPU vs CPU.
  GroupLayout L;
  std::vector<FeatGroup>& full_groups = L.full_groups;
  std::vector<int32_t>& perm_feats = L.perm_feats;
  int& split_n_multi = L.split_n_multi;
  int64_t& live_dense = L.live_dense;
  int& fp_nml = L.fp_nml;
  int& fp_obase = L.fp_obase;
  const int F = a.F, B = a.B, S = a.S;
  if (!use_subset && a.mode == 2 && a.missing_bin >= 0 && a.n_bins_host != nullptr) {
    std::vector<int32_t> multi, one;
    for (int f = 0; f < F; ++f) (a.n_bins_host[f] != 1 ? multi : one).push_back(f);
    int m0 = 0, m1 = (int)multi.size(), o0 = 0, o1 = (int)one.size();
    if (fp) {
      m0 = a.fp_mlo; m1 = a.fp_mhi; o0 = a.fp_olo; o1 = a.fp_ohi;
      if (m0 < 0 || m1 > (int)multi.size() || m1 <= m0 || o0 < 0 || o1 > (int)one.size() || o1 < o0)
        throw std::runtime_error("bad feature-parallel slice");
    }
    perm_feats.assign(multi.begin() + m0, multi.begin() + m1);
    const int n_multi = m1 - m0;
    fp_nml = n_multi;
    fp_obase = (int)multi.size() + o0;
    // node totals are read from local feature 0, which must be a multi-bin column: with no multi-bin
    // column at all every histogram word stays written and scanned (no CSR / reduced write-out)
    split_n_multi = n_multi > 0 ? n_multi : -1;
    if (GPU && n_multi > 0) live_dense = (int64_t)n_multi * a.B * a.S;
    perm_feats.insert(perm_feats.end(), one.begin() + o0, one.begin() + o1);
    const char* wenv = std::getenv("TMOG_HIST_WIDE");
    // (32-bit buffer offsets row * F + column: matrices below 2 GiB)
    const bool wide_ok = GPU && a.mode == 2 && S == 2 && F % 4 == 0 && !(wenv && wenv[0] == '0') &&
                         (int64_t)a.N * F < ((int64_t)1 << 31) - 64;
    for (FeatGroup g : (wide_ok ? equal_groups4(n_multi) : equal_groups(n_multi))) {
      if (wide_ok) {
        bool ok = perm_feats[g.f0] % 4 == 0;
        for (int i = 1; ok && i < g.nf; ++i) ok = perm_feats[g.f0 + i] == perm_feats[g.f0] + i;
        // with a compact histogram matrix every wide group must lie inside it (the kernel reads Xh only)
        if (ok && a.Xh != nullptr) ok = a.Fh % 4 == 0 && perm_feats[g.f0] + g.nf <= a.Fh;
        if (ok) g.flags |= TMOG_ITEM_WIDE;   // contiguous dword-aligned physical columns
      }
      full_groups.push_back(g);
    }
    const int n_one = o1 - o0;
    if (GPU && a.csr_ptr && a.csr_col && n_multi > 0 && n_one > 0 && a.csr_nf == n_one &&
        2 * n_one + 4 + 64 * 4 <= 64 * (B * S + 1))   // sums + list lengths of the CSR item (tree_hist_kernels.hip)
      full_groups.push_back(FeatGroup{n_multi, n_one, TMOG_ITEM_CSR});   // one item walks the rows' CSR lists
    else
      for (const FeatGroup& g : equal_groups(n_one))
        full_groups.push_back(FeatGroup{n_multi + g.f0, g.nf, GPU ? TMOG_ITEM_REG : 0});
  } else if (fp) {
    if (a.fp_mlo < 0 || a.fp_mhi > F || a.fp_mhi <= a.fp_mlo) throw std::runtime_error("bad feature-parallel slice");
    for (int f = a.fp_mlo; f < a.fp_mhi; ++f) perm_feats.push_back(f);
    fp_nml = (int)perm_feats.size();
    fp_obase = F;
    full_groups = equal_groups(fp_nml);
  } else {
    full_groups = equal_groups(F);
  }
  L.F_use = perm_feats.empty() ? F : (int)perm_feats.size();
  return L;
}

template <class BK>
void grow_group(BK& bk, const GrowArgs& a, int g, GroupResult& R, FpTurns* turns = nullptr) {
  const int j0 = a.group_start[g], j1 = a.group_start[g + 1];
  const int T = j1 - j0;
  const int F = a.F, S = a.S, B = a.B;
  R.S = S;
  if (T <= 0) return;
  int64_t entry0 = 0;
  for (int j = 0; j < j0; ++j) entry0 += a.job_count[j];
  int64_t total = 0;
  for (int j = j0; j < j1; ++j) total += a.job_count[j];
  uint32_t* rows = a.rows + entry0;
  uint32_t* rows_alt = a.rows_alt + entry0;
  uint32_t* leaf_rows = a.collect_leaves ? a.leaf_rows + entry0 : nullptr;
  int32_t* leaf_gid = a.collect_leaves ? a.leaf_gid + entry0 : nullptr;
  int64_t leaf_pos = 0;

  std::vector<int32_t> fsub(T);
  bool use_subset = false;
  int max_depth = 0;
  for (int t = 0; t < T; ++t) {
    const int k = a.job_fsub[j0 + t];
    fsub[t] = (k <= 0 || k >= F) ? F : k;
    use_subset |= fsub[t] < F;
    max_depth = std::max(max_depth, a.job_depth[j0 + t]);
  }
  SplitMix rng((uint64_t)a.rng_seed + 1000003ull * (uint64_t)g);

  std::vector<int64_t> lv_tree(T), lv_begin(T), lv_count(T);
  for (int t = 0; t < T; ++t) {
    lv_tree[t] = t;
    lv_count[t] = a.job_count[j0 + t];
    lv_begin[t] = t ? lv_begin[t - 1] + lv_count[t - 1] : 0;
  }
  std::vector<int64_t> lv_gid = R.add(lv_tree);

  const int32_t* all_feats = bk.all_features(F);
  int64_t* hist = nullptr;
  int64_t* prev_hist = nullptr;
  int cur_slot = 0;          // the backend keeps two grow-only histogram buffers per group
  std::vector<int64_t> pair_parent_off;
  Staging st1, st2, st3;   // level arrays (slot 0), scatter items (slot 1), leaf items (slot 2)

  auto collect = [&](const std::vector<int64_t>& idx) {
    if (!a.collect_leaves) return;
    std::vector<LeafItemH> items;
    for (int64_t i : idx) {
      const int64_t c = lv_count[i];
      for (int64_t k = 0, nl = leaf_items(c, a.chunk_rows); k < nl; ++k)
        items.push_back(leaf_item_at(k, lv_begin[i], c, a.chunk_rows, leaf_pos, (int32_t)lv_gid[i], 0));
      leaf_pos += std::max<int64_t>(c, 0);
    }
    if (items.empty()) return;
    st3.clear();
    const size_t o = st3.add(items);
    const uint8_t* d = bk.ship(st3, 2);
    bk.leaf_collect(rows, d + o, (int)items.size(), leaf_rows, leaf_gid);
  };

  const bool fp = a.fp_world > 0;   // 1 rank is allowed (tests run the exchange path on one GPU)
  if (fp && use_subset) throw std::runtime_error("feature-parallel growth needs jobs without feature subsets");
  GroupLayout L = group_layout<BK::kGPU>(a, use_subset, fp);
  std::vector<FeatGroup>& full_groups = L.full_groups;
  std::vector<int32_t>& perm_feats = L.perm_feats;
  const int split_n_multi = L.split_n_multi;
  const int64_t live_dense = L.live_dense;
  const int fp_nml = L.fp_nml, fp_obase = L.fp_obase;
  const int F_use = perm_feats.empty() ? F : (int)perm_feats.size();
  const bool trace = std::getenv("TMOG_GROW_TRACE") != nullptr;   // progress to stderr (debugging)
  if (trace)
    std::fprintf(stderr, "[grow g%d] T=%d F=%d F_use=%d S=%d B=%d fp=%d slice m[%d,%d) o[%d,%d)\n", g, T, F, F_use, S,
                 B, (int)fp, a.fp_mlo, a.fp_mhi, a.fp_olo, a.fp_ohi);
  // GPU histogram items accumulate a chunk of the statistics when a B x S table exceeds the LDS (many
  // classes / wide bins): one item per chunk, each writing disjoint words of the node histogram
  const int stat_sc = bk.stat_chunk(B, S);
  const int n_sc = (S + stat_sc - 1) / stat_sc;
  if (n_sc > 256) throw std::runtime_error("too many statistic chunks (classes x bins too large)");
  const int fp_mlo = fp ? a.fp_mlo : 0;
  const size_t fp_rb = fp_rec_bytes(S);
  const bool newton = hess_gate(a);
  static const bool timing = std::getenv("TMOG_GROW_TIMING") != nullptr;
  using tclock = std::chrono::steady_clock;
  auto ns_since = [](tclock::time_point t) {
    return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(tclock::now() - t).count();
  };
  tclock::time_point t_lvl = tclock::now();
  for (int depth = 0; depth <= max_depth; ++depth) {
    const int64_t n = (int64_t)lv_gid.size();
    if (n == 0) break;
    if (timing) t_lvl = tclock::now();
    std::vector<int> flags(n);   // kNode* bits (common/tree_plan.hpp)
    std::vector<int64_t> hist_nodes;
    auto can = [&](int64_t i) {
      const int t = (int)lv_tree[i];
      const bool gate = newton && depth > 0;   // the hessian: the node's second total, from its parent's split
      return can_split(depth, a.job_depth[j0 + t], lv_count[i], a.job_min_inst[j0 + t], gate, a.job_mcw[j0 + t],
                       gate ? R.tot[(size_t)lv_gid[i] * S + 1] : 0.0);
    };
    // subtraction trick: children come in (left, right) pairs
    const bool subtract = a.subtract && !use_subset && prev_hist && depth > 0;
    if (depth == 0)
      for (int64_t i = 0; i < n; ++i) flags[i] = root_flags(can(i));
    else
      for (int64_t q = 0; 2 * q + 1 < n; ++q)
        sibling_flags(can(2 * q), can(2 * q + 1), lv_count[2 * q], lv_count[2 * q + 1], subtract, &flags[2 * q],
                      &flags[2 * q + 1]);
    for (int64_t i = 0; i < n; ++i)
      if (flags[i] & kNodeNeed) hist_nodes.push_back(i);
    if (hist_nodes.empty()) {
      std::vector<int64_t> all(n);
      for (int64_t i = 0; i < n; ++i) all[i] = i;
      collect(all);
      break;
    }
    const int m = (int)hist_nodes.size();
    // ---- per-node feature lists
    std::vector<int32_t> feat_list, feat_off(m), nfeat(m);
    if (use_subset) {
      std::vector<int32_t> perm(F);
      for (int j = 0; j < m; ++j) {
        const int k = fsub[lv_tree[hist_nodes[j]]];
        for (int f = 0; f < F; ++f) perm[f] = f;
        for (int i = 0; i < k; ++i) std::swap(perm[i], perm[i + (int)rng.below((uint64_t)(F - i))]);
        std::sort(perm.begin(), perm.begin() + k);
        feat_off[j] = (int32_t)feat_list.size();
        nfeat[j] = k;
        feat_list.insert(feat_list.end(), perm.begin(), perm.begin() + k);
      }
    } else {
      for (int j = 0; j < m; ++j) {
        feat_off[j] = 0;
        nfeat[j] = F_use;
      }
      if (!perm_feats.empty()) feat_list = perm_feats;
    }
    std::vector<int64_t> hsz(m), hoff(m);
    int64_t hwords = 0;
    int max_nf = 0;
    for (int j = 0; j < m; ++j) {
      hsz[j] = (int64_t)nfeat[j] * B * S;
      hoff[j] = hwords;
      hwords += hsz[j];
      max_nf = std::max(max_nf, (int)nfeat[j]);
    }
    hist = bk.hist_buffer(cur_slot, (size_t)hwords);
    std::vector<int64_t> loc(n, -1);
    for (int j = 0; j < m; ++j) loc[hist_nodes[j]] = j;
    // ---- sibling pairs: the big node is derived from the parent's histogram and the small node's
    std::vector<int64_t> d_big, d_small, d_poff;
    for (int64_t q = 0; 2 * q + 1 < n; ++q) {
      const int64_t li = 2 * q, ri = 2 * q + 1;
      if (!(flags[li] & kNodePairLeft)) continue;
      const bool left_big = flags[li] & kNodeDerived;
      d_big.push_back(loc[left_big ? li : ri]);
      d_small.push_back(loc[left_big ? ri : li]);
      d_poff.push_back(pair_parent_off[q]);
    }
    // GPU: a sibling pair's subtraction and both children's split scans run as one pass (pair_scan_kernel)
    // -- the two nodes are flagged (paired slot) so the node-wise scan skips them; same decisions
    const bool pair_fuse = BK::kGPU && !use_subset && S <= 16 && B <= 64 && !d_big.empty() && pair_scan_enabled();
    std::vector<int32_t> d_sj, d_bj;
    if (pair_fuse)
      for (size_t q = 0; q < d_big.size(); ++q) {
        d_sj.push_back((int32_t)d_small[q]);
        d_bj.push_back((int32_t)d_big[q]);
      }
    std::vector<int64_t> nb(m), nc(m);
    std::vector<int32_t> nmd(m);
    std::vector<float> params((size_t)m * kPrmStride, 0.f);
    for (int j = 0; j < m; ++j) {
      const int64_t i = hist_nodes[j];
      const int t = (int)lv_tree[i];
      nb[j] = lv_begin[i];
      nc[j] = lv_count[i];
      nmd[j] = a.job_model[j0 + t];
      fill_node_params(&params[(size_t)j * kPrmStride], a.job_min_inst[j0 + t], a.job_min_gain[j0 + t],
                       a.job_mcw[j0 + t], a.job_lambda[j0 + t], pair_fuse && (flags[i & ~(int64_t)1] & kNodePairLeft),
                       a.missing_bin >= 0, a.job_eps[j0 + t], flags[i] & kNodeCan);
    }
    // ---- work items (GPU) / built-node arrays (CPU), laid out by common/tree_plan.hpp
    std::vector<HistItemH> hitems;
    std::vector<PartItemH> citems;
    std::vector<int64_t> z_off, z_size;
    std::vector<int64_t> zc_off, zc_size;   // nodes whose only multi-item group is the CSR one: zero its words
    std::vector<int64_t> b_nb, b_nc, b_nho;
    std::vector<int32_t> b_nfo, b_nnf, b_nmd;
    std::vector<NodeWork> work(m);
    std::vector<std::vector<FeatGroup>> sub_groups(use_subset ? m : 0);   // per-node subsets: groups of the node's own
    auto groups_of = [&](int j) -> const std::vector<FeatGroup>& { return use_subset ? sub_groups[j] : full_groups; };
    int n_wide = 0;
    int64_t n_other = 0, n_general = 0;
    for (int j = 0; j < m; ++j) {
      if (use_subset) sub_groups[j] = equal_groups(nfeat[j]);
      const std::vector<FeatGroup>& grp = groups_of(j);
      const NodeWork& w = work[j] = node_work(flags[hist_nodes[j]], nc[j], a.chunk_rows, grp.data(), (int)grp.size(),
                                              n_sc, live_dense, hsz[j]);
      for (int64_t k = 0; k < w.n_part; ++k) citems.push_back(part_item_at(j, k, nb[j], nc[j]));
      if (flags[hist_nodes[j]] & kNodeDerived) continue;
      b_nb.push_back(nb[j]);
      b_nc.push_back(nc[j]);
      b_nho.push_back(hoff[j]);
      b_nfo.push_back(feat_off[j]);
      b_nnf.push_back(nfeat[j]);
      b_nmd.push_back(nmd[j]);
      if (w.zero != kZeroNone) {
        int64_t zo, zs;
        zero_segment(w.zero, hoff[j], hsz[j], live_dense, &zo, &zs);
        (w.zero == kZeroCsr ? zc_off : z_off).push_back(zo);
        (w.zero == kZeroCsr ? zc_size : z_size).push_back(zs);
      }
      n_wide += (int)w.n_wide;
      n_other += w.n_other;
      n_general += w.n_general;
    }
    // wide-load items first: the GPU launches them as a kernel of their own (fewer registers)
    hitems.reserve((size_t)(n_wide + n_other));
    for (const bool wide : {true, false})
      for (int j = 0; j < m; ++j) {
        const std::vector<FeatGroup>& grp = groups_of(j);
        for (int64_t k = 0, nk = wide ? work[j].n_wide : work[j].n_other; k < nk; ++k)
          hitems.push_back(hist_item_at(wide, j, k, nb[j], nc[j], a.chunk_rows, grp.data(), (int)grp.size(), n_sc,
                                        live_dense));
      }
    const int need_general = n_general > 0;   // any item on the byte-gather path (not CSR, not wide-load)?
    std::vector<int64_t> d_soff, d_ooff, d_size;
    int64_t d_max = 0;
    for (size_t q = 0; q < d_big.size(); ++q) {
      d_soff.push_back(hoff[d_small[q]]);
      d_ooff.push_back(hoff[d_big[q]]);
      d_size.push_back(hsz[d_big[q]]);
      d_max = std::max(d_max, hsz[d_big[q]]);
    }
    int64_t z_max = 0, zc_max = 0;
    for (int64_t z : z_size) z_max = std::max(z_max, z);
    for (int64_t z : zc_size) zc_max = std::max(zc_max, z);
    // ---- ship everything in one copy
    st1.clear();
    const size_t o_nfo = st1.add(feat_off), o_nnf = st1.add(nfeat), o_nmd = st1.add(nmd), o_nho = st1.add(hoff);
    const size_t o_par = st1.add(params);
    const bool own_list = use_subset || !perm_feats.empty();
    const size_t o_fl = own_list ? st1.add(feat_list) : 0;
    const size_t o_hit = st1.add(hitems), o_cit = st1.add(citems);
    std::vector<int64_t> z_off_all(z_off), z_size_all(z_size);
    z_off_all.insert(z_off_all.end(), zc_off.begin(), zc_off.end());
    z_size_all.insert(z_size_all.end(), zc_size.begin(), zc_size.end());
    const size_t o_zo = st1.add(z_off_all), o_zs = st1.add(z_size_all);
    const size_t o_dp = st1.add(d_poff), o_ds = st1.add(d_soff), o_do = st1.add(d_ooff), o_dz = st1.add(d_size);
    const size_t o_bnb = st1.add(b_nb), o_bnc = st1.add(b_nc), o_bnfo = st1.add(b_nfo), o_bnnf = st1.add(b_nnf);
    const size_t o_bnmd = st1.add(b_nmd), o_bnho = st1.add(b_nho);
    const size_t o_nb = st1.add(nb), o_nc = st1.add(nc);
    const size_t o_sj = st1.add(d_sj), o_bj = st1.add(d_bj);
    tclock::time_point t_issue = tclock::now();
    if (timing) grow_timing().plan += ns_since(t_lvl);
    const uint8_t* d1 = bk.ship(st1, 0);
#define TM_P(T_, off) ((T_*)(d1 + (off)))
    const int32_t* flist = own_list ? TM_P(const int32_t, o_fl) : all_feats;
    // ---- histograms
    // one launch: the first z_off.size() segments are whole node histograms (dense prefix live_dense), the
    // rest start at a node's one-present-bin region (dense prefix 0)
    bk.zero_segments(hist, TM_P(const int64_t, o_zo), TM_P(const int64_t, o_zs), (int)(z_off.size() + zc_off.size()),
                     std::max(z_max, zc_max), live_dense, a.B * a.S, a.S, (int)z_off.size());
    bk.hist_build(a, rows, hitems.size() ? (const void*)(d1 + o_hit) : nullptr, (int)hitems.size(),
                  TM_P(const int32_t, o_nfo), flist, TM_P(const int32_t, o_nmd), TM_P(const int64_t, o_nho), hist,
                  (int)b_nb.size(), TM_P(const int64_t, o_bnb), TM_P(const int64_t, o_bnc),
                  TM_P(const int32_t, o_bnfo), TM_P(const int32_t, o_bnnf), TM_P(const int32_t, o_bnmd),
                  TM_P(const int64_t, o_bnho), stat_sc, n_wide, need_general);
    bool pairs_done = false;
    if constexpr (BK::kGPU) {
      if (pair_fuse) {
        bk.pair_scan(a, hist, prev_hist, TM_P(const int64_t, o_dp), TM_P(const int32_t, o_sj),
                     TM_P(const int32_t, o_bj), (int)d_sj.size(), TM_P(const int64_t, o_nho),
                     TM_P(const int32_t, o_nnf), TM_P(const int32_t, o_nfo), flist, TM_P(const float, o_par),
                     TM_P(const int32_t, o_nmd), max_nf, m, split_n_multi);
        pairs_done = true;
      }
    }
    if (!d_big.empty() && !pairs_done)
      bk.hist_subtract(hist, prev_hist, TM_P(const int64_t, o_dp), TM_P(const int64_t, o_ds),
                       TM_P(const int64_t, o_do), TM_P(const int64_t, o_dz), (int)d_big.size(), d_max, live_dense,
                       a.B * a.S, a.S);
    // ---- split scan + (GPU) one-pass partition -> one result block: decisions + per-node slot cursors
    const int64_t ncit = (int64_t)citems.size();
    const size_t r_cl = 0, r_feat = r_cl + 16 * (size_t)m, r_bin = r_feat + 4 * (size_t)m, r_gain = r_bin + 4 * (size_t)m;
    const size_t r_left = r_gain + 4 * (size_t)m, r_tot = r_left + 4 * (size_t)m * S, r_dl = r_tot + 4 * (size_t)m * S;
    const size_t r_bytes = r_dl + (size_t)m;
    uint8_t* res = bk.result_buffer(r_bytes);
    uint8_t* fp_send = fp ? bk.fp_send_buffer(fp_rb * (size_t)m) : nullptr;
    const FpSlice fps{fp_send, (int64_t)fp_rb, fp_mlo, fp_nml, fp_obase};
    bk.split_find(a, hist, m, TM_P(const int64_t, o_nho), TM_P(const int32_t, o_nnf), TM_P(const int32_t, o_nfo),
                  flist, TM_P(const float, o_par), TM_P(const int32_t, o_nmd), max_nf, (int32_t*)(res + r_feat),
                  (int32_t*)(res + r_bin), (float*)(res + r_gain), res + r_dl, (float*)(res + r_left),
                  (float*)(res + r_tot), (int64_t*)(res + r_cl), use_subset ? -1 : split_n_multi, fps);
    if (trace) std::fprintf(stderr, "[grow g%d] depth %d: %d nodes split_find done\n", g, depth, m);
    if (fp) {  // all-gather the ranks' best splits, merge into this level's decisions (on-stream on the GPU)
      if (const int ms = fp_delay_ms(a.fp_rank, g)) std::this_thread::sleep_for(std::chrono::milliseconds(ms));
      auto xchg = [&] {
        bk.fp_exchange_merge(a, fp_send, m, fp_rb, (int32_t*)(res + r_feat), (int32_t*)(res + r_bin),
                             (float*)(res + r_gain), res + r_dl, (float*)(res + r_left));
      };
      if (turns != nullptr) turns->run(g, xchg);
      else xchg();
      if (trace) std::fprintf(stderr, "[grow g%d] depth %d: exchange + merge issued\n", g, depth);
    }
    if (BK::kGPU)   // partition in place of the node ranges, straight from the device decisions
      bk.partition_fused(a, rows, rows_alt, d1 + o_cit, (int)ncit, TM_P(const int64_t, o_nb),
                         TM_P(const int64_t, o_nc), (const int32_t*)(res + r_feat), (const int32_t*)(res + r_bin),
                         res + r_dl, TM_P(const float, o_par), (const float*)(res + r_gain), (int64_t*)(res + r_cl));
    tclock::time_point t_wait = tclock::now();
    if (timing) grow_timing().issue += ns_since(t_issue);
    const uint8_t* h = bk.fetch(res, r_bytes);
    if (timing) {
      grow_timing().wait += ns_since(t_wait);
      grow_timing().levels += 1;
      t_lvl = tclock::now();
    }
    const int64_t* h_cur = (const int64_t*)(h + r_cl);   // GPU: [left, right] entries per node
    const int32_t* h_feat = (const int32_t*)(h + r_feat);
    const int32_t* h_bin = (const int32_t*)(h + r_bin);
    const float* h_gain = (const float*)(h + r_gain);
    const float* h_left = (const float*)(h + r_left);
    const float* h_tot = (const float*)(h + r_tot);
    const uint8_t* h_dl = h + r_dl;
    // ---- decisions
    std::vector<int64_t> sl;
    for (int j = 0; j < m; ++j) {
      const int64_t gid = lv_gid[hist_nodes[j]];
      for (int s = 0; s < S; ++s) R.tot[(size_t)gid * S + s] = (double)h_tot[(size_t)j * S + s];
      const float* P = &params[(size_t)j * kPrmStride];
      if (split_accepted(P, h_feat[j], h_gain + j)) sl.push_back(j);
    }
    {
      std::vector<uint8_t> splits(n, 0);
      for (int64_t j : sl) splits[hist_nodes[j]] = 1;
      std::vector<int64_t> lf;
      for (int64_t i = 0; i < n; ++i)
        if (!splits[i]) lf.push_back(i);
      collect(lf);
    }
    if (sl.empty()) break;
    const int64_t ns = (int64_t)sl.size();
    std::vector<int64_t> counts_sl(ns), out_begin(ns), nl(ns, 0);
    for (int64_t q = 0; q < ns; ++q) {
      const int64_t j = sl[q], gid = lv_gid[hist_nodes[j]];
      R.feat[gid] = h_feat[j];
      R.bin[gid] = h_bin[j];
      R.dl[gid] = h_dl[j];
      R.gain[gid] = (double)h_gain[j];
      counts_sl[q] = nc[j];
      out_begin[q] = q ? out_begin[q - 1] + counts_sl[q - 1] : 0;
    }
    // ---- partition of the splitting nodes' entries
    if (BK::kGPU) {
      for (int64_t q = 0; q < ns; ++q) {
        nl[q] = h_cur[2 * sl[q]];
        if (nl[q] < 0 || nl[q] + h_cur[2 * sl[q] + 1] != nc[sl[q]])
          throw std::runtime_error("partition cursor mismatch at depth " + std::to_string(depth));
      }
    } else {
      std::vector<int64_t> s_nb(ns), s_nc(ns);
      std::vector<int32_t> s_f(ns), s_b(ns);
      std::vector<uint8_t> s_d(ns);
      for (int64_t q = 0; q < ns; ++q) {
        const int64_t j = sl[q];
        s_nb[q] = nb[j];
        s_nc[q] = nc[j];
        s_f[q] = h_feat[j];
        s_b[q] = h_bin[j];
        s_d[q] = h_dl[j];
      }
      bk.partition_nodes(a, rows, rows_alt, (int)ns, s_nb.data(), s_nc.data(), s_f.data(), s_b.data(), s_d.data(),
                         out_begin.data(), nl.data());
    }
    // ---- next level: (left, right) children pairs
    std::vector<int64_t> ch_tree(2 * ns);
    for (int64_t q = 0; q < ns; ++q) ch_tree[2 * q] = ch_tree[2 * q + 1] = lv_tree[hist_nodes[sl[q]]];
    std::vector<int64_t> ch = R.add(ch_tree);
    std::vector<int64_t> new_begin(2 * ns), new_count(2 * ns);
    pair_parent_off.assign(ns, 0);
    for (int64_t q = 0; q < ns; ++q) {
      const int64_t j = sl[q], gid = lv_gid[hist_nodes[j]];
      const int64_t gl = ch[2 * q], gr = ch[2 * q + 1];
      R.left[gid] = gl;
      R.right[gid] = gr;
      for (int s = 0; s < S; ++s) {
        const double lt = (double)h_left[(size_t)j * S + s];
        const double tt = (double)h_tot[(size_t)j * S + s];
        R.tot[(size_t)gl * S + s] = lt;
        R.tot[(size_t)gr * S + s] = tt - lt;
      }
      const int64_t b0 = BK::kGPU ? nb[j] : out_begin[q];   // GPU children stay inside the parent's range
      new_begin[2 * q] = b0;
      new_begin[2 * q + 1] = b0 + nl[q];
      new_count[2 * q] = nl[q];
      new_count[2 * q + 1] = counts_sl[q] - nl[q];
      pair_parent_off[q] = hoff[j];
    }
#undef TM_P
    if (timing) grow_timing().plan += ns_since(t_lvl);
    std::swap(hist, prev_hist);
    cur_slot ^= 1;
    std::swap(rows, rows_alt);
    lv_tree = ch_tree;
    lv_gid = ch;
    lv_begin = new_begin;
    lv_count = new_count;
  }
  bk.finish();
  R.leaf_count = leaf_pos;
}

// Result accessors shared by both C ABIs.
inline int64_t result_nodes(const GrowResult* r, int g) { return (int64_t)r->groups[g].tree.size(); }

inline void result_copy(const GrowResult* r, int g, int64_t* tree, int64_t* feat, int64_t* bin, uint8_t* dl,
                        double* gain, double* tot, int64_t* left, int64_t* right) {
  const GroupResult& R = r->groups[g];
  const size_t n = R.tree.size();
  std::memcpy(tree, R.tree.data(), n * 8);
  std::memcpy(feat, R.feat.data(), n * 8);
  std::memcpy(bin, R.bin.data(), n * 8);
  std::memcpy(dl, R.dl.data(), n);
  std::memcpy(gain, R.gain.data(), n * 8);
  std::memcpy(tot, R.tot.data(), n * R.S * 8);
  std::memcpy(left, R.left.data(), n * 8);
  std::memcpy(right, R.right.data(), n * 8);
}

}  // namespace tmog
