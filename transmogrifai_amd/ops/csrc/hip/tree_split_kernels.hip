// Split finding of the histogram tree engine for CDNA4 (gfx950): the narrow scans (split_scan_kernel, and
// pair_scan_kernel fused with the sibling subtraction), the wide scan, the per-node reduction and the
// feature-parallel merge, over the fixed-point histograms of tree_hist_kernels.hip (layout contract there).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <stdint.h>
#include <math.h>

#include "common/tree_rules.hpp"
#include "hip/tmog_hip_abi.h"
#include "hip/tree_dev.hpp"

namespace {

using namespace tmog;   // common/tree_rules.hpp: the split / growth rules shared with the CPU twin

// Wave64 inclusive prefix sum of an int64 on the DPP lane network (GFX9 sequence: row_shr 1 / 2 / 4 / 8 inside
// the 16-lane rows, then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3), two 32-bit halves
// moved per step and added as one 64-bit value: 12 DPP moves + 6 adds instead of 6 x 2 ds_bpermute (LDS
// crossbar) + selects. Lanes without a source keep `old` = 0. Integer sums: identical to any other order.
template <int CTRL, int ROWS>
__device__ __forceinline__ int64_t dpp_shift64(int64_t v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(uint64_t)v, CTRL, ROWS, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((uint64_t)v >> 32), CTRL, ROWS, 0xF, false);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}
__device__ __forceinline__ int64_t wave_scan64(int64_t v) {
  v += dpp_shift64<0x111, 0xF>(v);    // row_shr:1
  v += dpp_shift64<0x112, 0xF>(v);    // row_shr:2
  v += dpp_shift64<0x114, 0xF>(v);    // row_shr:4
  v += dpp_shift64<0x118, 0xF>(v);    // row_shr:8
  v += dpp_shift64<0x142, 0xA>(v);    // row_bcast:15 -> rows 1, 3
  v += dpp_shift64<0x143, 0xC>(v);    // row_bcast:31 -> rows 2, 3
  return v;
}

__device__ __forceinline__ int64_t readlane64(int64_t v, int l) {
  const int lo = __builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, l);
  const int hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

// ------------------------------------------------------------------------------- split finding
// No FMA contraction from here on: gains are evaluated with exactly the CPU twin's IEEE operation
// sequence, so near-tied candidates resolve identically on both paths (hipcc contracts by default).
#pragma clang fp contract(off)
// Loops over the statistics of a node inside the SM-templated scans: unrolled to the compile-time bound with a
// runtime guard, so the per-statistic arrays (totals, scales, left / right sums) stay in registers -- a loop to
// the runtime S indexes them dynamically and puts them in scratch memory
#define TM_FOR_S(s) _Pragma("unroll") for (int s = 0; s < SM; ++s) if (s < S)

// A candidate as three 8-byte agent-scope (sc1) words -- stores that bypass the XCD-local caching and
// loads served from L2, for the hand-off between workgroups of the fused split reduction
__device__ __forceinline__ void store_best_sc1(SplitCand* p, const SplitCand& b) {
  uint64_t* w = reinterpret_cast<uint64_t*>(p);
  __hip_atomic_store(w, (uint64_t)__double_as_longlong(b.gain), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(w + 1, (uint64_t)(uint32_t)b.f | ((uint64_t)(uint32_t)b.b << 32), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(w + 2, (uint64_t)(uint32_t)b.dl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ SplitCand load_best_sc1(const SplitCand* p) {
  const uint64_t* w = reinterpret_cast<const uint64_t*>(p);
  const uint64_t g = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint64_t fb = __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint64_t dl = __hip_atomic_load(w + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return SplitCand{__longlong_as_double((long long)g), (int)(uint32_t)fb, (int)(uint32_t)(fb >> 32), (int)(uint32_t)dl};
}

// the wave's best candidate, on every lane
__device__ __forceinline__ void wave_best(SplitCand& best) {
  for (int off = 32; off > 0; off >>= 1) {
    SplitCand o;
    o.gain = __shfl_xor(best.gain, off, 64);
    o.f = __shfl_xor(best.f, off, 64);
    o.b = __shfl_xor(best.b, off, 64);
    o.dl = __shfl_xor(best.dl, off, 64);
    if (better(o, best)) best = o;
  }
}

// Split scan, two kernels. split_scan_kernel: grid (node, feature block of FPB = 16 features); each
// of the 4 waves scans 4 features (lane = bin, B <= 64) with an exact int64 wave prefix sum of the
// fixed-point histogram, converting to double only to evaluate gains (identical arithmetic to
// tmog_split_find_cpu, so both pick the same split bit for bit); the block's best candidate goes to
// cand[node][fb]. split_reduce_kernel: one wave per node picks the best candidate with the CPU's
// tie-break (gain, then lowest feature, dl, bin) and sums the winner's left statistics. Spreading a
// node over feature blocks fills the chip at the shallow levels (6 root nodes = 6 workgroups before).
// SM = compile-time bound on S (register arrays sized to it).
constexpr int FPB = 16;      // default features per scan workgroup (TMOG_SPLIT_FPB: 4, 8 or 16; 4 waves)

// Candidate slots per node: the node's feature blocks rounded up to 16 (16 x 24 B = 3 whole 128-B lines), so
// no cache line holds two nodes' candidates -- a reducer's L2 never caches a line of a node it has not
// finished (the fused split reduction's sc1 hand-off)
static inline int cand_stride(int fbmax) { return (fbmax + 15) & ~15; }

// TMOG_SCAN_GENERIC=1: kind 3 (Newton) also takes the generic instantiation of the narrow scans (run-time kind,
// unpipelined loads) -- the reference of the Newton instantiation. Read at every launch: tests toggle it.
static bool scan_newton(int kind, int S) {
  if (kind != 3 || S != 2) return false;       // Newton statistics are (g, h); S is compile-time there
  const char* e = std::getenv("TMOG_SCAN_GENERIC");
  return !(e && e[0] == '1');
}

static int split_fpb() {
  static const int v = [] {
    const char* e = std::getenv("TMOG_SPLIT_FPB");
    const int x = e ? std::atoi(e) : FPB;
    return (x == 4 || x == 8 || x == 16) ? x : FPB;
  }();
  return v;
}

// Everything the per-node split reduction reads and writes (split_reduce_kernel, or the last scan block of a
// node when the reduction is fused into the scan).
struct ReduceArgs {
  const int64_t* hist;
  const int64_t* node_hist_off;
  const int32_t* node_feat_off;
  const int32_t* feat_list;
  int B, S, missing_bin;
  const int32_t* node_model;
  const double* qinv;
  int fbmax;
  int cstride;      // candidate slots per node (fbmax rounded up to 16: 384 B, whole 128-B lines per node)
  const SplitCand* cand;
  int32_t* out_feat;
  int32_t* out_bin;
  float* out_gain;
  uint8_t* out_dl;
  float* out_left;
  float* out_total;
  unsigned long long* cursors;
  uint8_t* rec;
  int64_t rec_bytes;
  int fp_mlo, fp_nml, fp_obase;
};

// One wave: node j's best candidate under the CPU twin's tie-break (gain, then lowest feature, dl, bin), the
// node totals and the winner's left statistics.
__device__ __forceinline__ void reduce_node(const ReduceArgs& ra, int j, int lane, bool sc1 = false) {
  const int B = ra.B, S = ra.S, fbmax = ra.fbmax, missing_bin = ra.missing_bin;
  if (ra.cursors && lane < 2) ra.cursors[2 * j + lane] = 0;   // partition_fused_kernel's per-node slot cursors
  SplitCand b = SplitCand::none();
  for (int i = lane; i < fbmax; i += 64) {      // any number of feature blocks
    const SplitCand* cp = ra.cand + (int64_t)j * ra.cstride + i;
    const SplitCand c = sc1 ? load_best_sc1(cp) : *cp;
    if (better(c, b)) b = c;
  }
  wave_best(b);
  const bool found = b.found() && b.gain > -INFINITY;
  const int64_t* h = ra.hist + ra.node_hist_off[j];
  const double* qi = ra.qinv + (int64_t)(ra.node_model ? ra.node_model[j] : 0) * S;
  if (lane == 0) {
    ra.out_feat[j] = found ? ra.feat_list[ra.node_feat_off[j] + b.f] : -1;
    ra.out_bin[j] = found ? b.b : -1;
    ra.out_gain[j] = found ? (float)b.gain : -INFINITY;
    ra.out_dl[j] = (uint8_t)(found ? b.dl : 0);
  }
  for (int s = 0; s < S; ++s) {
    int64_t t = 0, l = 0;
    const int64_t* hf = h + (int64_t)(found ? b.f : 0) * B * S;
    for (int bb = lane; bb < B; bb += 64) {       // any number of bins
      t += h[(int64_t)bb * S + s];
      if (found && bb <= b.b) l += hf[(int64_t)bb * S + s];
    }
    if (found && b.dl && lane == 0) l += hf[(int64_t)missing_bin * S + s];
    for (int off = 32; off > 0; off >>= 1) {
      t += __shfl_xor(t, off, 64);
      l += __shfl_xor(l, off, 64);
    }
    if (lane == 0) {
      ra.out_total[(int64_t)j * S + s] = (float)((double)t * qi[s]);
      ra.out_left[(int64_t)j * S + s] = (float)((double)l * qi[s]);
      if (ra.rec)
        reinterpret_cast<float*>(ra.rec + (int64_t)j * ra.rec_bytes + kFpLeft)[s] = (float)((double)l * qi[s]);
    }
  }
  if (ra.rec && lane == 0) {   // feature-parallel split record
    uint8_t* r = ra.rec + (int64_t)j * ra.rec_bytes;
    fp_rec_store(r, found, b, ra.fp_mlo, ra.fp_nml, ra.fp_obase,
                 [&] { return ra.feat_list[ra.node_feat_off[j] + b.f]; });
  }
}

// Per-node split evaluation state of the narrow scans (split_scan_kernel, pair_scan_kernel): node totals
// (fixed point and scaled), the node's parameters, and this thread's best candidate so far.
// NEWTON: the gain kind is 3 at compile time (XGBoost's only kind) -- the instantiation holds no impurity code
// (Gini, entropy's fp64 log2, variance), which the run-time kind inlines at every consider() site; the Newton
// expressions and their order are those of the generic instantiation's kind == 3 branch.
template <int SM, bool NEWTON = false>
struct NodeScan {
  int64_t totq[SM];
  double tot[SM], q[SM];
  double tcount, pimp, parent_gain, min_inst, min_gain, mcw, lambda;
  int S, kind;
  bool allow_missing;
  SplitCand best;

  // totq_in: the node's fixed-point totals (every lane holds the same values)
  __device__ __forceinline__ void init(const int64_t* totq_in, const double* qi, const float* P, int S_, int kind_,
                                       int missing_bin) {
    S = S_;
    kind = NEWTON ? 3 : kind_;
    best = SplitCand::none();
    min_inst = P[kPrmMinInst];
    min_gain = P[kPrmMinGain];
    mcw = P[kPrmMcw];
    lambda = P[kPrmLambda];
    allow_missing = P[kPrmAllowMissing] > 0.5f && missing_bin >= 0;
    TM_FOR_S(s) {
      totq[s] = totq_in[s];
      q[s] = qi[s];
      tot[s] = (double)totq[s] * q[s];
    }
    if constexpr (NEWTON) {
      parent_gain = newton_parent(tot[0], tot[1], lambda);
    } else {
      pimp = impurity<SM>([&](int s) { return tot[s]; }, S, kind, &tcount);
      parent_gain = kind == 3 ? newton_parent(tot[0], tot[1], lambda) : 0.0;
    }
  }

  // one candidate (left statistics lq, bin b, missing direction dl) with the CPU twin's arithmetic
  __device__ __forceinline__ void consider(const int64_t* lq, int f, int b, int dl) {
    double left[SM], right[SM];
    TM_FOR_S(s) {
      left[s] = (double)lq[s] * q[s];
      right[s] = (double)(totq[s] - lq[s]) * q[s];
    }
    double gain;
    bool ok = true;
    if (NEWTON || kind == 3) {
      // invalid by min_child_weight: skip the two fp64 divisions (whole waves skip at small nodes)
      if (newton_invalid(left[1], right[1], mcw)) return;
      gain = newton_gain(left[0], left[1], right[0], right[1], lambda, parent_gain);
    } else if constexpr (!NEWTON) {
      double lc, rc;
      const double li = impurity<SM>([&](int s) { return left[s]; }, S, kind, &lc);
      const double ri = impurity<SM>([&](int s) { return right[s]; }, S, kind, &rc);
      ok = impurity_split_gain(pimp, tcount, lc, li, rc, ri, min_inst, min_gain, &gain);
    }
    if (ok) {
      SplitCand c{gain, f, b, dl};
      if (better(c, best)) best = c;
    }
  }

  // multi-bin feature f: lane = bin, v = this lane's bin statistics (0 past nb), miss = the missing bin's
  // (same on every lane). Exact int64 wave prefix sum, then the lane's (bin, dl) candidates.
  __device__ __forceinline__ void scan_feature(int64_t* v, const int64_t* miss, int nb, int f, int lane) {
    TM_FOR_S(s) v[s] = wave_scan64(v[s]);
    // candidates b < nb - 1; with a missing bin dl = 0 also b = nb - 1 (present left, missing right).
    // An empty missing bin makes every dl = 1 candidate equal to its dl = 0 twin, which wins the tie
    // (better(): dl ascending; the CPU twin's first-wins scan order) -- skip them.
    bool any_miss = false;
    TM_FOR_S(s) any_miss |= miss[s] != 0;
    const int n_dl = allow_missing ? (any_miss ? 2 : 1) : 1;
    if (lane < nb - 1 + (allow_missing ? 1 : 0)) {
      for (int dl = 0; dl < n_dl; ++dl) {
        if (lane == nb - 1 && dl) continue;
        int64_t lq[SM];
        TM_FOR_S(s) lq[s] = v[s] + (dl ? miss[s] : 0);
        consider(lq, f, lane, dl);
      }
    }
  }

};

// node totals from local feature 0 of a histogram (every row is counted once per feature, including the
// missing bin), on every lane of the wave
template <int SM>
__device__ __forceinline__ void node_totals(const int64_t* h, int B, int S, int lane, int64_t* totq) {
  int64_t v[SM];
  TM_FOR_S(s) v[s] = lane < B ? h[lane * S + s] : 0;     // all loads before the reductions
  TM_FOR_S(s) totq[s] = readlane64(wave_scan64(v[s]), 63);
}

// The row of feature f that a lane of the narrow scans reads: its own bin's (bin 0 past the B bins, so every
// load is unconditional). The Newton instantiations issue these one feature ahead of the scan that uses them.
template <int SM>
__device__ __forceinline__ void load_row(const int64_t* __restrict__ h, int f, int B, int S, int lane, int64_t* v) {
  const int64_t o = (int64_t)f * B * S + (lane < B ? lane : 0) * S;
  TM_FOR_S(s) v[s] = h[o + s];
}

// End of a batch of independent wave-uniform loads: they are all issued above this point and their values
// (scalar registers) are complete below it, whatever uses them first.
template <class T>
__device__ __forceinline__ void pin_scalar(T& v) {
  asm volatile("" : "+s"(v));
}
template <class... T>
__device__ __forceinline__ void batch_end(T&... v) {
  __builtin_amdgcn_sched_barrier(0);
  (pin_scalar(v), ...);
}

// node_totals from the lane's row of local feature 0 (load_row), already loaded
template <int SM>
__device__ __forceinline__ void row_totals(const int64_t* row, int B, int S, int lane, int64_t* totq) {
  TM_FOR_S(s) totq[s] = readlane64(wave_scan64(lane < B ? row[s] : 0), 63);
}

// NEWTON: compile-time gain kind 3 (NodeScan) and a software-pipelined feature loop -- the rows of the wave's next
// feature are in flight while it scans the current one. The generic instantiation keeps the run-time kind and the
// load -> wait -> scan loop (TMOG_SCAN_GENERIC=1 selects it for kind 3 too: the reference of the Newton one).
template <int SM, bool NEWTON>
__global__ void __launch_bounds__(256) split_scan_kernel(
    const int64_t* __restrict__ hist, const int64_t* __restrict__ node_hist_off, const int32_t* __restrict__ node_nfeat,
    const int32_t* __restrict__ node_feat_off, const int32_t* __restrict__ feat_list,
    const int32_t* __restrict__ feat_nbins, int B, int S, int kind, const float* __restrict__ node_params,
    int missing_bin, const int32_t* __restrict__ node_model, const double* __restrict__ qinv, int fbmax,
    SplitCand* __restrict__ cand, int n_multi, int fpb, unsigned* __restrict__ done, ReduceArgs ra,
    const int* __restrict__ dm) {
  const int cstride = ra.cstride;
  if constexpr (NEWTON) S = SM;      // the launcher takes this instantiation at S == SM only: no run-time S guards
  const int j = blockIdx.x / fbmax;
  const int fb = blockIdx.x - j * fbmax;
  if (dm != nullptr && j >= *dm) return;      // device-planned level: node count on the device
  const int lane = threadIdx.x & 63;
  // NEWTON: the wave index as a scalar, so the feature index, its bin count and row offset are too
  const int wave = NEWTON ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : (int)(threadIdx.x >> 6);
  // paired slot: the node was scanned with its subtraction partner by pair_scan_kernel (same cand slots, all
  // written by that earlier launch): with the fused reduction its block 0 reduces it, the others have nothing to do
  if (node_params[(int64_t)j * kPrmStride + kPrmPaired] > 0.5f) {
    if (done && fb == 0 && wave == 0) reduce_node(ra, j, lane);
    return;
  }
  const int nf = node_nfeat[j];
  // n_multi >= 0: local features [n_multi, nf) have one present bin; their blocks (fb >= fb_multi)
  // take 256 features each, one thread per feature, instead of 16 per block through the scan
  const int f_lim = n_multi >= 0 ? min(n_multi, nf) : nf;
  const int fb_multi = n_multi >= 0 ? (n_multi + fpb - 1) / fpb : fbmax;
  const bool one_blk = fb >= fb_multi;
  __shared__ SplitCand s_best[4];
  NodeScan<SM, NEWTON> ns;
  ns.best = SplitCand::none();
  // "may split" slot (tree_grow.hpp): nodes built only as a subtraction partner are not scanned
  if (node_params[(int64_t)j * kPrmStride + kPrmMaySplit] > 0.5f &&
      (one_blk ? (n_multi + (fb - fb_multi) * 256 < nf) : (fb * fpb < f_lim))) {
    const int64_t* h = hist + node_hist_off[j];
    const int32_t* fl = feat_list + node_feat_off[j];
    const int f_end = one_blk ? 0 : min(f_lim, (fb + 1) * fpb);
    const int mbin = missing_bin >= 0 ? missing_bin : 0;
    // NEWTON: the next feature's bin count, own-bin row and missing-bin row, issued a feature ahead -- the first
    // feature's here, with the node totals' rows, the following one's before each scan
    [[maybe_unused]] int64_t nv[SM], nm[SM];
    [[maybe_unused]] int nb_next = 0;
    [[maybe_unused]] auto issue = [&](int f) {
      load_row<SM>(h, f, B, S, lane, nv);
      const int64_t* hf = h + (int64_t)f * B * S;
      TM_FOR_S(s) nm[s] = hf[mbin * S + s];
      nb_next = feat_nbins[fl[f]];
    };
    int64_t totq[SM];
    if constexpr (NEWTON) {
      int64_t r0[SM];
      load_row<SM>(h, 0, B, S, lane, r0);
      if (fb * fpb + wave < f_end) issue(fb * fpb + wave);
      __builtin_amdgcn_sched_barrier(0);
      row_totals<SM>(r0, B, S, lane, totq);
    } else {
      node_totals<SM>(h, B, S, lane, totq);
    }
    ns.init(totq, qinv + (int64_t)(node_model ? node_model[j] : 0) * S, node_params + (int64_t)j * kPrmStride, S,
            kind, missing_bin);
    if (one_blk) {
      const int f = n_multi + (fb - fb_multi) * 256 + (int)threadIdx.x;
      if (f < nf && ns.allow_missing && feat_nbins[fl[f]] == 1) {
        const int64_t* hf = h + (int64_t)f * B * S;
        int64_t lq[SM];
        TM_FOR_S(s) lq[s] = hf[s];
        ns.consider(lq, f, 0, 0);
      }
    }
    if constexpr (NEWTON) {
      for (int f = fb * fpb + wave; f < f_end; f += 4) {
        int64_t v[SM], miss[SM];
        const int nb = nb_next;
        TM_FOR_S(s) {
          v[s] = nv[s];
          miss[s] = nm[s];
        }
        if (f + 4 < f_end) issue(f + 4);
        __builtin_amdgcn_sched_barrier(0);      // the next feature's loads stay ahead of this one's scan
        if (nb == 1) {       // one present bin: lane 0 holds bin 0 (see the generic loop)
          if (ns.allow_missing && lane == 0) ns.consider(v, f, 0, 0);
          continue;
        }
        TM_FOR_S(s) {
          v[s] = lane < nb ? v[s] : 0;
          miss[s] = ns.allow_missing ? miss[s] : 0;
        }
        ns.scan_feature(v, miss, nb, f, lane);
      }
    } else {
      for (int f = fb * fpb + wave; f < f_end; f += 4) {
        const int nb = feat_nbins[fl[f]];
        const int64_t* hf = h + (int64_t)f * B * S;
        if (nb == 1) {
          // one present bin (one-hot / null indicator): the only candidate is present-left,
          // missing-right -- no scan, one lane
          if (ns.allow_missing && lane == 0) {
            int64_t lq[SM];
            TM_FOR_S(s) lq[s] = hf[s];
            ns.consider(lq, f, 0, 0);
          }
          continue;
        }
        int64_t v[SM], miss[SM];
        const int bl = lane < nb ? lane : 0;
        TM_FOR_S(s) {          // unconditional loads, selected afterwards (issued together)
          v[s] = hf[bl * S + s];
          miss[s] = hf[mbin * S + s];
        }
        TM_FOR_S(s) {
          v[s] = lane < nb ? v[s] : 0;
          miss[s] = ns.allow_missing ? miss[s] : 0;
        }
        ns.scan_feature(v, miss, nb, f, lane);
      }
    }
  }
  wave_best(ns.best);
  if (lane == 0) s_best[wave] = ns.best;
  __syncthreads();
  if (done == nullptr) {
    if (threadIdx.x == 0) {
      SplitCand b = s_best[0];
      for (int w = 1; w < 4; ++w)
        if (better(s_best[w], b)) b = s_best[w];
      cand[(int64_t)j * cstride + fb] = b;
    }
    return;
  }
  // Fused reduction: the last of the node's fbmax blocks to finish reduces it -- one launch per level fewer.
  // Hand-off (MI355X_MICROARCH.md, inter-workgroup visibility, first row of the sc1 table): the candidate
  // goes out as agent-scope (sc1) stores by wave 0, which waits for them (vmcnt(0)) before its agent-scope
  // ticket add; the block whose add returns fbmax - 1 reads every candidate of the node with sc1 loads in
  // that same wave. No L2 write-back / L1 invalidate fences.
  // HARDWARE ASSUMPTION (not a HIP memory-model guarantee -- every access here is relaxed): on gfx950 an
  // sc1 store is written through to the coherence point before vmcnt reaches 0, an sc1 load is served from
  // it, and the reader's loads cannot be hoisted above the ticket add (they are issued after the wave-uniform
  // branch on its result, and the atomics are volatile to the compiler). The portable form -- release on
  // the ticket add, an agent-scope acquire fence in the winning block -- costs an L2 write-back per node on
  // this part (agent scope spans the 8 XCDs' L2s). TMOG_FUSED_REDUCE=0 selects the separate reduce launch;
  // tests/test_gpu_kernels.py checks the two paths give identical trees over many nodes and levels.
  if (wave == 0) {
    unsigned last = 0;
    if (lane == 0) {
      SplitCand b = s_best[0];
      for (int w = 1; w < 4; ++w)
        if (better(s_best[w], b)) b = s_best[w];
      store_best_sc1(cand + (int64_t)j * cstride + fb, b);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the sc1 stores have left before the ticket
      last = __hip_atomic_fetch_add(done + j, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
             (unsigned)(fbmax - 1);
    }
    last = __shfl(last, 0, 64);
    if (last) {
      reduce_node(ra, j, lane, true);
      if (lane == 0) __hip_atomic_store(done + j, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Subtraction + split scan of a sibling pair in one pass (replaces hist_subtract_kernel + the two nodes'
// split_scan blocks). Block (q, fb) covers feature block fb of pair q exactly as split_scan_kernel does for
// one node: it loads the parent's and the built (small) child's rows, stores big = parent - small, and
// scans both children from registers -- the histograms the subtraction already streams are not read
// again by a separate scan. Node totals: small from its feature 0, big = parent's - small's. Writes
// cand[j_small][fb] and cand[j_big][fb]; the two nodes carry the paired slot so split_scan_kernel skips
// them. Words outside the live set (one-present-bin columns above bin 0) are left alone, as before.
// Load schedule. The kernel is bound by exposed load latency, not by VALU issue or bandwidth (profiles/README.md):
// a wave runs a chain of dependent loads (pair -> node offsets -> rows) and then up to four features of ~400
// VALU instructions each. The generic instantiation (run-time kind) waits for each feature's rows right before
// scanning them. The NEWTON instantiation (kind 3 at compile time, no impurity code: fewer registers, more
// resident waves) keeps one feature in flight: the first feature's rows and bin count are issued with the node
// totals' rows as soon as the node offsets are known, and each feature's successor is issued before the current
// one is scanned (the sched_barrier keeps the compiler from sinking those loads). The current rows are complete
// before the successor's loads go out, the big child's stores follow them in program order, and the next wait
// on the vector memory counter stands after the scan: no store drains the prefetch.
// The wave index is a scalar there, so feature index, bin count and row base live in SGPRs.
template <int SM, bool NEWTON>
__global__ void __launch_bounds__(256) pair_scan_kernel(
    int64_t* __restrict__ hist, const int64_t* __restrict__ parent, const int64_t* __restrict__ parent_off,
    const int32_t* __restrict__ small_j, const int32_t* __restrict__ big_j, int n_pairs,
    const int64_t* __restrict__ node_hist_off, const int32_t* __restrict__ node_nfeat,
    const int32_t* __restrict__ node_feat_off, const int32_t* __restrict__ feat_list,
    const int32_t* __restrict__ feat_nbins, int B, int S, int kind, const float* __restrict__ node_params,
    int missing_bin, const int32_t* __restrict__ node_model, const double* __restrict__ qinv, int fbmax,
    SplitCand* __restrict__ cand, int n_multi, int fpb, int cstride, const int* __restrict__ dnp) {
  if constexpr (NEWTON) S = SM;      // the launcher takes this instantiation at S == SM only: no run-time S guards
  const int q = blockIdx.x / fbmax;
  const int fb = blockIdx.x - q * fbmax;
  if (dnp != nullptr) n_pairs = *dnp;          // device-planned level: pair count on the device
  if (q >= n_pairs) return;
  const int lane = threadIdx.x & 63;
  const int wave = NEWTON ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : (int)(threadIdx.x >> 6);
  // NEWTON: the dependent loads of the prologue go out in three batches (batch_end(): the compiler otherwise
  // issues them one by one, each waited for before the next): the pair; the two nodes' offsets and "may split"
  // flags; the node totals' rows with the first feature's. The nodes' models, which only the scales need, are
  // read behind the third.
  int js = small_j[q], jb = big_j[q];
  int64_t poff = parent_off[q];
  if constexpr (NEWTON) batch_end(js, jb, poff);
  int nf = node_nfeat[js];                 // no per-node feature subsets on this path: same list for both
  int64_t hs_off = node_hist_off[js], hb_off = node_hist_off[jb];
  int fl_off = node_feat_off[js];
  float may_s = node_params[(int64_t)js * kPrmStride + kPrmMaySplit];
  float may_b = node_params[(int64_t)jb * kPrmStride + kPrmMaySplit];
  if constexpr (NEWTON) batch_end(nf, hs_off, hb_off, fl_off, may_s, may_b);
  const int64_t* P = parent + poff;
  const int64_t* Hs = hist + hs_off;
  int64_t* Hb = hist + hb_off;
  const int32_t* fl = feat_list + fl_off;
  const bool scan_s = may_s > 0.5f, scan_b = may_b > 0.5f;
  const int f_lim = n_multi >= 0 ? min(n_multi, nf) : nf;
  const int fb_multi = n_multi >= 0 ? (n_multi + fpb - 1) / fpb : fbmax;
  const bool one_blk = fb >= fb_multi;
  const int f_end = one_blk ? 0 : min(f_lim, (fb + 1) * fpb);
  // NEWTON: the next feature's bin count and this lane's rows of the built child and the parent, in flight
  [[maybe_unused]] int64_t na[SM], np_[SM];
  [[maybe_unused]] int nb_next = 0;
  [[maybe_unused]] auto issue = [&](int f) {
    load_row<SM>(Hs, f, B, S, lane, na);
    load_row<SM>(P, f, B, S, lane, np_);
    nb_next = feat_nbins[fl[f]];
  };
  __shared__ SplitCand s_best[2][4];
  NodeScan<SM, NEWTON> ns, nb_;
  {
    int64_t ts[SM], tp[SM], tb[SM];
    if constexpr (NEWTON) {
      int64_t rs[SM], rp[SM];
      load_row<SM>(Hs, 0, B, S, lane, rs);
      load_row<SM>(P, 0, B, S, lane, rp);
      if (fb * fpb + wave < f_end) issue(fb * fpb + wave);
      __builtin_amdgcn_sched_barrier(0);
      row_totals<SM>(rs, B, S, lane, ts);
      row_totals<SM>(rp, B, S, lane, tp);
    } else {
      node_totals<SM>(Hs, B, S, lane, ts);
      node_totals<SM>(P, B, S, lane, tp);
    }
    TM_FOR_S(s) tb[s] = tp[s] - ts[s];
    const int model_s = node_model ? node_model[js] : 0, model_b = node_model ? node_model[jb] : 0;
    ns.init(ts, qinv + (int64_t)model_s * S, node_params + (int64_t)js * kPrmStride, S, kind, missing_bin);
    nb_.init(tb, qinv + (int64_t)model_b * S, node_params + (int64_t)jb * kPrmStride, S, kind, missing_bin);
  }
  // feature f from this lane's rows pa (built child) and pp (parent): the big child's row out, both scans
  auto scan_pair = [&](int f, int nbins, const int64_t* pa, const int64_t* pp) {
    const int64_t o = (int64_t)f * B * S;
    int64_t vs[SM], vb[SM], ms[SM], mb[SM];
    TM_FOR_S(s) {
      const int64_t a = lane < B ? pa[s] : 0;
      const int64_t c = lane < B ? pp[s] - pa[s] : 0;
      if (lane < B) Hb[o + lane * S + s] = c;
      // missing bin statistics from the lane holding it
      ms[s] = missing_bin >= 0 ? readlane64(a, missing_bin) : 0;   // kernel argument: wave-uniform lane
      mb[s] = missing_bin >= 0 ? readlane64(c, missing_bin) : 0;
      vs[s] = lane < nbins ? a : 0;
      vb[s] = lane < nbins ? c : 0;
    }
    if (nbins == 1) {
      if (lane == 0) {
        if (scan_s && ns.allow_missing) ns.consider(vs, f, 0, 0);
        if (scan_b && nb_.allow_missing) nb_.consider(vb, f, 0, 0);
      }
      return;
    }
    if (scan_s) {
      if (!ns.allow_missing)
        TM_FOR_S(s) ms[s] = 0;
      ns.scan_feature(vs, ms, nbins, f, lane);
    }
    if (scan_b) {
      if (!nb_.allow_missing)
        TM_FOR_S(s) mb[s] = 0;
      nb_.scan_feature(vb, mb, nbins, f, lane);
    }
  };
  if (one_blk) {
    const int f = n_multi + (fb - fb_multi) * 256 + (int)threadIdx.x;
    if (f < nf) {
      const int64_t o = (int64_t)f * B * S;      // live words of a one-present-bin column: bin 0
      int64_t ls[SM], lb[SM];
      TM_FOR_S(s) {
        ls[s] = Hs[o + s];
        lb[s] = P[o + s] - ls[s];
        Hb[o + s] = lb[s];
      }
      if (feat_nbins[fl[f]] == 1) {
        if (scan_s && ns.allow_missing) ns.consider(ls, f, 0, 0);
        if (scan_b && nb_.allow_missing) nb_.consider(lb, f, 0, 0);
      }
    }
  } else if constexpr (NEWTON) {
    for (int f = fb * fpb + wave; f < f_end; f += 4) {
      int64_t pa[SM], pp[SM];
      const int nbins = nb_next;
      TM_FOR_S(s) {
        pa[s] = na[s];
        pp[s] = np_[s];
      }
      if (f + 4 < f_end) issue(f + 4);
      __builtin_amdgcn_sched_barrier(0);      // the next feature's loads stay ahead of this one's stores and scan
      scan_pair(f, nbins, pa, pp);
    }
  } else {
    for (int f = fb * fpb + wave; f < f_end; f += 4) {
      const int nbins = feat_nbins[fl[f]];
      int64_t pa[SM], pp[SM];
      load_row<SM>(Hs, f, B, S, lane, pa);           // every load unconditional (issued together)
      load_row<SM>(P, f, B, S, lane, pp);
      scan_pair(f, nbins, pa, pp);
    }
  }
  wave_best(ns.best);
  wave_best(nb_.best);
  if (lane == 0) {
    s_best[0][wave] = ns.best;
    s_best[1][wave] = nb_.best;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    SplitCand b = s_best[threadIdx.x][0];
    for (int w = 1; w < 4; ++w)
      if (better(s_best[threadIdx.x][w], b)) b = s_best[threadIdx.x][w];
    cand[(int64_t)(threadIdx.x ? jb : js) * cstride + fb] = b;
  }
}

// Wide split scan (S > 16 classes or B > 64 bins): one workgroup per (node, local feature). The
// feature's B x S fixed-point histogram is copied into LDS and prefix-summed over bins per statistic
// (one thread per statistic), node totals come from local feature 0 as in the narrow kernel, then the
// threads stride over the (bin, missing direction) candidates and evaluate each with exactly the CPU
// twin's operation order (impurity sums over s in order), so both paths pick the same split.
__global__ void __launch_bounds__(256) split_scan_wide_kernel(
    const int64_t* __restrict__ hist, const int64_t* __restrict__ node_hist_off, const int32_t* __restrict__ node_nfeat,
    const int32_t* __restrict__ node_feat_off, const int32_t* __restrict__ feat_list,
    const int32_t* __restrict__ feat_nbins, int B, int S, int kind, const float* __restrict__ node_params,
    int missing_bin, const int32_t* __restrict__ node_model, const double* __restrict__ qinv, int fbmax,
    SplitCand* __restrict__ cand, int n_multi, int cstride) {
  extern __shared__ __attribute__((aligned(16))) int64_t wl[];
  int64_t* H = wl;                       // [B][S] prefix sums
  int64_t* totq = H + (int64_t)B * S;    // [S]
  int64_t* miss = totq + S;              // [S]
  double* q = reinterpret_cast<double*>(miss + S);   // [S]
  __shared__ SplitCand s_best[4];
  const int j = blockIdx.x / fbmax;
  const int f = blockIdx.x - j * fbmax;
  const int nf = node_nfeat[j];
  SplitCand best = SplitCand::none();
  const float* P = node_params + (int64_t)j * kPrmStride;
  const bool live = f < nf && P[kPrmMaySplit] > 0.5f;
  const int64_t* h = hist + node_hist_off[j];
  const int32_t* fl = feat_list + node_feat_off[j];
  const double* qi = qinv + (int64_t)(node_model ? node_model[j] : 0) * S;
  const double min_inst = P[kPrmMinInst], min_gain = P[kPrmMinGain], mcw = P[kPrmMcw], lambda = P[kPrmLambda];
  const bool allow_missing = P[kPrmAllowMissing] > 0.5f && missing_bin >= 0;
  const int nb = live ? feat_nbins[fl[f]] : 0;
  const bool one = live && n_multi >= 0 && f >= n_multi;     // one-present-bin column: bin 0 only
  const int64_t* hf = h + (int64_t)f * B * S;
  if (live) {
    for (int i = threadIdx.x; i < B * S; i += blockDim.x) H[i] = (one && i >= S) ? 0 : hf[i];
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
      int64_t t = 0;
      for (int bb = 0; bb < B; ++bb) t += h[(int64_t)bb * S + s];
      totq[s] = t;
      miss[s] = allow_missing ? hf[(int64_t)missing_bin * S + s] : 0;
      q[s] = qi[s];
    }
  }
  __syncthreads();
  if (live)
    for (int s = threadIdx.x; s < S; s += blockDim.x)
      for (int bb = 1; bb < B; ++bb) H[(int64_t)bb * S + s] += H[(int64_t)(bb - 1) * S + s];
  __syncthreads();
  if (live) {
    // the CPU twin's arithmetic over the scaled LDS sums (the integer expressions in its operation order)
    auto tot = [&](int s) { return (double)totq[s] * q[s]; };
    double tcount = 0;
    const double pimp = impurity<0>(tot, S, kind, &tcount);
    const double parent_gain = kind == 3 ? newton_parent(tot(0), tot(1), lambda) : 0.0;
    const int nd = allow_missing ? 2 : 1;
    const int nbc = one ? 1 : nb - 1 + (allow_missing ? 1 : 0);   // candidate bins per direction
    for (int c = threadIdx.x; c < nbc * nd; c += blockDim.x) {
      const int dl = c / nbc, b = one ? 0 : c - dl * nbc;
      if (one && (dl || !allow_missing)) continue;
      if (!one && b == nb - 1 && dl) continue;
      const int64_t* lp = H + (int64_t)b * S;
      auto left = [&](int s) { return (double)(lp[s] + (dl ? miss[s] : 0)) * q[s]; };
      auto right = [&](int s) { return (double)(totq[s] - lp[s] - (dl ? miss[s] : 0)) * q[s]; };
      double gain;
      bool ok;
      if (kind == 3) {
        ok = !newton_invalid(left(1), right(1), mcw);
        gain = newton_gain(left(0), left(1), right(0), right(1), lambda, parent_gain);
      } else {
        double lc, rc;
        const double li = impurity<0>(left, S, kind, &lc);
        const double ri = impurity<0>(right, S, kind, &rc);
        ok = impurity_split_gain(pimp, tcount, lc, li, rc, ri, min_inst, min_gain, &gain);
      }
      if (ok) {
        const SplitCand cb{gain, f, b, dl};
        if (better(cb, best)) best = cb;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wave_best(best);
  if (lane == 0) s_best[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    SplitCand bb = s_best[0];
    for (int w = 1; w < 4; ++w)
      if (better(s_best[w], bb)) bb = s_best[w];
    cand[(int64_t)j * cstride + f] = bb;
  }
}

__global__ void __launch_bounds__(64) split_reduce_kernel(ReduceArgs ra) { reduce_node(ra, blockIdx.x, threadIdx.x); }

// Feature-parallel merge: node j's decision is the best of the R ranks' records under the split scan's
// order (gain, then lowest full-list position, dl, bin) -- the candidate a single rank scanning every
// feature would pick (fp_merge_node, shared with common/tree_grow.hpp fp_merge_host).
// m_stride: records per rank in recv (the all-gather's count; >= m); dm (device-planned levels): the real node count
// is read from device memory, the grid covers the host bound m.
__global__ void fp_merge_kernel(const uint8_t* __restrict__ recv, int R, int m, int64_t rb, int S,
                                int32_t* __restrict__ out_feat, int32_t* __restrict__ out_bin,
                                float* __restrict__ out_gain, uint8_t* __restrict__ out_dl,
                                float* __restrict__ out_left, int64_t m_stride, const int* __restrict__ dm) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m || (dm != nullptr && j >= *dm)) return;
  fp_merge_node(recv, R, m_stride, j, rb, S, out_feat, out_bin, out_gain, out_dl, out_left);
}

// Launch arithmetic of the scans, written once. Wide: split_scan_wide_kernel, one workgroup per (node, feature).
inline bool scan_is_wide(int B, int S) { return S > TM_MAX_S || B > 64; }
// Feature blocks per node of the narrow scans: fpb features each, and with n_multi >= 0 the one-present-bin
// features [n_multi, max_nfeat) 256 each. An n_multi split adds at most one block to the unsplit count
// (fpb <= 16 < 256), which is how tmog_hip_split_cand_bytes bounds it without knowing n_multi.
inline int scan_fbmax(int n_multi, int max_nfeat, int fpb) {
  return n_multi >= 0 ? (n_multi + fpb - 1) / fpb + (max_nfeat - n_multi + 255) / 256 : (max_nfeat + fpb - 1) / fpb;
}
// The narrow scans' instantiation for S statistics; LAUNCH takes the template arguments <SM, NEWTON>.
#define TM_SCAN_LADDER(LAUNCH)               \
  if (scan_newton(kind, S)) LAUNCH(2, true); \
  else if (S <= 2) LAUNCH(2, false);         \
  else if (S == 3) LAUNCH(3, false);         \
  else if (S <= 4) LAUNCH(4, false);         \
  else LAUNCH(TM_MAX_S, false)

}  // namespace

int tmog::prime_tree_split() { return prime_kernel(&split_reduce_kernel); }

// ------------------------------------------------------------------------------------- C ABI
extern "C" {

int tmog_hip_split_find(const int64_t* hist, int n_nodes, const int64_t* node_hist_off, const int32_t* node_nfeat,
                        const int32_t* node_feat_off, const int32_t* feat_list, const int32_t* feat_nbins, int B,
                        int S, int kind, const float* node_params, int missing_bin, const int32_t* node_model,
                        const double* qinv, int max_nfeat, void* cand_ws, int32_t* out_feat, int32_t* out_bin,
                        float* out_gain, uint8_t* out_dl, float* out_left, float* out_total, int64_t* cursors,
                        int n_multi, void* rec, int64_t rec_bytes, int fp_mlo, int fp_nml, int fp_obase,
                        hipStream_t stream, unsigned* done, const int* dm) {
  if (n_nodes == 0) return 0;
  const bool wide = scan_is_wide(B, S);
  // device-counted launches take the narrow scan with the fused reduction (no separate per-node launch)
  if (dm != nullptr && (done == nullptr || wide)) return -2;
  if (n_multi > max_nfeat) n_multi = -1;
  if (wide && (S > TM_WIDE_MAX_S || B * S > TM_WIDE_MAX_BS)) return -2;
  SplitCand* cand = (SplitCand*)cand_ws;   // >= tmog_hip_split_cand_bytes(n_nodes, max_nfeat, B, S) bytes
  const int fpb = wide ? 0 : split_fpb();
  const int fbmax = wide ? max_nfeat : scan_fbmax(n_multi, max_nfeat, fpb);   // wide: a workgroup per (node, feature)
  // done (n_nodes zeroed counters, left zeroed): the node reduction runs inside the narrow scan's last block
  const ReduceArgs ra{hist, node_hist_off, node_feat_off, feat_list, B, S, missing_bin, node_model, qinv, fbmax,
                      cand_stride(fbmax), cand, out_feat, out_bin, out_gain, out_dl, out_left, out_total,
                      (unsigned long long*)cursors, (uint8_t*)rec, rec_bytes, fp_mlo, fp_nml, fp_obase};
  if (wide) {
    const size_t lds = ((size_t)B * S + 3 * (size_t)S) * 8;
    hipLaunchKernelGGL(split_scan_wide_kernel, dim3(n_nodes * fbmax), dim3(256), lds, stream, hist, node_hist_off,
                       node_nfeat, node_feat_off, feat_list, feat_nbins, B, S, kind, node_params, missing_bin,
                       node_model, qinv, fbmax, cand, n_multi, cand_stride(fbmax));
  } else {
#define TM_SPLIT(...)                                                                                          \
  hipLaunchKernelGGL((split_scan_kernel<__VA_ARGS__>), dim3(n_nodes * fbmax), dim3(256), 0, stream, hist, node_hist_off,  \
                     node_nfeat, node_feat_off, feat_list, feat_nbins, B, S, kind, node_params, missing_bin,    \
                     node_model, qinv, fbmax, cand, n_multi, fpb, done, ra, dm)
    TM_SCAN_LADDER(TM_SPLIT);
#undef TM_SPLIT
  }
  if (wide || done == nullptr)
    hipLaunchKernelGGL(split_reduce_kernel, dim3(n_nodes), dim3(64), 0, stream, ra);
  return (int)hipGetLastError();
}

// Fused subtraction + split scan of sibling pairs (pair_scan_kernel); the same candidate layout as
// tmog_hip_split_find, whose scan then skips the pairs' nodes (the paired slot). Narrow path only.
int tmog_hip_pair_scan(int64_t* hist, const int64_t* parent, const int64_t* parent_off, const int32_t* small_j,
                       const int32_t* big_j, int n_pairs, const int64_t* node_hist_off, const int32_t* node_nfeat,
                       const int32_t* node_feat_off, const int32_t* feat_list, const int32_t* feat_nbins, int B, int S,
                       int kind, const float* node_params, int missing_bin, const int32_t* node_model,
                       const double* qinv, int max_nfeat, void* cand_ws, int n_multi, hipStream_t stream,
                       const int* dnp) {
  if (n_pairs == 0) return 0;
  if (scan_is_wide(B, S)) return -2;
  if (n_multi > max_nfeat) n_multi = -1;
  const int fpb = split_fpb();
  const int fbmax = scan_fbmax(n_multi, max_nfeat, fpb);
#define TM_PAIR(...)                                                                                           \
  hipLaunchKernelGGL((pair_scan_kernel<__VA_ARGS__>), dim3(n_pairs * fbmax), dim3(256), 0, stream, hist, parent, parent_off, \
                     small_j, big_j, n_pairs, node_hist_off, node_nfeat, node_feat_off, feat_list, feat_nbins, B, S, \
                     kind, node_params, missing_bin, node_model, qinv, fbmax, (SplitCand*)cand_ws, n_multi, fpb,    \
                     cand_stride(fbmax), dnp)
  TM_SCAN_LADDER(TM_PAIR);
#undef TM_PAIR
  return (int)hipGetLastError();
}

// recv holds m_stride records per rank, the merged nodes are the first *dm of them (device-planned levels: m_stride is
// the level's host bound) or, with dm null, all m_stride.
int tmog_hip_fp_merge(const void* recv, int R, int m, int64_t rec_bytes, int S, int32_t* out_feat, int32_t* out_bin,
                      float* out_gain, uint8_t* out_dl, float* out_left, hipStream_t stream) {
  return tmog_hip_fp_merge_dev(recv, R, m, rec_bytes, S, out_feat, out_bin, out_gain, out_dl, out_left, nullptr, stream);
}

int tmog_hip_fp_merge_dev(const void* recv, int R, int m_stride, int64_t rec_bytes, int S, int32_t* out_feat,
                          int32_t* out_bin, float* out_gain, uint8_t* out_dl, float* out_left, const int* dm,
                          hipStream_t stream) {
  if (m_stride == 0) return 0;
  hipLaunchKernelGGL(fp_merge_kernel, dim3((m_stride + 255) / 256), dim3(256), 0, stream, (const uint8_t*)recv, R,
                     m_stride, rec_bytes, S, out_feat, out_bin, out_gain, out_dl, out_left, (int64_t)m_stride, dm);
  return (int)hipGetLastError();
}

size_t tmog_hip_split_cand_bytes(int n_nodes, int max_nfeat, int B, int S) {
  const int fpb = split_fpb();       // scan_fbmax without a split, + 1: its bound for any n_multi
  const int fbmax = scan_is_wide(B, S) ? max_nfeat : scan_fbmax(-1, max_nfeat, fpb) + 1;
  return (size_t)n_nodes * cand_stride(fbmax) * sizeof(SplitCand);
}

}  // extern "C"
