// Histogram tree engine kernels for CDNA4 (gfx950): the histogram part. Split finding is in
// tree_split_kernels.hip, partition and leaf collection in tree_partition_kernels.hip, forest scoring in
// forest_predict_kernels.hip; tree_dev.hpp holds what they share.
//
// Replaces the per-level statistics aggregation of Spark MLlib trees (DTStatsAggregator, used by
// OpRandomForestClassifier.scala:59-154 / OpGBTClassifier.scala:47-142 / DT) and XGBoost4J's
// hist updater (OpXGBoostClassifier.scala:47-403): SURVEY.md kernels K23 (histogram, split scan,
// partition), K24/K25 (GBT / Newton stats) and K29 (ensemble traversal).
//
// Layout contract (identical to ../host/tree_cpu.cpp, orchestrated by models/tree_engine.py):
//   Xb    uint8 [N][F] row-major bins          rows  uint32 (row | weight<<24)
//   hist  int64 fixed point, node j at node_hist_off[j], index ((fl * B) + bin) * S + s;
//         value = hist * qinv[model][s] (see "Fixed-point statistics" below)
//
// Histogram kernel mapping (wave64-first): a wave-instruction covers R = 64 / FG rows x FG
// features -- lane (r, f) handles feature f of row r, so lanes of one instruction touch distinct LDS
// histogram rows (feature-major, padded by one word so bank = f + bin*S + s spreads). All waves of
// the workgroup share the table through integer LDS atomics; the R copies are folded on the way out
// and a node covered by one row-chunk stores with plain stores, otherwise 64-bit integer atomics.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <stdint.h>
#include <math.h>

#include "common/tree_rules.hpp"
#include "hip/tmog_hip_abi.h"
#include "hip/tree_dev.hpp"

namespace {

using namespace tmog;   // common/tree_rules.hpp: the split / growth rules shared with the CPU twin

// (Histogram work items: HistItem, common/tmog_abi.h.)
//
// Fixed-point statistics. Every per-row contribution is quantised to an integer,
//   q = rint(v * qscale[model][s]),  |q| <= qmax = (2^31 - 1) / chunk_rows - 1,
// with power-of-two scales chosen on the device from the per-model max |v| (tree_engine._quant_scales).
// Workgroup LDS partials are int32 (ds_add_u32: ~17x the throughput of ds_add_f32 on gfx950, see
// benchmarks/lds_atomic_bench.hip) and cannot overflow for a chunk of <= chunk_rows rows; the
// global histogram is int64, so sums, the subtraction trick and the split scan's prefix sums are
// exact and order-independent -- GPU and CPU (../host/tree_cpu.cpp) histograms are bit-identical and
// runs are deterministic. Class counts (MODE 0) and the variance count are integer weights (scale 1).
//
// Staged row record (entry bits, q0, q1, q2):
//   MODE 0 (class counts):   q0 = w, q1 = class
//   MODE 1 (variance stats): q0 = w, q1 = q(w*t), q2 = q(w*t*t)
//   MODE 2 (grad / hess):    q0 = q(w*g), q1 = q(w*h)
// (Entry decoding: ent_row / ent_w, tree_dev.hpp.)
template <int MODE>
__device__ __forceinline__ int4 stage_row(uint32_t e, int64_t model, int64_t stride, const float* __restrict__ y,
                                          const float* __restrict__ t1, const float* __restrict__ t2,
                                          const float* __restrict__ qs, int wide) {
  const int64_t r = ent_row(e, wide);
  const float w = (float)ent_w(e, wide);
  int4 s;
  s.x = (int)e;
  if (MODE == 0) {
    s.y = (int)ent_w(e, wide); s.z = (int)y[r]; s.w = 0;
  } else if (MODE == 1) {
    const float t = t1[model * stride + r];
    const float wt = w * t;
    s.y = (int)ent_w(e, wide);
    s.z = (int)rintf(wt * qs[1]);
    s.w = (int)rintf((wt * t) * qs[2]);
  } else {
    s.y = (int)rintf((w * t1[model * stride + r]) * qs[0]);
    s.z = (int)rintf((w * t2[model * stride + r]) * qs[1]);
    s.w = 0;
  }
  return s;
}

// Statistic chunk [s0, s0 + Sc) of a histogram item (Sc < S when B * S does not fit the LDS table:
// many classes or wide bins -- each chunk is its own item, writing disjoint words).
template <int MODE>
__device__ __forceinline__ void add_row(int* my, int bin, int S, int s0, int Sc, const int4& st) {
  if (MODE == 0) {
    const int c = st.z - s0;
    if (c >= 0 && c < Sc) atomicAdd(my + bin * Sc + c, st.y);
  } else if (MODE == 1) {
    int* hb = my + bin * Sc;
    const int v[3] = {st.y, st.z, st.w};
    for (int k = 0; k < Sc; ++k) atomicAdd(hb + k, v[s0 + k]);
  } else {
    int* hb = my + bin * Sc;
    if (Sc == 2) {
      atomicAdd(hb, st.y); atomicAdd(hb + 1, st.z);
    } else {
      atomicAdd(hb, s0 ? st.z : st.y);
    }
  }
}

// Histogram build. Lane mapping (wave64): a wave-instruction covers R = 64 / FG rows x FG features;
// lane (rsub, fidx) owns histogram row (rsub, fidx) of the workgroup's LDS table, shared by its 4
// waves through integer LDS atomics -- lanes of one instruction never address the same word.
//  1. each wave takes 64 row entries at once (one coalesced load of the packed (row, weight) list)
//     and every lane gathers + quantises the statistics of *its* row (64 independent gathers);
//  2. the 64 records are staged in a wave-private LDS slot (one ds_write_b128 per lane);
//  3. lane (rsub, fidx) walks the staged rows R at a time, 8 rows unrolled: 8 broadcast ds_read_b128,
//     8 independent bin gathers Xb[row*F + feat] in flight, then the ds_add_u32s.
//
// Sparse missing bin (MODE 2, skip_bin >= 0; XGBoost's sparsity-aware histogram): entries whose bin is
// the reserved missing bin (XGBoost ``missing`` = 0.0 in the reference grid, i.e. every zero of the
// one-hot / null-indicator columns) issue no LDS atomic. Each wave instead folds its 64 staged rows'
// (g, h) into the chunk total with two wave reductions, and before the write-out the missing bin of
// every feature is recovered exactly as chunk total - sum of the other bins (integer arithmetic, so
// the histogram stays bit-identical to the CPU twin). Masking lanes does not shorten an LDS atomic
// wave-instruction, so this alone saves little; what it enables is the register path below.
//
// Register path (TMOG_ITEM_REG, sparse mode only): when every feature of the group has a single present
// bin (one-hot and null-indicator columns under ``missing`` = 0: value 1 -> bin 0, value 0 -> missing
// bin) a lane just sums the (g, h) of its rows with bin 0 in two registers -- no LDS atomics in the
// row loop at all, one per lane at the end. The tree grower groups such columns together
// (common/tree_grow.hpp), so on the headline table ~40 % of the feature groups skip the atomics.
// PMC on the tree micro-benchmark: ~0.064 LDS wave-instructions per CU-cycle at ~11 cycles each for
// a ds_add_u32 -> the LDS atomic unit is ~70 % busy; VALU ~12 % busy, so trading atomics for VALU pays.
// CSR path (TMOG_ITEM_CSR, MODE 2 with a sparse missing bin): one item covers ALL one-present-bin columns
// of a node row-chunk. Such a column's histogram has two non-zero bins -- the present bin 0 and the
// missing bin -- and the missing bin is the chunk total minus bin 0, so only the entries with bin 0
// matter: the row's CSR list (csr_ptr / csr_col, local column ids). The wave walks its 64 staged
// rows one at a time with the lanes spread over that row's list (coalesced 2-byte id loads; the ids
// of one row are distinct, so an LDS atomic wave-instruction never conflicts), kCsrU rows in flight.
// On the headline table that is ~50 entries per row instead of ~530 byte gathers.
constexpr int kCsrU = 16;
constexpr int kCsrG = 8;     // row slots per lane group in flight (register budget of the whole kernel)

// Wave64 int32 sum / max of non-negatives on DPP, result wave-uniform (the inclusive scan ends in lane 63): 6 DPP
// adds + one readlane instead of 6 ds_bpermute round trips through the LDS crossbar. Whole wave active.
template <bool MAX>
__device__ __forceinline__ int wave_reduce32(int v) {
#define TM_DPP_STEP(CTRL, ROWS)                                                         \
  {                                                                                     \
    const int t = __builtin_amdgcn_update_dpp(0, v, CTRL, ROWS, 0xF, false);           \
    v = MAX ? max(v, t) : v + t;                                                        \
  }
  TM_DPP_STEP(0x111, 0xF) TM_DPP_STEP(0x112, 0xF) TM_DPP_STEP(0x114, 0xF) TM_DPP_STEP(0x118, 0xF)
  TM_DPP_STEP(0x142, 0xA) TM_DPP_STEP(0x143, 0xC)
#undef TM_DPP_STEP
  return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ void hist_csr_item(const HistItem& it, const uint32_t* __restrict__ rows,
                                              const int32_t* __restrict__ node_model,
                                              const int64_t* __restrict__ node_hist_off, int64_t* __restrict__ hist,
                                              int B, int S, const float* __restrict__ t1,
                                              const float* __restrict__ t2, int64_t stride,
                                              const float* __restrict__ qscale, int skip_bin,
                                              const int64_t* __restrict__ csr_ptr,
                                              const uint16_t* __restrict__ csr_col, int* lds,
                                              const int2* __restrict__ gh, int wide) {
  const int nf = it.nf;
  int* a0 = lds;            // bin-0 sum of q(w g) per column
  int* a1 = lds + nf;       // bin-0 sum of q(w h)
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwaves = blockDim.x >> 6;
  const int soff = (2 * nf + 3) & ~3;        // per-wave row stage + list lengths after the sums
  int4* stg = reinterpret_cast<int4*>(lds + soff) + wave * 64;
  int* lens = lds + soff + 4 * 64 * nwaves + wave * 64;
  for (int i = threadIdx.x; i < 2 * nf; i += blockDim.x) lds[i] = 0;
  __syncthreads();
  const int64_t model = node_model ? node_model[it.node] : 0;
  const float* qs = qscale + model * S;
  const uint32_t* rp = rows + it.begin;
  const int64_t cnt = it.count;
  const float* t1m = t1 + model * stride;
  const float* t2m = t2 + model * stride;
  // One-chunk-ahead pipeline (as in hist_wide_item): the next chunk's entry is loaded before this
  // chunk's list walk, its statistics and list bounds after the first batch of id loads.
  const int64_t step = (int64_t)nwaves * 64;
  // staged statistics (gh != null): the entry's quantised (g, h) ride with the entry in node order, one
  // coalesced 8-byte load instead of two scattered 4-byte gathers per row
  const int2* ghp = gh ? gh + it.begin : nullptr;
  uint32_t e_n = 0;
  float g_n = 0.f, h_n = 0.f;
  int2 q_n = make_int2(0, 0);
  int64_t p0_n = 0, p1_n = 0;
  if ((int64_t)wave * 64 < cnt) {
    const int64_t i0 = min((int64_t)wave * 64 + lane, cnt - 1);
    e_n = rp[i0];
    const int64_t r = ent_row(e_n, wide);
    if (ghp) q_n = ghp[i0];
    else { g_n = t1m[r]; h_n = t2m[r]; }
    p0_n = csr_ptr[r]; p1_n = csr_ptr[r + 1];
  }
  for (int64_t base = (int64_t)wave * 64; base < cnt; base += step) {
    const int nrows = (int)min((int64_t)64, cnt - base);
    const float wt = (float)ent_w(e_n, wide);
    int4 mine;
    mine.x = (int)e_n;
    mine.y = ghp ? q_n.x : (int)rintf((wt * g_n) * qs[0]);
    mine.z = ghp ? q_n.y : (int)rintf((wt * h_n) * qs[1]);
    mine.w = 0;
    const int64_t q0 = p0_n;
    const int len = lane < nrows ? (int)(p1_n - p0_n) : 0;
    const bool more = base + step < cnt;             // wave-uniform
    const int64_t i_n = min(base + step + lane, cnt - 1);
    if (more) e_n = rp[i_n];
    // Row records go through the wave's LDS stage (q(g), q(h), list start) + list length: the lane groups
    // read them with plain LDS loads (no cross-lane shuffles, whose sources must all be active) and keep
    // only the entry ids in registers across the id gathers.
    stg[lane] = make_int4(mine.y, mine.z, (int)(uint32_t)(uint64_t)q0, (int)((uint64_t)q0 >> 32));
    lens[lane] = len;
    // Lane groups of W (a power of two >= this chunk's longest list, <= 64) take one row each, so a
    // wave-instruction covers 64 / W rows at (nearly) full lane use instead of one row per instruction
    // (the headline's rows carry ~17 entries).
    const int mx = wave_reduce32<true>(len);
    const int W = mx <= 8 ? 8 : mx <= 16 ? 16 : mx <= 32 ? 32 : 64;
    const int RPI = 64 / W;
    const int rs = lane / W, k = lane - rs * W;
    __builtin_amdgcn_s_waitcnt(0xC07F);        // lgkmcnt(0): staged records visible to the wave
    __builtin_amdgcn_wave_barrier();
    for (int j0 = 0; j0 < nrows; j0 += RPI * kCsrG) {
      int col[kCsrG];
      bool ok[kCsrG];
#pragma unroll
      for (int u = 0; u < kCsrG; ++u) {
        const int src = j0 + u * RPI + rs;
        const int sl = min(src, 63);
        const int ln = src < nrows ? lens[sl] : 0;
        const int4 rr = stg[sl];
        const int64_t k0 = (int64_t)(((uint64_t)(uint32_t)rr.w << 32) | (uint64_t)(uint32_t)rr.z);
        ok[u] = k < ln;
        col[u] = csr_col[ok[u] ? k0 + k : k0 > 0 ? k0 - 1 : 0];   // unpredicated load of a valid id
      }
      __builtin_amdgcn_sched_barrier(0);
      if (j0 == 0 && more) {
        const int64_t r = ent_row(e_n, wide);
        if (ghp) q_n = ghp[i_n];
        else { g_n = t1m[r]; h_n = t2m[r]; }
        p0_n = csr_ptr[r]; p1_n = csr_ptr[r + 1];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kCsrG; ++u)
        if (ok[u]) {
          const int2 gh = *reinterpret_cast<const int2*>(&stg[min(j0 + u * RPI + rs, 63)]);
          atomicAdd(a0 + col[u], gh.x);
          atomicAdd(a1 + col[u], gh.y);
        }
      if (W == 64) {                       // lists longer than the lane group
#pragma unroll
        for (int u = 0; u < kCsrG; ++u) {
          const int src = j0 + u * RPI + rs;
          const int sl = min(src, 63);
          const int ln = src < nrows ? lens[sl] : 0;
          if (ln <= 64) continue;
          const int4 rr = stg[sl];
          const int64_t k0 = (int64_t)(((uint64_t)(uint32_t)rr.w << 32) | (uint64_t)(uint32_t)rr.z);
          for (int kk = k + 64; kk < ln; kk += 64) {
            const int c = csr_col[k0 + kk];
            atomicAdd(a0 + c, rr.x);
            atomicAdd(a1 + c, rr.y);
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();           // the stage is rewritten by the next chunk
  }
  __syncthreads();
  // Only bin 0 of these columns is written: the split scan and split reduce evaluate a one-present-bin
  // column from its bin 0 and the node totals (read from a multi-bin column), and zero_segments /
  // hist_subtract maintain only that word, so no other word of these columns is ever live.
  int64_t* out = hist + node_hist_off[it.node] + (int64_t)it.fg0 * B * S;
  const int per = B * S;
  const bool excl = (it.excl & TMOG_ITEM_SOLE) != 0;
  for (int k = threadIdx.x; k < nf * S; k += blockDim.x) {
    const int f = k / S, s = k - f * S;
    const int v = s ? a1[f] : a0[f];
    int64_t* w = out + (int64_t)f * per + s;
    if (excl) *w = v;
    else if (v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(w), (unsigned long long)(int64_t)v);
  }
}


// Wide-load path (MODE 2, TMOG_ITEM_WIDE): a dense group of FG <= 64 multi-bin columns that are physically
// contiguous and dword aligned in Xb (col0 % 4 == 0, row stride % 4 == 0; the XGBoost learner pads its
// growth-order matrix to that). Lane (rs, d) loads dword d of the group's row segment -- 4 bins of one
// row in one 4-byte load -- so a wave-instruction covers 64 / ceil(FG/4) rows (4 for FG = 64) and
// kWideU instructions keep 4x the bytes of the byte-gather path in flight for the same registers (the
// kernel is gather-latency bound: MI355X_MICROARCH.md "72 KiB in flight per CU"). The statistics are
// packed as one 64-bit word (q(g) << 32) + q(h) per (feature, bin) -- h >= 0 and its per-item sum stays
// below 2^31 (qmax), so the low half never carries -- and added with ONE ds_add_u64 instead of two
// ds_add_u32. Output is identical (integer sums) to the byte path and the CPU twin.
constexpr int kWideU = 16;

// LDS table layout (bank-conflict free): the ds_add_u64 of a wave-instruction is serviced in 4 groups of 16
// contiguous lanes, and a group conflicts when two of its lanes hit one bank (byte address / 4 mod 32). Lanes are
// (rs, d) with the dword count padded to NP = 16 / 8 / 4 / 2 / 1 (a power of two), so a 16-lane group holds
// 16 / NP rows of one group of NP dwords; lane position p = lane % 16 is unique in its group. Word
// (k, b, p) = k * (B + 1) * 16 + b * 16 + p holds feature 4 d + k, bin b, for row slot p / NP: its bank pair
// 2 p mod 32 depends on the lane position only, never on the (data-dependent) bin -- the feature-major layout
// put lanes of random bins on random banks (~3.5-way per group). Row slots of one group are separate copies,
// folded before the write-out; the table stays 64 x (B + 1) words.
__device__ __forceinline__ void hist_wide_item(const HistItem& it, const uint8_t* __restrict__ Xb, int F, int col0,
                                               const uint32_t* __restrict__ rows,
                                               const int32_t* __restrict__ node_model,
                                               const int64_t* __restrict__ node_hist_off, int64_t* __restrict__ hist,
                                               int B, const float* __restrict__ t1, const float* __restrict__ t2,
                                               int64_t stride, const float* __restrict__ qscale, int skip_bin,
                                               int* lds, const int2* __restrict__ gh, int wide) {
  const int FG = it.nf;
  const int ND = (FG + 3) >> 2;                    // dwords of the group's row segment (<= 16)
  const int NP = ND <= 1 ? 1 : ND <= 2 ? 2 : ND <= 4 ? 4 : ND <= 8 ? 8 : 16;
  const int RPI = 64 / NP;                         // rows per wave-instruction (>= 4)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int rs = lane / NP, d = lane - rs * NP;
  const int pos = lane & 15;
  const int sub = (B + 1) * 16;                    // words per k-plane
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(lds);
  const int twords = 4 * sub;                      // == 64 * (B + 1): the launcher's LDS size
  const int toff = (2 * twords + 3) & ~3;
  int4* stage = reinterpret_cast<int4*>(lds + toff) + wave * 64;
  int* tot = lds + toff + 4 * 64 * nwaves;
  for (int i = threadIdx.x; i < twords; i += blockDim.x) tab[i] = 0ull;
  if (threadIdx.x < 2) tot[threadIdx.x] = 0;
  __syncthreads();
  const bool sparse = skip_bin >= 0;
  const int64_t model = node_model ? node_model[it.node] : 0;
  const float* qs = qscale + model * 2;
  const uint32_t* rp = rows + it.begin;
  const int64_t cnt = it.count;
  // buffer loads: one descriptor for the group's first column (wave-uniform) and a 32-bit per-lane byte
  // offset row * F + 4 d (the grower takes this path only for matrices below 2 GiB) -- one VGPR per
  // gather address instead of two. Pad lanes (d >= ND) re-read the last dword and add 0.
  const uint64_t xbase = (uint64_t)(uintptr_t)(Xb + col0);
  const uint32_t xlo = __builtin_amdgcn_readfirstlane((uint32_t)xbase);
  const uint32_t xhi = __builtin_amdgcn_readfirstlane((uint32_t)(xbase >> 32));
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(uintptr_t)(((uint64_t)xhi << 32) | xlo), (short)0, 0x7FFFFFFF, 0x00020000);
  const uint32_t lane_off = 4u * (uint32_t)min(d, ND - 1);
  const float* t1m = t1 + model * stride;
  const float* t2m = t2 + model * stride;
  // Software pipeline over the wave's 64-row chunks: the next chunk's row entry is loaded before this
  // chunk's bin gathers and its (g, h) right after them, so the dependent entry -> statistic -> bin
  // latency chain of a chunk overlaps the previous chunk's gathers and atomics instead of adding up.
  const int64_t step = (int64_t)nwaves * 64;
  const int2* ghp = gh ? gh + it.begin : nullptr;   // staged (g, h): coalesced with the entries
  uint32_t e_n = 0;
  float g_n = 0.f, h_n = 0.f;
  int2 q_n = make_int2(0, 0);
  if ((int64_t)wave * 64 < cnt) {
    const int64_t i0 = min((int64_t)wave * 64 + lane, cnt - 1);
    e_n = rp[i0];
    if (ghp) q_n = ghp[i0];
    else {
      g_n = t1m[ent_row(e_n, wide)];
      h_n = t2m[ent_row(e_n, wide)];
    }
  }
  for (int64_t base = (int64_t)wave * 64; base < cnt; base += step) {
    const int nrows = (int)min((int64_t)64, cnt - base);
    const float wt = (float)ent_w(e_n, wide);
    int4 mine;
    mine.x = (int)e_n;
    mine.y = ghp ? q_n.x : (int)rintf((wt * g_n) * qs[0]);
    mine.z = ghp ? q_n.y : (int)rintf((wt * h_n) * qs[1]);
    mine.w = 0;
    const bool more = base + step < cnt;             // wave-uniform
    const int64_t i_n = min(base + step + lane, cnt - 1);
    if (more) {
      e_n = rp[i_n];
      if (ghp) q_n = ghp[i_n];                 // independent of the entry: issued with it
    }
    stage[lane] = make_int4(mine.y, mine.z, mine.x, 0);   // (q(g), q(h), entry): (g, h) 8-byte aligned
    if (sparse) {
      const int a = wave_reduce32<false>(lane < nrows ? mine.y : 0);
      const int b = wave_reduce32<false>(lane < nrows ? mine.z : 0);
      if (lane == 0) {
        atomicAdd(tot, a);
        atomicAdd(tot + 1, b);
      }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);        // lgkmcnt(0): staged records visible to the wave
    __builtin_amdgcn_wave_barrier();
    {                                          // RPI * kWideU >= 64 (NP <= 16): one pass covers the chunk
      // only the row ids stay in registers across the gathers; (g, h) are re-read from the LDS stage
      // at the atomics (fewer VGPRs -> more waves, i.e. more gathers in flight per CU)
      uint32_t off[kWideU], w[kWideU];
#pragma unroll
      for (int u = 0; u < kWideU; ++u)
        off[u] = (wide ? (uint32_t)stage[min(u * RPI + rs, 63)].z * (uint32_t)F     // < 2^31 (grower guard)
                       : __umul24((uint32_t)stage[min(u * RPI + rs, 63)].z & 0xFFFFFFu, (uint32_t)F)) + lane_off;
#pragma unroll
      for (int u = 0; u < kWideU; ++u) w[u] = __builtin_amdgcn_raw_buffer_load_b32(xrs, (int)off[u], 0, 0);
      __builtin_amdgcn_sched_barrier(0);       // keep the next chunk's statistic loads behind the gathers
      if (more && !ghp) {
        g_n = t1m[ent_row(e_n, wide)];
        h_n = t2m[ent_row(e_n, wide)];
      }
      __builtin_amdgcn_sched_barrier(0);
      // branch-free: masked-off work (rows past the chunk, pad features) adds 0 to the lane's own word
      // instead of toggling EXEC around every atomic (a masked lane costs the same)
#pragma unroll
      for (int u = 0; u < kWideU; ++u) {
        const bool live = u * RPI + rs < nrows;
        const int2 st = *reinterpret_cast<const int2*>(&stage[min(u * RPI + rs, 63)]);
        const unsigned long long pk = live ? ((unsigned long long)(uint32_t)st.x << 32) + (unsigned long long)(uint32_t)st.y
                                           : 0ull;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int bin = (int)((w[u] >> (8 * k)) & 0xFFu);
          atomicAdd(tab + k * sub + bin * 16 + pos, 4 * d + k < FG ? pk : 0ull);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  // fold the 16 / NP row-slot copies of every (k, bin) row into its first NP words
  if (NP < 16) {
    for (int i = threadIdx.x; i < 4 * B * NP; i += blockDim.x) {
      const int r = i / NP, dd = i - r * NP;                   // r = k * B + bin
      unsigned long long* row = tab + (r / B) * sub + (r % B) * 16;
      unsigned long long acc = row[dd];
      for (int c = NP; c < 16; c += NP) acc += row[c + dd];
      row[dd] = acc;
    }
    __syncthreads();
  }
  auto tix = [sub](int f, int b) { return (f & 3) * sub + b * 16 + (f >> 2); };
  if (sparse) {       // missing bin = chunk totals - the other bins, packed into the spare bin-B word
    for (int f = threadIdx.x; f < FG; f += blockDim.x) {
      long long g = 0, h = 0;
      for (int b = 0; b < B; ++b) {
        if (b == skip_bin) continue;
        const unsigned long long v = tab[tix(f, b)];
        g += (long long)v >> 32;
        h += (long long)(v & 0xFFFFFFFFull);
      }
      const long long mg = (long long)tot[0] - g, mh = (long long)tot[1] - h;
      tab[tix(f, B)] = ((unsigned long long)mg << 32) + (unsigned long long)(uint32_t)mh;
    }
    __syncthreads();
  }
  int64_t* out = hist + node_hist_off[it.node] + (int64_t)it.fg0 * B * 2;
  const bool excl = (it.excl & TMOG_ITEM_SOLE) != 0;
  for (int k = threadIdx.x; k < FG * B; k += blockDim.x) {
    const int f = k / B, b = k - f * B;
    const unsigned long long v = tab[tix(f, (sparse && b == skip_bin) ? B : b)];
    const int64_t g = (long long)v >> 32, h = (long long)(v & 0xFFFFFFFFull);
    int64_t* o = out + (int64_t)k * 2;
    if (excl) {
      o[0] = g;
      o[1] = h;
    } else {
      if (g != 0) atomicAdd(reinterpret_cast<unsigned long long*>(o), (unsigned long long)g);
      if (h != 0) atomicAdd(reinterpret_cast<unsigned long long*>(o + 1), (unsigned long long)h);
    }
  }
}

constexpr int HIST_U = 16;   // row bins gathered per lane before their LDS atomics (loads in flight)

// Diagnostics only (tmog_hip_debug_flags, TMOG_HIST_DEBUG): bit 0 skips CSR items, bit 1 skips wide /
// dense multi-bin items -- the trees are then wrong; used to time the item kinds separately.
__device__ int g_hist_debug = 0;

// Wide-load items in a kernel of their own (TMOG_HIST_WIDE_SPLIT=1; the grower puts them first): the mixed
// kernel's register budget is set by its general and CSR paths, this one's by the wide path alone, so
// more waves -- more row gathers in flight -- fit on a CU (OCC = requested waves per SIMD: 7 is
// the LDS limit of these 21 KB workgroups, at a couple of spilled registers; TMOG_HIST_WIDE_OCC picks).
template <int OCC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(OCC))) hist_wide_kernel(
    const uint8_t* __restrict__ Xb, int F, const uint32_t* __restrict__ rows, const HistItem* __restrict__ items,
    const int32_t* __restrict__ node_feat_off, const int32_t* __restrict__ feat_list,
    const int32_t* __restrict__ node_model, const int64_t* __restrict__ node_hist_off, int64_t* __restrict__ hist,
    int B, const float* __restrict__ t1, const float* __restrict__ t2, int64_t stride,
    const float* __restrict__ qscale, int skip_bin, const int2* __restrict__ gh, int wide,
    const uint8_t* __restrict__ Xh, int Fh) {
  extern __shared__ int lds_w[];
  if (g_hist_debug & 2) return;
  const HistItem it = items[blockIdx.x];
  hist_wide_item(it, Xh, Fh, feat_list[node_feat_off[it.node] + it.fg0], rows, node_model, node_hist_off, hist, B,
                 t1, t2, stride, qscale, skip_bin, lds_w, gh, wide);
}


// GEN = false (MODE 2 launches whose items are all CSR / wide-load, the XGBoost case): the byte-gather
// path is not compiled in, so its registers do not cap the occupancy of the other two (106 -> ~74 VGPRs).
template <int MODE, bool GEN = true>
__global__ void __launch_bounds__(256) hist_build_kernel(
    const uint8_t* __restrict__ Xb, int F, const uint32_t* __restrict__ rows, const HistItem* __restrict__ items,
    const int32_t* __restrict__ node_feat_off, const int32_t* __restrict__ feat_list,
    const int32_t* __restrict__ node_model, const int64_t* __restrict__ node_hist_off, int64_t* __restrict__ hist,
    int B, int S, const float* __restrict__ y, const float* __restrict__ t1, const float* __restrict__ t2,
    int64_t stride, const float* __restrict__ qscale, int skip_bin, const int64_t* __restrict__ csr_ptr,
    const uint16_t* __restrict__ csr_col, int Sc, const int2* __restrict__ gh, const int* __restrict__ dcount,
    int wide, const uint8_t* __restrict__ Xh, int Fh) {
  extern __shared__ __attribute__((aligned(16))) int lds[];
  // dcount (device-planned levels, tree_resident.hip): the grid is an upper bound, the item count is on the device
  if (dcount != nullptr && (int)blockIdx.x >= *dcount) return;
  const HistItem it = items[blockIdx.x];
  const int s0 = ((it.excl >> TMOG_ITEM_SC_SHIFT) & 0xFF) * Sc;   // statistic chunk of this item
  const int sc = min(Sc, S - s0);
  if (MODE == 2 && g_hist_debug) {
    if ((g_hist_debug & 1) && (it.excl & TMOG_ITEM_CSR)) return;
    if ((g_hist_debug & 2) && !(it.excl & TMOG_ITEM_CSR)) return;
  }
  if (MODE == 2 && (it.excl & TMOG_ITEM_CSR)) {
    hist_csr_item(it, rows, node_model, node_hist_off, hist, B, S, t1, t2, stride, qscale, skip_bin, csr_ptr,
                  csr_col, lds, gh, wide);
    return;
  }
  if (MODE == 2 && (it.excl & TMOG_ITEM_WIDE)) {        // wide-load items read the compact matrix (GrowArgs.Xh, or Xb)
    hist_wide_item(it, Xh, Fh, feat_list[node_feat_off[it.node] + it.fg0], rows, node_model, node_hist_off, hist, B,
                   t1, t2, stride, qscale, skip_bin, lds, gh, wide);
    return;
  }
  if constexpr (!GEN) {
    return;
  } else {
  const int FG = it.nf;
  const int R = 64 / FG;
  const int rowstride = B * sc + 1;           // padded feature row (this item's statistic chunk)
  const int ncopy_words = R * FG * rowstride;  // <= 64 * rowstride
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwaves = blockDim.x >> 6;
  int4* stage = reinterpret_cast<int4*>(lds + ((ncopy_words + 3) & ~3)) + wave * 64;
  int* tot = lds + ((ncopy_words + 3) & ~3) + 4 * 64 * 4;     // chunk totals (sparse missing bin)
  const bool sparse = MODE == 2 && skip_bin >= 0;
  const bool regacc = sparse && (it.excl & TMOG_ITEM_REG);
  const bool excl = (it.excl & TMOG_ITEM_SOLE) != 0;
  for (int i = threadIdx.x; i < ncopy_words; i += blockDim.x) lds[i] = 0;
  if (threadIdx.x < TM_MAX_S) tot[threadIdx.x] = 0;
  __syncthreads();

  const int rsub = lane / FG;
  const int fidx = lane - rsub * FG;
  const bool active = rsub < R;
  const int feat = active ? feat_list[node_feat_off[it.node] + it.fg0 + fidx] : 0;
  const int64_t model = node_model ? node_model[it.node] : 0;
  const float* qs = qscale + model * S;
  int* my = lds + (rsub * FG + fidx) * rowstride;
  const uint32_t* rp = rows + it.begin;
  const int64_t cnt = it.count;

  int racc0 = 0, racc1 = 0;     // register path sums (bin 0 of this lane's feature)
  // Loads are never predicated (a masked "load or skip" makes hipcc branch around every load and wait
  // vmcnt(0) per element): out-of-range slots read a valid dummy record and are masked at the atomic.
  for (int64_t base = (int64_t)wave * 64; base < cnt; base += (int64_t)nwaves * 64) {
    const int64_t ri = min(base + lane, cnt - 1);
    const int nrows = (int)min((int64_t)64, cnt - base);
    int4 mine;
    if (MODE == 2 && gh) {
      const int2 q = gh[it.begin + ri];
      mine = make_int4((int)rp[ri], q.x, q.y, 0);
    } else {
      mine = stage_row<MODE>(rp[ri], model, stride, y, t1, t2, qs, wide);
    }
    stage[lane] = mine;
    if (sparse) {
      // chunk totals: one wave reduction of the 64 staged (g, h) records, one LDS add per wave
      const int a = wave_reduce32<false>(lane < nrows ? mine.y : 0);
      const int b = wave_reduce32<false>(lane < nrows ? mine.z : 0);
      if (lane == 0) {
        atomicAdd(tot, a);
        atomicAdd(tot + 1, b);
      }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);        // lgkmcnt(0): staged records visible to the wave
    __builtin_amdgcn_wave_barrier();
    if (regacc) {
      for (int j0 = 0; j0 < nrows; j0 += R * 8) {
        int4 st[8];
        int bin[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) st[u] = stage[min(j0 + u * R + rsub, 63)];
#pragma unroll
        for (int u = 0; u < 8; ++u) bin[u] = (int)Xb[(int64_t)ent_row((uint32_t)st[u].x, wide) * F + feat];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const bool hit = j0 + u * R + rsub < nrows && bin[u] == 0;
          racc0 += hit ? st[u].y : 0;
          racc1 += hit ? st[u].z : 0;
        }
      }
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    for (int j0 = 0; j0 < nrows; j0 += R * HIST_U) {
      int4 st[HIST_U];
      int bin[HIST_U];
#pragma unroll
      for (int u = 0; u < HIST_U; ++u) st[u] = stage[min(j0 + u * R + rsub, 63)];
#pragma unroll
      for (int u = 0; u < HIST_U; ++u) bin[u] = (int)Xb[(int64_t)ent_row((uint32_t)st[u].x, wide) * F + feat];
#pragma unroll
      for (int u = 0; u < HIST_U; ++u)
        if (active && j0 + u * R + rsub < nrows && bin[u] != skip_bin) add_row<MODE>(my, bin[u], S, s0, sc, st[u]);
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();

  int64_t* out = hist + node_hist_off[it.node] + (int64_t)it.fg0 * B * S;
  const int words = FG * B * S;
  if (regacc) {
    if (active) {
      atomicAdd(my, racc0);
      atomicAdd(my + 1, racc1);
    }
    __syncthreads();
  }
  if (sparse) {
    // fold the R copies into copy 0, then recover each feature's missing bin from the chunk totals
    if (R > 1) {
      for (int k = threadIdx.x; k < words; k += blockDim.x) {
        const int f = k / (B * S);
        const int rem = k - f * (B * S);
        int acc = 0;
        for (int r = 0; r < R; ++r) acc += lds[(r * FG + f) * rowstride + rem];
        lds[f * rowstride + rem] = acc;
      }
      __syncthreads();
    }
    for (int t = threadIdx.x; t < FG * S; t += blockDim.x) {
      const int f = t / S, s = t - (t / S) * S;
      int* row = lds + f * rowstride;
      int sum = 0;
      for (int b = 0; b < B; ++b) sum += (b == skip_bin) ? 0 : row[b * S + s];
      row[skip_bin * S + s] = tot[s] - sum;
    }
    __syncthreads();
    // TMOG_ITEM_LIVE0: the group's columns have one present bin and only their bin 0 is live (the grower
    // orders multi-bin columns first and zero / subtract maintain bin 0 alone, see hist_csr_item)
    const int wlimit = (it.excl & TMOG_ITEM_LIVE0) ? S : B * S;
    for (int k = threadIdx.x; k < words; k += blockDim.x) {
      const int f = k / (B * S);
      if (k - f * (B * S) >= wlimit) continue;
      const int64_t acc = lds[f * rowstride + (k - f * (B * S))];
      if (excl) out[k] = acc;
      else if (acc != 0) atomicAdd(reinterpret_cast<unsigned long long*>(out + k), (unsigned long long)acc);
    }
    return;
  }
  // fold the R private copies and write the node histogram of this feature group (chunk slots only)
  const int cwords = FG * B * sc;
  for (int k = threadIdx.x; k < cwords; k += blockDim.x) {
    const int f = k / (B * sc);
    const int rem = k - f * (B * sc);
    int64_t acc = 0;
    for (int r = 0; r < R; ++r) acc += lds[(r * FG + f) * rowstride + rem];
    const int bin = rem / sc, c = rem - bin * sc;
    int64_t* w = out + ((int64_t)f * B + bin) * S + s0 + c;
    if (excl) *w = acc;
    else if (acc != 0) atomicAdd(reinterpret_cast<unsigned long long*>(w), (unsigned long long)acc);
  }
  }   // GEN
}

// sibling = parent - small (histogram subtraction trick), size words each
// Word k of a node's live region: with dense >= 0 the region is the first `dense` words (the multi-bin
// columns, every bin) followed by bin 0 of each one-present-bin column -- the only words the split scan,
// the split reduce and the next level's subtraction read of those columns (tree_grow.hpp orders the
// multi-bin columns first), so ~530 of the headline table's ~730 columns move S words instead of B * S.
// 32-bit index math (a node's histogram is < 2^31 words; int64 division is a long software sequence)
__device__ __forceinline__ int live_word(int k, int dense, int per, int S) {
  if (dense < 0 || k < dense) return k;
  const int t = k - dense, f = t / S;
  return dense + f * per + (t - f * S);
}

__global__ void hist_subtract_kernel(int64_t* __restrict__ hist, const int64_t* __restrict__ parent,
                                     const int64_t* __restrict__ parent_off, const int64_t* __restrict__ small_off,
                                     const int64_t* __restrict__ out_off, const int64_t* __restrict__ size, int n,
                                     int64_t dense, int per, int S) {
  const int j = blockIdx.y;
  if (j >= n) return;
  const int sz = (int)live_words(size[j], dense, per, S);
  const int dn = (int)dense;
  const int64_t* p = parent + parent_off[j];
  const int64_t* s = hist + small_off[j];
  int64_t* o = hist + out_off[j];
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < sz; k += gridDim.x * blockDim.x) {
    const int w = live_word(k, dn, per, S);
    o[w] = p[w] - s[w];
  }
}

// zero the histograms of nodes built from several row chunks (their items accumulate atomically);
// single-chunk and derived nodes are fully overwritten, so the level buffer is never memset whole
__global__ void zero_segments_kernel(int64_t* __restrict__ hist, const int64_t* __restrict__ off,
                                     const int64_t* __restrict__ size, int n, int64_t dense, int per, int S,
                                     int n_dense, const int* __restrict__ dcnt) {
  const int j = blockIdx.y;
  if (dcnt != nullptr) {       // device-planned level: [segments, whole-node segments] on the device
    n = dcnt[0];
    n_dense = dcnt[1];
  }
  if (j >= n) return;
  int64_t* o = hist + off[j];
  const int64_t dj = j < n_dense ? dense : 0;      // segments past n_dense start at a one-present-bin region
  const int sz = (int)live_words(size[j], dj, per, S);
  const int dn = (int)dj;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < sz; k += gridDim.x * blockDim.x)
    o[live_word(k, dn, per, S)] = 0;
}

// Dynamic LDS of a histogram workgroup: 64 padded copies of the B x Sc table + the 4 waves' row stage + totals
// (hist_build_kernel's general path), and the wide-load items' 64 features x (B + 1) packed int64 words + stage +
// totals (hist_wide_item).
inline size_t hist_lds_bytes(int B, int Sc) {
  return (size_t)(((64 * (B * Sc + 1)) + 3) & ~3) * sizeof(int) + 4 * 64 * sizeof(int4) + TM_MAX_S * sizeof(int);
}
inline size_t hist_wide_lds_bytes(int B) {
  return (size_t)((2 * (64 * (B + 1) + 17) + 3) & ~3) * sizeof(int) + 4 * 64 * sizeof(int4) + 4 * sizeof(int);
}

}  // namespace

int tmog::prime_tree_hist() { return prime_kernel(&zero_segments_kernel); }

// ------------------------------------------------------------------------------------- C ABI
extern "C" {

int tmog_hip_debug_flags(int flags) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_hist_debug), &flags, sizeof(int));
}

int tmog_hip_hist_build(const uint8_t* Xb, int F, const uint32_t* rows, const void* items, int n_items,
                        const int32_t* node_feat_off, const int32_t* feat_list, const int32_t* node_model,
                        const int64_t* node_hist_off, int64_t* hist, int B, int mode, int S, const float* y,
                        const float* t1, const float* t2, int64_t stride, const float* qscale, int skip_bin,
                        const int64_t* csr_ptr, const uint16_t* csr_col, int Sc, int n_wide, int need_general,
                        hipStream_t stream, const int32_t* gh_words, const int* dcount, int wide_rows,
                        const uint8_t* Xh, int Fh) {
  if (n_items == 0) return 0;
  if (Xh == nullptr) {
    Xh = Xb;
    Fh = F;
  }
  if (dcount != nullptr && n_wide != 0) return -2;   // device-counted launches: one mixed launch
  const int2* gh = reinterpret_cast<const int2*>(gh_words);
  if (gh && mode != 2) return -2;
  if (Sc <= 0 || Sc > S) Sc = S;
  size_t lds = hist_lds_bytes(B, Sc);
  if (mode == 2 && S == 2) lds = std::max(lds, hist_wide_lds_bytes(B));
  if (lds > 160 * 1024) return -2;
  if (skip_bin >= B || (mode == 2 && skip_bin >= 0 && (S != 2 || Sc != S))) return -2;
  if (mode == 0 && S > TM_WIDE_MAX_S) return -2;
  if ((csr_ptr != nullptr) != (csr_col != nullptr) || (csr_ptr && (mode != 2 || skip_bin <= 0))) return -2;
  const HistItem* it = (const HistItem*)items;
  if (n_wide < 0 || n_wide > n_items || (n_wide > 0 && (mode != 2 || S != 2))) return -2;
  // The grower lists the wide-load items first. By default they share the launch with the other items
  // (the mixed kernel runs them concurrently with the CSR items); TMOG_HIST_WIDE_SPLIT=1 launches them
  // as hist_wide_kernel -- measured slower on the headline (1086 vs 974 ms per step: the two launches
  // serialise and each has its own tail), kept for experiments.
  static const bool split_wide = [] { const char* e = std::getenv("TMOG_HIST_WIDE_SPLIT"); return e && e[0] == '1'; }();
  if (!split_wide) n_wide = 0;
  if (n_wide > 0) {
    static const int occ = [] { const char* e = std::getenv("TMOG_HIST_WIDE_OCC"); return e ? std::atoi(e) : 6; }();
#define TM_HIST_WIDE(OCC)                                                                                      \
  hipLaunchKernelGGL(hist_wide_kernel<OCC>, dim3(n_wide), dim3(256), lds, stream, Xb, F, rows, it, node_feat_off, \
                     feat_list, node_model, node_hist_off, hist, B, t1, t2, stride, qscale, skip_bin, gh, wide_rows, Xh, Fh)
    if (occ >= 7) TM_HIST_WIDE(7);
    else TM_HIST_WIDE(6);
#undef TM_HIST_WIDE
    it += n_wide;
    n_items -= n_wide;
    if (n_items == 0) return (int)hipGetLastError();
  }
  // Modes 0 and 1 have no missing bin to skip; their CSR lists and staged (g, h) are null by the guards above.
  const int skip = (mode == 0 || mode == 1) ? -1 : skip_bin;
#define TM_HIST(...)                                                                                           \
  hipLaunchKernelGGL((hist_build_kernel<__VA_ARGS__>), dim3(n_items), dim3(256), lds, stream, Xb, F, rows, it, \
                     node_feat_off, feat_list, node_model, node_hist_off, hist, B, S, y, t1, t2, stride, qscale, \
                     skip, csr_ptr, csr_col, Sc, gh, dcount, wide_rows, Xh, Fh)
  if (mode == 0) TM_HIST(0);
  else if (mode == 1) TM_HIST(1);
  else if (need_general) TM_HIST(2);
  else TM_HIST(2, false);
#undef TM_HIST
  return (int)hipGetLastError();
}

// The grids of the subtract / zero kernels are sized to the live words of the largest node, what they touch
// (sized from the full B x S words they launched ~4x the workgroups the live region needs)
int tmog_hip_hist_subtract(int64_t* hist, const int64_t* parent, const int64_t* parent_off, const int64_t* small_off,
                           const int64_t* out_off, const int64_t* size, int n, int64_t max_size, int64_t dense,
                           int per, int S, hipStream_t stream) {
  if (n == 0) return 0;
  if (max_size >= (int64_t)1 << 31) return -2;
  int gx = (int)min((live_words(max_size, dense, per, S) + 255) / 256, (int64_t)1024);
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(hist_subtract_kernel, dim3(gx, n), dim3(256), 0, stream, hist, parent, parent_off, small_off,
                     out_off, size, n, dense, per, S);
  return (int)hipGetLastError();
}

int tmog_hip_zero_segments(int64_t* hist, const int64_t* off, const int64_t* size, int n, int64_t max_size,
                           int64_t dense, int per, int S, hipStream_t stream, int n_dense, const int* dn) {
  if (n == 0) return 0;
  if (max_size >= (int64_t)1 << 31) return -2;
  const int64_t lw = std::max(live_words(max_size, dense, per, S), live_words(max_size, 0, per, S));
  int gx = (int)min((lw + 255) / 256, (int64_t)1024);
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(zero_segments_kernel, dim3(gx, n), dim3(256), 0, stream, hist, off, size, n, dense, per, S,
                     n_dense, dn);
  return (int)hipGetLastError();
}

// Loads the code objects of the four tree translation units (histograms, split finding, partition, scoring) on the
// current device from the calling thread: each unit's tmog::prime_* asks for the attributes of one of its kernels.
// The HIP runtime loads a translation unit's kernels at the first launch of any of them; the tree grower's
// job-group threads make first launches into the three growth units and the boosting loop scores with the forest
// kernels, and that first load racing on two threads crashed inside the runtime under the profiler (rocprofv3
// --kernel-trace, XGBoost-only run). The growers call this before they spawn the threads. First non-zero status.
int tmog_hip_tree_prime() {
  for (int (*prime)() : {prime_tree_hist, prime_tree_split, prime_tree_partition, prime_forest_predict})
    if (const int rc = prime()) return rc;
  return 0;
}

// Largest statistic chunk whose per-workgroup LDS table (64 copies of B x Sc words) fits the LDS.
int tmog_hip_hist_stat_chunk(int B, int S) {
  int sc = S;
  while (sc > 1 && hist_lds_bytes(B, sc) > 160 * 1024) --sc;
  return sc;
}

}  // extern "C"
