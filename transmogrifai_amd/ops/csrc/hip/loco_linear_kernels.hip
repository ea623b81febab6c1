// Exact leave-one-column-out (LOCO) insights of the linear-margin learners, CDNA4 (gfx950).
//
// The score of these learners is link(b + W^T x), so zeroing column j moves the margin by exactly -W[j, :] x_j and
// zeroing a column group by the sum of those terms: the LOCO change of every candidate follows from one pass over
// the record's non-zeros, and the top-K selection of RecordInsightsLOCO is done on the spot. Only cols [n, K] and
// diffs [n, K, C] are written; there is no perturbed batch and no [n, m, C] candidate array.
//
// Mapping: one wave per record, a workgroup of four waves strides over the records.
//   pass 1  the row is read once, 64 columns per step (coalesced), widened to fp64 and kept in the wave's LDS slice;
//           each lane sums W[j, :] x_j of its columns, the partial margins are folded across the wave by a butterfly
//           of cross-lane moves (fixed order), the base scores s(m) and the explained score column follow.
//   pass 2  per non-zero: t_j = W[j, :] x_j and the change s(m) - s(m - t_j). A plain column is a candidate at once.
//           A grouped column (text hashes, date circles) adds to its group's LDS accumulator [G][C]: the changes
//           under Avg (divided by the group size at the end), the t_j under LeaveOutVector (one link evaluation at
//           the end). The lanes of a chunk that fall in one group are summed in lane order by cross-lane moves and
//           one lane adds to LDS (loop over the chunk's distinct groups by ballot): no floating-point atomics, so
//           a run is bitwise repeatable. The same lane records the group's first active column.
//   select  the running top-kk positives and top-kk negatives live in registers, lane i holding the i-th best
//           (key, id). The lanes of a chunk that beat the kk-th key are found by ballot and inserted one at a time
//           by a compare-and-shift across lanes; groups are offered after the last chunk. Candidates arrive in
//           candidate order (plain columns by column, then groups in plan order) and an equal key goes behind, so
//           ties keep the earlier candidate. The two lists are merged by rank (positives before negatives on an
//           equal key; |v| or v descending, first K) and the C changes of the winners are recomputed.
//
// Deviations from a fully staged design, neither of them measured against the alternative:
//   * W and cand_of_col are not staged in LDS. Only the non-zero lanes read them (C_m fp64 per non-zero), they are
//     at most d C_m 8 bytes and shared by all waves through L2; staging would cost a full copy per workgroup and
//     the LDS that bounds the group count.
//   * A row wider than kRowSlice columns is read again from memory in pass 2 instead of from LDS.
//
// LDS: a workgroup may take all 160 KB of a CU. Per wave: the row slice (d rounded up to 64, fp64, at most
// kRowSlice = 2048 columns = 16 KB) and G (8 C + 4) bytes of group state. When that exceeds 160 KB the slice is
// dropped, so the group limit is 4 G (8 C + 4) <= 163840: G <= 310 at C = 16, 2048 at C = 2, 3413 at C = 1.
// Beyond it the launcher returns -3 and the caller uses its host formula.
//
// All arithmetic is fp64 in plain C++ (exp, 1/x, pow); there is no product larger than C_m per non-zero, so no
// matrix instructions. A NaN or infinite cell keeps whatever the arithmetic gives (a NaN key is no insight); no index
// is derived from a cell's value, and the caller guarantees 0 <= cand_of_col[j] < n_plain + G.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip/tmog_hip_abi.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kRowSlice = 2048;
constexpr int kMaxBlocks = 2048;
constexpr size_t kLdsLimit = 160 * 1024;

enum Link : int { kIdentity = 0, kExp, kInverse, kSigmoid, kSquare, kPower, kBinary, kStep, kSoftmax, kLinks };

struct LocoLinArgs {
  const void* X;               // [n][ldx] fp32 or fp64, unit column stride
  int64_t n;
  int d;
  int64_t ldx;
  const double* W;             // [d][Cm]
  const double* b;             // [Cm]
  int Cm, C, link;
  double param;
  const int32_t* cand_of_col;  // [d] candidate of a column: plain < n_plain <= n_plain + group
  int n_plain, G;
  const double* gsize;         // [G]
  int kk, K, abs_mode, leave_out;
  int slice;                   // columns of the wave's LDS row slice (0: pass 2 reads the row again)
  int64_t* cols;               // [n][K]
  double* diffs;               // [n][K][C]
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The scores s[0 .. C) of the margins m[0 .. Cm): CMAX > 1 is the softmax, CMAX == 1 the scalar links.
template <int CMAX, int S>
__device__ __forceinline__ void link_scores(const LocoLinArgs& a, const double (&m)[CMAX], double (&s)[S]) {
  if constexpr (CMAX > 1) {
    double mx = m[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
      if (c < a.Cm) mx = fmax(mx, m[c]);
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      s[c] = c < a.Cm ? exp(m[c] - mx) : 0.0;
      sum += s[c];
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) s[c] = s[c] / sum;
  } else {
    const double e = m[0];
    double r;
    switch (a.link) {
      case kExp: r = exp(e); break;
      case kInverse: r = 1.0 / e; break;
      case kSigmoid:
      case kBinary: r = 1.0 / (1.0 + exp(-e)); break;
      case kSquare: r = e * e; break;
      case kPower: r = pow(fmax(e, 1e-12), 1.0 / a.param); break;
      case kStep: r = e > a.param ? 1.0 : 0.0; break;
      case kSoftmax: r = 1.0; break;
      default: r = e; break;
    }
    s[0] = a.link == kBinary ? 1.0 - r : r;
    s[1] = a.link == kBinary ? r : 0.0;
  }
}

template <int S>
__device__ __forceinline__ double pick(const double (&v)[S], int ex) {
  double r = v[0];
#pragma unroll
  for (int c = 1; c < S; ++c)
    if (c == ex) r = v[c];
  return r;
}

// A sorted list of at most kk (key, id) held one per lane, best first; key < 0 marks an empty slot.
struct TopList {
  double key;
  int id;
};

// Inserts (k, id), wave-uniform, behind every entry whose key is >= k.
__device__ __forceinline__ void top_insert(TopList& L, int lane, int kk, double k, int id) {
  const int at = __popcll(__ballot(lane < kk && L.key >= k));
  if (at >= kk) return;
  const double uk = __shfl_up(L.key, 1, 64);
  const int ui = __shfl_up(L.id, 1, 64);
  if (lane < kk && lane > at) {
    L.key = uk;
    L.id = ui;
  } else if (lane == at) {
    L.key = k;
    L.id = id;
  }
}

// Offers the candidates of the lanes with `has` (key k > 0), in lane order.
__device__ __forceinline__ void top_offer(TopList& L, int lane, int kk, bool has, double k, int id) {
  const double kth = __shfl(L.key, kk - 1, 64);
  unsigned long long mask = __ballot(has && k > kth);
  while (mask) {
    const int l = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    top_insert(L, lane, kk, __shfl(k, l, 64), __shfl(id, l, 64));
  }
}

template <typename XT, int CMAX>
__global__ void __launch_bounds__(kThreads) loco_linear_kernel(LocoLinArgs a) {
  constexpr int S = CMAX == 1 ? 2 : CMAX;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int GC = a.G * a.C;
  const size_t per_wave = ((size_t)GC + a.slice) * 8 + (((size_t)a.G * 4 + 7) & ~(size_t)7);
  double* gacc = reinterpret_cast<double*>(smem + wave * per_wave);     // [G][C]
  double* xrow = gacc + GC;                                             // [slice]
  int32_t* first = reinterpret_cast<int32_t*>(xrow + a.slice);          // [G]
  const XT* X = static_cast<const XT*>(a.X);

  for (int64_t rec = (int64_t)blockIdx.x * kWaves + wave; rec < a.n; rec += (int64_t)gridDim.x * kWaves) {
    const XT* xr = X + rec * a.ldx;
    for (int i = lane; i < GC; i += 64) gacc[i] = 0.0;
    for (int i = lane; i < a.G; i += 64) first[i] = -1;

    // ---- pass 1: the base margin
    double m[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) m[c] = 0.0;
    for (int j0 = 0; j0 < a.d; j0 += 64) {
      const int j = j0 + lane;
      const double x = j < a.d ? (double)xr[j] : 0.0;
      if (a.slice) xrow[j] = x;                       // slice is d rounded up to 64
      if (x != 0.0) {
        const double* w = a.W + (size_t)j * a.Cm;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < a.Cm) m[c] += w[c] * x;
      }
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      for (int off = 32; off > 0; off >>= 1) m[c] += __shfl_xor(m[c], off, 64);
      m[c] = c < a.Cm ? a.b[c] + m[c] : 0.0;
    }
    int ex = a.C == 2 ? 1 : 0;
    if (a.C > 2) {                                    // the predicted class: the first largest margin
      double best = m[0];
#pragma unroll
      for (int c = 1; c < CMAX; ++c)
        if (c < a.Cm && m[c] > best) {
          best = m[c];
          ex = c;
        }
    }
    double s0[S];
    link_scores<CMAX, S>(a, m, s0);
    wave_sync();

    auto xval = [&](int j) { return a.slice ? xrow[j] : (double)xr[j]; };
    // the change of zeroing what moves the margin by -t
    auto change = [&](const double(&t)[CMAX], double(&ch)[S]) {
      double mp[CMAX], sp[S];
#pragma unroll
      for (int c = 0; c < CMAX; ++c) mp[c] = m[c] - t[c];
      link_scores<CMAX, S>(a, mp, sp);
#pragma unroll
      for (int c = 0; c < S; ++c) ch[c] = s0[c] - sp[c];
    };
    auto column_change = [&](int j, double x, double(&t)[CMAX], double(&ch)[S]) {
      const double* w = a.W + (size_t)j * a.Cm;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) t[c] = c < a.Cm ? w[c] * x : 0.0;
      change(t, ch);
    };
    auto group_change = [&](int g, double(&ch)[S]) {
      if (a.leave_out) {
        double t[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) t[c] = c < a.Cm ? gacc[g * a.C + c] : 0.0;
        change(t, ch);
      } else {
        const double gs = a.gsize[g];
#pragma unroll
        for (int c = 0; c < S; ++c) ch[c] = c < a.C ? gacc[g * a.C + c] / gs : 0.0;
      }
    };

    // ---- pass 2: candidates
    TopList pos{-1.0, -1}, neg{-1.0, -1};
    for (int j0 = 0; j0 < a.d; j0 += 64) {
      const int j = j0 + lane;
      const double x = j < a.d ? xval(j) : 0.0;
      const bool nz = x != 0.0;
      double t[CMAX], ch[S];
      int cand = -1;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) t[c] = 0.0;
#pragma unroll
      for (int c = 0; c < S; ++c) ch[c] = 0.0;
      if (nz) {
        cand = a.cand_of_col[j];
        column_change(j, x, t, ch);
      }
      const bool plain = nz && cand < a.n_plain, grouped = nz && cand >= a.n_plain;
      const double v = pick(ch, ex);
      top_offer(pos, lane, a.kk, plain && v > 0.0, v, j);
      top_offer(neg, lane, a.kk, plain && v < 0.0, -v, j);
      unsigned long long pending = __ballot(grouped);
      while (pending) {                               // the distinct groups of this chunk
        const int leader = __ffsll((long long)pending) - 1;
        const int g = __shfl(cand, leader, 64) - a.n_plain;
        const unsigned long long members = __ballot(grouped && cand - a.n_plain == g);
        double sum[S];
#pragma unroll
        for (int c = 0; c < S; ++c) sum[c] = 0.0;
        for (unsigned long long rem = members; rem; rem &= rem - 1) {
          const int l = __ffsll((long long)rem) - 1;
#pragma unroll
          for (int c = 0; c < S; ++c) {
            const double mine = a.leave_out ? (c < CMAX ? t[c < CMAX ? c : 0] : 0.0) : ch[c];   // t is [CMAX]
            if (c < a.C) sum[c] += __shfl(mine, l, 64);
          }
        }
        if (lane == leader) {
#pragma unroll
          for (int c = 0; c < S; ++c)
            if (c < a.C) gacc[g * a.C + c] += sum[c];
          if (first[g] < 0) first[g] = j;
        }
        pending &= ~members;
      }
      wave_sync();
    }
    for (int g0 = 0; g0 < a.G; g0 += 64) {
      const int g = g0 + lane;
      const bool has = g < a.G && first[g] >= 0;
      double ch[S];
#pragma unroll
      for (int c = 0; c < S; ++c) ch[c] = 0.0;
      if (has) group_change(g, ch);
      const double v = pick(ch, ex);
      top_offer(pos, lane, a.kk, has && v > 0.0, v, a.d + g);
      top_offer(neg, lane, a.kk, has && v < 0.0, -v, a.d + g);
    }

    // ---- merge by rank and write
    const int P = __popcll(__ballot(lane < a.kk && pos.key > 0.0));
    const int Nn = __popcll(__ballot(lane < a.kk && neg.key > 0.0));
    int rpos = lane, rneg = a.abs_mode ? lane : P;
    for (int l = 0; l < a.kk; ++l) {
      const double pk = __shfl(pos.key, l, 64), nk = __shfl(neg.key, l, 64);
      if (a.abs_mode) {
        rpos += l < Nn && nk > pos.key;               // positives first on an equal key
        rneg += l < P && pk >= neg.key;
      } else {                                        // negatives by v descending, the earlier first on a tie
        rneg += l < Nn && (nk < neg.key || (nk == neg.key && l < lane));
      }
    }
    int64_t* cols = a.cols + rec * a.K;
    double* diffs = a.diffs + rec * a.K * a.C;
    auto emit = [&](int rank, int id) {
      double t[CMAX], ch[S];
      int col = id;
      if (id < a.d) {
        column_change(id, xval(id), t, ch);
      } else {
        group_change(id - a.d, ch);
        col = first[id - a.d];
      }
      cols[rank] = col;
#pragma unroll
      for (int c = 0; c < S; ++c)
        if (c < a.C) diffs[(size_t)rank * a.C + c] = ch[c];
    };
    if (lane < P && rpos < a.K) emit(rpos, pos.id);
    if (lane < Nn && rneg < a.K) emit(rneg, neg.id);
    for (int r = P + Nn + lane; r < a.K; r += 64) {   // no insight
      cols[r] = -1;
      for (int c = 0; c < a.C; ++c) diffs[(size_t)r * a.C + c] = 0.0;
    }
    wave_sync();                                      // the next record clears the LDS this one read
  }
}

template <typename XT, int CMAX>
int launch(const LocoLinArgs& a, size_t lds, hipStream_t stream) {
  static const bool lds_attr =
      hipFuncSetAttribute((const void*)loco_linear_kernel<XT, CMAX>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)kLdsLimit) == hipSuccess;
  if (lds > 64 * 1024 && !lds_attr) return -3;
  const int64_t blocks = (a.n + kWaves - 1) / kWaves;
  hipLaunchKernelGGL((loco_linear_kernel<XT, CMAX>), dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)),
                     dim3(kThreads), lds, stream, a);
  return (int)hipGetLastError();
}

template <typename XT>
int launch_classes(const LocoLinArgs& a, size_t lds, hipStream_t stream) {
  if (a.Cm == 1) return launch<XT, 1>(a, lds, stream);
  if (a.Cm <= 4) return launch<XT, 4>(a, lds, stream);
  return launch<XT, 16>(a, lds, stream);
}

}  // namespace

extern "C" {

// Top-K LOCO insights of n records under the margin model link(b + W^T x): cols [n][K] (int64, -1 = no insight)
// and diffs [n][K][C] (fp64, 0 where there is no insight), K = min(abs_mode ? top_k : 2 top_k, 2 min(top_k, m)) with
// m = n_plain + G candidates, C = 2 for the binary link and Cm otherwise; every cell of both is written. X is
// [n][ldx] (fp64 when x_fp64, else fp32), cand_of_col maps a column to its candidate (plain columns 0 .. n_plain - 1
// in column order, group g to n_plain + g), gsize holds the G group sizes. All arrays in device memory. Returns -2
// for arguments outside the kernel's limits (1 <= Cm <= 16, 1 <= top_k <= 64, a known link, Cm > 1 only with the
// softmax), -3 when the group state of a workgroup does not fit the LDS.
int tmog_hip_loco_linear(const void* X, int x_fp64, int64_t n, int d, int64_t ldx, const double* W, const double* b,
                         int Cm, int link, double link_param, const int32_t* cand_of_col, int n_plain, int G,
                         const double* gsize, int top_k, int abs_mode, int leave_out, int64_t* cols, double* diffs,
                         hipStream_t stream) {
  if (Cm < 1 || Cm > 16 || top_k < 1 || top_k > 64 || link < 0 || link >= kLinks || d < 0 || n_plain < 0 || G < 0 ||
      ldx < d || (Cm > 1 && link != kSoftmax))
    return -2;
  const int64_t cands = (int64_t)n_plain + G;
  if (n == 0 || cands == 0) return 0;
  const int C = link == kBinary ? 2 : Cm;
  const int kk = (int)(top_k < cands ? top_k : cands);
  const int want = abs_mode ? top_k : 2 * top_k;
  const int K = want < 2 * kk ? want : 2 * kk;
  const size_t group_bytes = (size_t)G * C * 8 + (((size_t)G * 4 + 7) & ~(size_t)7);
  int slice = d <= kRowSlice ? (d + 63) & ~63 : 0;
  if (kWaves * (group_bytes + (size_t)slice * 8) > kLdsLimit) slice = 0;
  const size_t lds = kWaves * (group_bytes + (size_t)slice * 8);
  if (lds > kLdsLimit) return -3;
  LocoLinArgs a{X, n, d, ldx, W, b, Cm, C, link, link_param, cand_of_col, n_plain, G, gsize, kk, K,
                abs_mode != 0, leave_out != 0, slice, cols, diffs};
  return x_fp64 ? launch_classes<double>(a, lds, stream) : launch_classes<float>(a, lds, stream);
}

}  // extern "C"
