// Weighted fp64 Grams and fp64 margins of the sparse design, for the regression learners (CDNA4, gfx950).
//
// Linear regression (normal equations) and the GLM's IRLS need G_k = A_k^T diag(w_k) A_k, A_k = [X | 1 | y_k], for K
// weight columns. On a wide, mostly-zero X (ops/linear.py SparseDesign: dense block Xd [N][dd], sparse block Xs as CSR
// plus segmented CSC) the dense wgram_kernel (stats_kernels.hip) multiplies zeros; here the Gram is taken from the
// non-zeros. With E_k = [Xd | 1 | y_k] (the "dense side", De = dd + 1 (+ 1) columns) G_k has three blocks: E^T W E is
// the caller's (tmog_hip_wgram on Xd); sparse_wgram_kernel and sparse_wgram_fold_kernel write Xs^T W [Xs | E], that is
// every row and column of G that belongs to a sparse column. Positions: a row of that block is [ds sparse | De dense
// side], `pos` maps a position to its row / column of G (the original column order).
//
//   item      A run of `nslice` CSC segments (at most 4096 pairs each) of one sparse column j; one wave owns it and an
//             LDS accumulator acc [KW][wp] doubles of its own (a workgroup is one wave, so waves never share one).
//   rows      The wave loads 64 of the item's pairs (r, v_j) at once, one a lane, with row_ptr[r], row_ptr[r + 1] and
//             the KW weights w_k[r] (and y_k[r]); they are read back lane by lane as wave-uniform values. Row r's
//             elements are its CSR pairs (c, v_c) followed by E[r, :]; the lanes stride over them and element `pos`
//             adds (w_k v_j) * value into acc[k][pos], KW weight columns per index read. Only pos >= j (the upper
//             triangle; the dense side lies above every sparse column) inside the pass's range [c0, c0 + wp).
//             kRows rows are in flight: their element loads are issued together, then added row by row.
//   no atomic A CSR row holds a column once and a wave adds one row at a time, so the lanes of an addition hit distinct
//             words; rows follow each other in program order (LDS executes a wave's accesses in order; a wave-level
//             fence keeps the compiler from moving them). No fp64 atomics, in LDS or in memory.
//   numbers   X is fp32 widened to fp64, w and y are fp64: a term is fma(w v_j, v_c, acc), the products and sums of
//             the dense kernel.
//   partials  A finished item writes acc to part [item][KW][wp]; the fold kernel adds a column's items in item order
//             and writes G[j][p] and G[p][j] for every position p >= j of the range, so each sparse row and column
//             of G is written in full (a column without pairs has no item and folds to zeros) and G is symmetric
//             bit for bit. The caller sizes `nslice` so that part stays within kPartBytes; the buffer is reused by
//             every chunk of KW weights and every column range, in stream order.
//   LDS       acc is KW * wp * 8 bytes a wave: KW = 4 and wp <= kWidthMax = 2048 is 64 KB, two waves on a CU's 160 KB
//             at the widest, three at the text configuration's 1352 + 10 columns. A wider block runs in column ranges
//             of wp positions (elements outside the range are skipped, the row walk is repeated). The dense side costs
//             every pair De additions: dd <= kDdMax = 254 keeps it to four lane trips; past it the dense Gram is the
//             better tool and the caller uses it.
//
// sparse_margin_f64_kernel: eta [N][P] = Xs B_s + Xd B_d + b0 in fp64 (B fp64), the IRLS margins without an fp64 copy
// of X. Lanes as in sparse_lr_kernel: (row slot) x (problem column), PC = 16, 32 or 64 columns, P above 64 in chunks
// on blockIdx.y. A row's pairs are added in CSR order, then the dense columns in order, then b0: a fixed order. Past
// its own end a row's pairs are (column 0, 0) and the B value is replaced by 0 before the fma, so a row of B that is
// not finite reaches only the rows that hold its column.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hip/tmog_hip_abi.h"

namespace {

constexpr int KW = 4;                        // weight columns per index read
constexpr int kWidthMax = 2048;              // positions of one pass: KW * kWidthMax * 8 = 64 KB of LDS a wave
constexpr int kDdMax = 254;                  // dense columns of the design
constexpr int kRows = 8;                     // rows of an item in flight
constexpr int64_t kPartBytes = (int64_t)128 << 20;

struct SGramArgs {
  const int64_t* seg_begin;                  // [n_seg + 1] first pair of a CSC segment
  const int32_t* csc_row;
  const float* csc_val;
  const int64_t* col_seg;                    // [ds + 1] first segment of a sparse column
  const int32_t* item_col;                   // [n_items]
  const int64_t* item_seg;                   // [n_items] first segment
  int nslice;                                // segments per item
  const int64_t* row_ptr;                    // CSR of the sparse block
  const int32_t* col;
  const float* val;
  const float* Xd;                           // [N][dd] or null
  int ds, dd, De;
  const double* W;                           // [N][ldw]
  int64_t ldw;
  const double* Y;                           // [N][ldy] or null
  int64_t ldy;
  int per_weight;
  int K, k0;                                 // weight columns k0 .. k0 + KW - 1 of K
  int c0, wp;                                // positions [c0, c0 + wp) of this pass
  double* part;                              // [n_items][KW][wp]
};

__device__ __forceinline__ int lane_i32(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ int64_t lane_i64(int64_t v, int l) {
  const uint32_t lo = (uint32_t)lane_i32((int)(uint32_t)v, l), hi = (uint32_t)lane_i32((int)(v >> 32), l);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double lane_f64(double v, int l) {
  return __hiloint2double(lane_i32(__double2hiint(v), l), lane_i32(__double2loint(v), l));
}
// the accumulator is handed from lane to lane between two rows: nothing moves across this point
__device__ __forceinline__ void row_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(64) sparse_wgram_kernel(SGramArgs a) {
  extern __shared__ __attribute__((aligned(16))) double acc[];     // [KW][wp]
  const int lane = threadIdx.x;
  const int64_t item = blockIdx.x;
  const int j = a.item_col[item];
  const int lo = max(j, a.c0), hi = min(a.c0 + a.wp, a.ds + a.De);
  if (lo >= hi) return;                              // nothing of column j's rows lies in this range
  for (int i = lane; i < KW * a.wp; i += 64) acc[i] = 0.0;
  row_order();
  const int ycol = a.Y ? a.ds + a.dd + 1 : -1;
  const int64_t s0 = a.item_seg[item];
  const int64_t s1 = min(s0 + a.nslice, a.col_seg[j + 1]);
  const int64_t pb = a.seg_begin[s0], pe = a.seg_begin[s1];

  // element i of row r (pairs [ra, ra + rn) of the CSR, then the dense side): its position, -1 when it is not added
  auto load_elem = [&](int i, int r, int64_t ra, int rn, float* x) -> int {
    int pos = -1;
    *x = 1.f;
    if (i < rn) {
      pos = a.col[ra + i];
      *x = a.val[ra + i];
    } else if (i < rn + a.De) {
      const int e = i - rn;
      pos = a.ds + e;
      if (e < a.dd) *x = a.Xd[(int64_t)r * a.dd + e];
    }
    return (pos >= lo && pos < hi) ? pos : -1;
  };
  auto add_elem = [&](int pos, float x, const double* wv, const double* yk) {
    if (pos >= 0) {
      double* p = acc + (pos - a.c0);
#pragma unroll
      for (int k = 0; k < KW; ++k) p[k * a.wp] = fma(wv[k], pos == ycol ? yk[k] : (double)x, p[k * a.wp]);
    }
  };

  for (int64_t base = pb; base < pe; base += 64) {
    const int nb = (int)min((int64_t)64, pe - base);
    const bool have = lane < nb;
    const int r = have ? a.csc_row[base + lane] : 0;
    const double vj = have ? (double)a.csc_val[base + lane] : 0.0;
    const int64_t ra = a.row_ptr[r];
    const int rn = have ? (int)(a.row_ptr[r + 1] - ra) : 0;
    double wv[KW], yk[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      const int kk = min(a.k0 + k, a.K - 1);
      wv[k] = (have && a.k0 + k < a.K) ? a.W[(int64_t)r * a.ldw + kk] * vj : 0.0;
      yk[k] = a.Y ? a.Y[(int64_t)r * a.ldy + (a.per_weight ? kk : 0)] : 0.0;
    }
    for (int t = 0; t < nb; t += kRows) {
      int ur[kRows], un[kRows], pos[kRows];
      int64_t ua[kRows];
      float x[kRows];
#pragma unroll
      for (int u = 0; u < kRows; ++u) {              // the element loads of kRows rows, issued together
        const int tt = min(t + u, 63);
        ur[u] = lane_i32(r, tt);
        ua[u] = lane_i64(ra, tt);
        un[u] = t + u < nb ? lane_i32(rn, tt) : -a.De;         // past the batch: no elements at all
        pos[u] = load_elem(lane, ur[u], ua[u], un[u], &x[u]);
      }
#pragma unroll
      for (int u = 0; u < kRows; ++u) {
        const int tt = min(t + u, 63);
        double wu[KW], yu[KW];
#pragma unroll
        for (int k = 0; k < KW; ++k) {
          wu[k] = lane_f64(wv[k], tt);
          yu[k] = lane_f64(yk[k], tt);
        }
        add_elem(pos[u], x[u], wu, yu);
        row_order();
        for (int i0 = 64; i0 < un[u] + a.De; i0 += 64) {       // a row of more than 64 elements: further trips
          float xe;
          const int pe_ = load_elem(i0 + lane, ur[u], ua[u], un[u], &xe);
          add_elem(pe_, xe, wu, yu);
          row_order();
        }
      }
    }
  }
  for (int k = 0; k < KW; ++k) {
    double* out = a.part + (item * KW + k) * a.wp;
    for (int p = lo + lane; p < hi; p += 64) out[p - a.c0] = acc[k * a.wp + p - a.c0];
  }
}

// Sparse row j of G_{k0 + k}: positions p >= j of the range, the column's items added in item order; the value goes to
// G[pos[j]][pos[p]] and to its mirror. grid (ds, weights of the chunk)
__global__ void __launch_bounds__(256) sparse_wgram_fold_kernel(const double* __restrict__ part,
                                                                const int64_t* __restrict__ col_item,
                                                                const int32_t* __restrict__ pos, int ds, int De, int c0,
                                                                int wp, int k0, int D, double* __restrict__ G) {
  const int j = blockIdx.x, k = blockIdx.y;
  const int lo = max(j, c0), hi = min(c0 + wp, ds + De);
  const int64_t it0 = col_item[j], it1 = col_item[j + 1];
  double* g = G + (int64_t)(k0 + k) * D * D;
  const int64_t mj = pos[j];
  for (int p = lo + threadIdx.x; p < hi; p += 256) {
    double s = 0.0;
    for (int64_t it = it0; it < it1; ++it) s += part[(it * KW + k) * wp + p - c0];
    const int64_t mp = pos[p];
    g[mj * D + mp] = s;
    g[mp * D + mj] = s;
  }
}

constexpr int kWaves = 4;      // waves per workgroup of the margin kernel
constexpr int kU = 8;          // B row gathers in flight per wave

template <int PC>
__global__ void __launch_bounds__(64 * kWaves) sparse_margin_f64_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const float* __restrict__ val, int64_t N,
    const double* __restrict__ Bs, int ldb, const float* __restrict__ Xd, int dd, const double* __restrict__ Bd,
    const double* __restrict__ b0, int P, double* __restrict__ eta, int64_t lde) {
  constexpr int RS = 64 / PC;                      // row slots per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane / PC, pc = lane % PC;
  const int p = blockIdx.y * PC + pc;
  const bool p_ok = p < P;
  const int pl = p_ok ? p : P - 1;                 // a column that exists: loads need no guard, results are dropped
  const int64_t row = ((int64_t)blockIdx.x * kWaves + wave) * RS + slot;
  const bool row_ok = row < N;
  const int64_t ra = row_ok ? row_ptr[row] : 0;
  const int nrow = row_ok ? (int)(row_ptr[row + 1] - ra) : 0;
  int nmax = nrow;                                 // the longest row of the wave's slots
  if (RS >= 2) nmax = max(nmax, __shfl_xor(nmax, 32, 64));
  if (RS >= 4) nmax = max(nmax, __shfl_xor(nmax, 16, 64));
  double acc = 0.0;
  for (int base = 0; base < nmax; base += PC) {
    const bool have = base + pc < nrow;
    const int my_i = have ? col[ra + base + pc] : 0;
    const float my_v = have ? val[ra + base + pc] : 0.f;
    const int n = min(PC, nmax - base);            // wave-uniform
    for (int t = 0; t < n; t += kU) {
      float xs[kU];
      double bv[kU];
#pragma unroll
      for (int k = 0; k < kU; ++k) {
        const int src = slot * PC + t + k;         // t + k < PC: PC is a multiple of kU
        const int i = __shfl(my_i, src, 64);
        xs[k] = __shfl(my_v, src, 64);
        bv[k] = Bs[(int64_t)i * ldb + pl];
      }
#pragma unroll
      for (int k = 0; k < kU; ++k) acc = fma((double)xs[k], base + t + k < nrow ? bv[k] : 0.0, acc);
    }
  }
  if (!(row_ok && p_ok)) return;
  double dacc = 0.0;
  const float* xrow = Xd + row * (int64_t)dd;
  for (int k = 0; k < dd; ++k) dacc = fma((double)xrow[k], Bd[(int64_t)k * ldb + pl], dacc);
  eta[row * lde + p] = (acc + dacc) + (b0 ? b0[p] : 0.0);
}

}  // namespace

extern "C" {

int tmog_hip_sparse_wgram_kw() { return KW; }

int tmog_hip_sparse_wgram_width_max() { return kWidthMax; }

int tmog_hip_sparse_wgram_dd_max() { return kDdMax; }

int64_t tmog_hip_sparse_wgram_part_bytes() { return kPartBytes; }

int tmog_hip_sparse_wgram(const int64_t* seg_begin, const int32_t* csc_row, const float* csc_val,
                          const int64_t* col_seg, const int32_t* item_col, const int64_t* item_seg,
                          const int64_t* col_item, int64_t n_items, int nslice, const int64_t* row_ptr,
                          const int32_t* col, const float* val, int64_t N, int ds, const float* Xd, int dd,
                          const double* W, int64_t ldw, int K, const double* Y, int64_t ldy, int per_weight,
                          const int32_t* pos, int wp, double* G, hipStream_t stream) {
  const int De = dd + 1 + (Y ? 1 : 0);
  if (N <= 0 || ds <= 0 || K <= 0 || dd < 0 || dd > kDdMax || (dd > 0 && Xd == nullptr)) return -2;
  if (wp <= 0 || wp > kWidthMax || n_items < 0 || nslice <= 0) return -2;
  const int64_t bytes = n_items * KW * (int64_t)wp * (int64_t)sizeof(double);
  if (bytes > kPartBytes) return -2;
  double* part = nullptr;
  if (n_items > 0) {
    hipError_t e = hipMallocAsync((void**)&part, bytes, stream);
    if (e != hipSuccess) return (int)e;
  }
  SGramArgs a{seg_begin, csc_row, csc_val, col_seg, item_col, item_seg, nslice, row_ptr, col, val, Xd, ds, dd, De,
              W, ldw, Y, ldy, per_weight, K, 0, 0, wp, part};
  const int D = ds + De;
  for (int k0 = 0; k0 < K; k0 += KW) {
    for (int c0 = 0; c0 < D; c0 += wp) {
      a.k0 = k0;
      a.c0 = c0;
      if (n_items > 0)
        hipLaunchKernelGGL(sparse_wgram_kernel, dim3((unsigned)n_items), dim3(64), (size_t)KW * wp * sizeof(double),
                           stream, a);
      hipLaunchKernelGGL(sparse_wgram_fold_kernel, dim3((unsigned)ds, (unsigned)std::min(KW, K - k0)), dim3(256), 0,
                         stream, part, col_item, pos, ds, De, c0, wp, k0, D, G);
    }
  }
  if (part) (void)hipFreeAsync(part, stream);
  return (int)hipGetLastError();
}

int tmog_hip_sparse_margin_f64(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N,
                               const double* Bs, int ldb, const float* Xd, int dd, const double* Bd, const double* b0,
                               int P, double* eta, int64_t lde, hipStream_t stream) {
  if (N <= 0 || P <= 0 || dd < 0 || (dd > 0 && (Xd == nullptr || Bd == nullptr))) return -2;
  const int pc = P <= 16 ? 16 : P <= 32 ? 32 : 64;
  const int64_t groups = (N + 64 / pc - 1) / (64 / pc);
  const dim3 grid((unsigned)((groups + kWaves - 1) / kWaves), (unsigned)((P + pc - 1) / pc));
#define TM_SMG(PCV)                                                                                             \
  hipLaunchKernelGGL((sparse_margin_f64_kernel<PCV>), grid, dim3(64 * kWaves), 0, stream, row_ptr, col, val, N, \
                     Bs, ldb, Xd, dd, Bd, b0, P, eta, lde)
  if (pc == 16) TM_SMG(16);
  else if (pc == 32) TM_SMG(32);
  else TM_SMG(64);
#undef TM_SMG
  return (int)hipGetLastError();
}

}  // extern "C"
