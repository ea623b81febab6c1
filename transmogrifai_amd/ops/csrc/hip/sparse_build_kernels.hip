// CSR and segmented CSC of a dense device matrix, built without atomics and without a sort (CDNA4, gfx950).
//
// ops/linear.py SparseDesign and ops/lda.py DocTermCSR keep the non-zeros of a wide, mostly-zero matrix X [N][d] as a
// CSR (row-major, columns ascending within a row) and a CSC (column-major, rows ascending within a column). Both
// orders are fixed, so every non-zero's two positions are computed, not claimed: counts first, scans of the counts,
// then one pass that writes each entry at its place. The matrix is cut into row tiles of kTR = 64 rows and column
// groups of 64 columns (one wave, a lane per column: a wave's load of a row is one coalesced 256-byte read, 512 in fp64).
//
//   count     count_kernel: a lane owns one column of one tile, walks the tile's rows (kU loads in flight) with the
//             counter in a register and writes tile_cnt [T][d] -- a byte, the count is at most 64. walk_kernel<false>
//             folds the table into nz [d]: a workgroup per column group, its 16 waves each summing a run of tiles,
//             the 16 partials added in wave order. Python decides on nz which columns are kept (smap) and scans the
//             kept columns' counts into col_start on the host: d numbers, the build's one synchronisation.
//   offsets   walk_kernel<true> walks the same table again and writes tile_off [T][d], a kept column's non-zeros in
//             the tiles above: the start of tile t inside CSC column j is col_start[j] + tile_off[t][c].
//             tile_nnz_kernel (a wave per tile) adds a tile's kept counts and tile_scan_kernel (one workgroup) scans
//             them into tile_start [T + 1], the CSR position of a tile's first entry.
//   fill      fill_kernel, one workgroup of 4 waves per row tile, waves assigned to column groups. Sweep 1: per (row,
//             group) the popcount of the ballot "kept column and non-zero" goes into an LDS table [64][groups] of
//             16-bit counts (32 KB at d = 16384: the width limit); a thread per row scans its row into exclusive
//             prefixes and a row total, the totals are scanned into row starts and written as row_ptr. Sweep 2: a
//             wave takes a group and walks the rows in ascending order, each lane keeping its column's CSC cursor in a
//             register. A non-zero's CSR position is tile start + row start + group prefix + rank in the ballot; its
//             CSC position is the cursor, then incremented. Column order within a row and row order within a column
//             fall out of the walk. X is read three times in all (count, sweep 1, sweep 2).
//   row sums  row_sum_kernel: a thread per row adds the row's fp32 values in fp64, in column order.
//
// A value is a non-zero iff its bits below the sign are not all zero: x != 0 in the source type, NaN and denormals
// included, -0.0 not. It is stored as its fp32 bits, an fp64 source rounded to nearest first (so an fp64 entry below
// the fp32 range is an entry of value 0.0f).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip/tmog_hip_abi.h"

namespace {

constexpr int kTR = TMOG_SPARSE_BUILD_TR;        // rows per tile
constexpr int kDMax = TMOG_SPARSE_BUILD_DMAX;    // columns: the LDS table of fill_kernel is kTR x (kDMax / 64) x 2 B
constexpr int kU = 8;                            // row loads in flight per lane
constexpr int kFillWaves = 4;
constexpr int kWalkWaves = 16;
constexpr int kScanThreads = 1024;

static_assert(kTR == 64 && kTR % kU == 0, "a tile's column count fits a byte and a row per lane of wave 0");

template <typename B>
__device__ __forceinline__ bool nonzero(B b) { return (B)(b << 1) != 0; }

__device__ __forceinline__ float value_f32(uint32_t b) { return __uint_as_float(b); }
__device__ __forceinline__ float value_f32(uint64_t b) { return (float)__longlong_as_double((long long)b); }

// kU rows of one column, r0 .. r0 + kU - 1 of `rows`; 0 past the end or when the lane has no column to read
template <typename B>
__device__ __forceinline__ void load_rows(const B* __restrict__ x, int64_t ldx, int r0, int rows, bool on, B (&v)[kU]) {
#pragma unroll
  for (int u = 0; u < kU; ++u) v[u] = (on && r0 + u < rows) ? x[(int64_t)(r0 + u) * ldx] : (B)0;
}

template <typename B>
__global__ void __launch_bounds__(256) count_kernel(const B* __restrict__ X, int64_t ldx, int64_t N, int d,
                                                    uint8_t* __restrict__ tile_cnt) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= d) return;
  const int64_t row0 = (int64_t)blockIdx.x * kTR;
  const int rows = (int)min((int64_t)kTR, N - row0);
  const B* x = X + row0 * ldx + c;
  int n = 0;
  for (int r0 = 0; r0 < rows; r0 += kU) {
    B v[kU];
    load_rows(x, ldx, r0, rows, true, v);
#pragma unroll
    for (int u = 0; u < kU; ++u) n += nonzero(v[u]) ? 1 : 0;
  }
  tile_cnt[(int64_t)blockIdx.x * d + c] = (uint8_t)n;
}

// A workgroup per column group, wave w the tiles [w * chunk, (w + 1) * chunk). SCAN false: nz[c] = the column's sum.
// SCAN true: tile_off[t][c] = the sum over the tiles above t, for the kept columns.
template <bool SCAN>
__global__ void __launch_bounds__(64 * kWalkWaves) walk_kernel(const uint8_t* __restrict__ tile_cnt, int64_t T, int d,
                                                               const int32_t* __restrict__ smap,
                                                               int64_t* __restrict__ nz,
                                                               int32_t* __restrict__ tile_off) {
  __shared__ int32_t part[kWalkWaves][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  bool live = c < d;
  if (SCAN && live) live = smap[c] >= 0;
  const int64_t chunk = (T + kWalkWaves - 1) / kWalkWaves;
  const int64_t t0 = min(T, (int64_t)w * chunk), t1 = min(T, t0 + chunk);
  const uint8_t* cnt = tile_cnt + c;
  int32_t s = 0;                                   // at most N < 2^31
  if (live) {
    for (int64_t t = t0; t < t1; t += kU) {
      int32_t v[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) v[u] = t + u < t1 ? (int32_t)cnt[(t + u) * d] : 0;
#pragma unroll
      for (int u = 0; u < kU; ++u) s += v[u];
    }
  }
  part[w][lane] = s;
  __syncthreads();
  if (!SCAN) {
    if (w == 0 && live) {
      int64_t total = 0;
      for (int k = 0; k < kWalkWaves; ++k) total += part[k][lane];
      nz[c] = total;
    }
  } else if (live) {
    int32_t run = 0;
    for (int k = 0; k < w; ++k) run += part[k][lane];
    int32_t* off = tile_off + c;
    for (int64_t t = t0; t < t1; t += kU) {
      int32_t v[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) v[u] = t + u < t1 ? (int32_t)cnt[(t + u) * d] : 0;
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (t + u < t1) off[(t + u) * d] = run;
        run += v[u];
      }
    }
  }
}

// tile_nnz[t] = the kept columns' counts of tile t: a wave per tile
__global__ void __launch_bounds__(256) tile_nnz_kernel(const uint8_t* __restrict__ tile_cnt, int64_t T, int d,
                                                       const int32_t* __restrict__ smap,
                                                       int32_t* __restrict__ tile_nnz) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;                              // a whole wave
  const uint8_t* cnt = tile_cnt + t * d;
  int32_t s = 0;
  for (int c = lane; c < d; c += 64) s += smap[c] >= 0 ? (int32_t)cnt[c] : 0;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) tile_nnz[t] = s;
}

// tile_start = exclusive scan of tile_nnz, tile_start[T] the total: one workgroup, a run of tiles per thread
__global__ void __launch_bounds__(kScanThreads) tile_scan_kernel(const int32_t* __restrict__ tile_nnz, int64_t T,
                                                                 int64_t* __restrict__ tile_start) {
  __shared__ int64_t part[kScanThreads];
  const int64_t per = (T + kScanThreads - 1) / kScanThreads;
  const int64_t t0 = min(T, (int64_t)threadIdx.x * per), t1 = min(T, t0 + per);
  int64_t s = 0;
  for (int64_t t = t0; t < t1; ++t) s += tile_nnz[t];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int i = 0; i < kScanThreads; ++i) {
      const int64_t v = part[i];
      part[i] = run;
      run += v;
    }
    tile_start[T] = run;
  }
  __syncthreads();
  int64_t run = part[threadIdx.x];
  for (int64_t t = t0; t < t1; ++t) {
    tile_start[t] = run;
    run += tile_nnz[t];
  }
}

template <typename B>
__global__ void __launch_bounds__(64 * kFillWaves) fill_kernel(
    const B* __restrict__ X, int64_t ldx, int64_t N, int d, const int32_t* __restrict__ smap,
    const int64_t* __restrict__ col_start, const int32_t* __restrict__ tile_off,
    const int64_t* __restrict__ tile_start, int64_t* __restrict__ row_ptr, int32_t* __restrict__ col,
    float* __restrict__ val, int32_t* __restrict__ csc_row, float* __restrict__ csc_val,
    float* __restrict__ csc_val_sq, int64_t* __restrict__ csc_pos) {
  extern __shared__ uint16_t tab[];                // [kTR][gp]: counts, then exclusive prefixes along a row
  __shared__ int32_t row_start[kTR + 1];           // row totals, then their exclusive scan
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int G = (d + 63) / 64, gp = G | 1;
  const int64_t tile = blockIdx.x;
  const int64_t row0 = tile * kTR;
  const int rows = (int)min((int64_t)kTR, N - row0);
  const B* xt = X + row0 * ldx;

  // sweep 1: non-zeros of the kept columns per (row, group)
  for (int g = w; g < G; g += kFillWaves) {
    const int c = g * 64 + lane;
    const bool kept = c < d && smap[c] >= 0;
    for (int r0 = 0; r0 < rows; r0 += kU) {
      B v[kU];
      load_rows(xt + c, ldx, r0, rows, kept, v);
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const unsigned long long m = __ballot(kept && nonzero(v[u]));
        if (lane == u && r0 + u < rows) tab[(r0 + u) * gp + g] = (uint16_t)__popcll(m);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kTR) {
    int32_t run = 0;
    if ((int)threadIdx.x < rows) {
      uint16_t* row = tab + threadIdx.x * gp;
      for (int g = 0; g < G; ++g) {
        const int32_t v = row[g];
        row[g] = (uint16_t)run;                    // below d <= kDMax
        run += v;
      }
    }
    row_start[threadIdx.x] = run;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t run = 0;
    for (int r = 0; r < kTR; ++r) {
      const int32_t v = row_start[r];
      row_start[r] = run;
      run += v;
    }
    row_start[kTR] = run;
  }
  __syncthreads();
  const int64_t base = tile_start[tile];
  if ((int)threadIdx.x < rows) row_ptr[row0 + threadIdx.x + 1] = base + row_start[threadIdx.x + 1];
  if (tile == 0 && threadIdx.x == 0) row_ptr[0] = 0;

  // sweep 2: every non-zero to its CSR and its CSC position
  for (int g = w; g < G; g += kFillWaves) {
    const int c = g * 64 + lane;
    const int j = c < d ? smap[c] : -1;
    const bool kept = j >= 0;
    int64_t cur = kept ? col_start[j] + tile_off[tile * d + c] : 0;
    for (int r0 = 0; r0 < rows; r0 += kU) {
      B v[kU];
      load_rows(xt + c, ldx, r0, rows, kept, v);
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const bool hit = kept && nonzero(v[u]);    // false past the tile's rows: those loads gave 0
        const unsigned long long m = __ballot(hit);
        if (hit) {
          const int r = r0 + u;
          const int rank = __popcll(m & ((1ull << lane) - 1ull));
          const int64_t p = base + row_start[r] + tab[r * gp + g] + rank;
          const float f = value_f32(v[u]);
          col[p] = j;
          val[p] = f;
          csc_row[cur] = (int32_t)(row0 + r);
          if (csc_val) csc_val[cur] = f;
          if (csc_val_sq) csc_val_sq[cur] = f * f;
          if (csc_pos) csc_pos[cur] = p;
          ++cur;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(256) row_sum_kernel(const int64_t* __restrict__ row_ptr,
                                                      const float* __restrict__ val, int64_t N,
                                                      double* __restrict__ row_sum) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double s = 0.0;
  for (int64_t p = row_ptr[i], e = row_ptr[i + 1]; p < e; ++p) s += (double)val[p];
  row_sum[i] = s;
}

bool shape_ok(const void* X, int64_t ldx, int64_t N, int d) {
  return X != nullptr && N >= 1 && N < ((int64_t)1 << 31) && d >= 1 && d <= kDMax && ldx >= 0;
}

}  // namespace

extern "C" {

int tmog_hip_sparse_build_count(const void* X, int f64, int64_t ldx, int64_t N, int d, uint8_t* tile_cnt, int64_t* nz,
                                hipStream_t stream) {
  if (!shape_ok(X, ldx, N, d) || tile_cnt == nullptr || nz == nullptr) return -2;
  const int64_t T = (N + kTR - 1) / kTR;
  const dim3 grid((unsigned)T, (unsigned)((d + 255) / 256));
  if (f64)
    hipLaunchKernelGGL(count_kernel<uint64_t>, grid, dim3(256), 0, stream, (const uint64_t*)X, ldx, N, d, tile_cnt);
  else
    hipLaunchKernelGGL(count_kernel<uint32_t>, grid, dim3(256), 0, stream, (const uint32_t*)X, ldx, N, d, tile_cnt);
  hipLaunchKernelGGL(walk_kernel<false>, dim3((unsigned)((d + 63) / 64)), dim3(64 * kWalkWaves), 0, stream, tile_cnt,
                     T, d, (const int32_t*)nullptr, nz, (int32_t*)nullptr);
  return (int)hipGetLastError();
}

int tmog_hip_sparse_build_fill(const void* X, int f64, int64_t ldx, int64_t N, int d, const int32_t* smap,
                               const int64_t* col_start, const uint8_t* tile_cnt, int32_t* tile_off,
                               int32_t* tile_nnz, int64_t* tile_start, int64_t* row_ptr, int32_t* col, float* val,
                               int32_t* csc_row, float* csc_val, float* csc_val_sq, int64_t* csc_pos,
                               double* row_sum, hipStream_t stream) {
  if (!shape_ok(X, ldx, N, d) || smap == nullptr || col_start == nullptr || tile_cnt == nullptr ||
      tile_off == nullptr || tile_nnz == nullptr || tile_start == nullptr || row_ptr == nullptr)
    return -2;
  const int64_t T = (N + kTR - 1) / kTR;
  const int G = (d + 63) / 64;
  hipLaunchKernelGGL(walk_kernel<true>, dim3((unsigned)G), dim3(64 * kWalkWaves), 0, stream, tile_cnt, T, d, smap,
                     (int64_t*)nullptr, tile_off);
  hipLaunchKernelGGL(tile_nnz_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, stream, tile_cnt, T, d, smap,
                     tile_nnz);
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, tile_nnz, T, tile_start);
  const size_t lds = (size_t)kTR * (G | 1) * sizeof(uint16_t);
  if (f64)
    hipLaunchKernelGGL(fill_kernel<uint64_t>, dim3((unsigned)T), dim3(64 * kFillWaves), lds, stream,
                       (const uint64_t*)X, ldx, N, d, smap, col_start, tile_off, tile_start, row_ptr, col, val,
                       csc_row, csc_val, csc_val_sq, csc_pos);
  else
    hipLaunchKernelGGL(fill_kernel<uint32_t>, dim3((unsigned)T), dim3(64 * kFillWaves), lds, stream,
                       (const uint32_t*)X, ldx, N, d, smap, col_start, tile_off, tile_start, row_ptr, col, val,
                       csc_row, csc_val, csc_val_sq, csc_pos);
  if (row_sum != nullptr)
    hipLaunchKernelGGL(row_sum_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, row_ptr, val, N,
                       row_sum);
  return (int)hipGetLastError();
}

}  // extern "C"
