// The scaffold of the forest explanation kernels (shap_kernels.hip, loco_kernels.hip, pd_kernels.hip,
// pd_pair_kernels.hip), written once. A workgroup of kTileThreads lanes owns a tile of rows: it zeroes an int64 fixed-point tile in LDS, stages
// the bins of the forest's used columns of its rows next to it, accumulates with 64-bit LDS integer atomics and at
// the end converts the tile to fp64 and writes it with plain stores. The launchers size the tile from the LDS
// budget by one rule and start the kernel through one function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tmog {

constexpr int kTileThreads = 512;
constexpr int kTileMaxRows = 64;
constexpr size_t kTileLdsLimit = 160 * 1024;
constexpr size_t kTileLdsShare = 80 * 1024;   // two workgroups per CU while the tile stays >= 16 rows

// What every kernel of the family is told about the rows and its tile; each embeds it in its own arguments.
struct RowTile {
  const uint8_t* Xb;         // [.][F] binned matrix
  int F;
  int64_t n;                 // rows to serve: row_list[0 .. n), or rows 0 .. n - 1 when row_list is null
  const int32_t* row_list;
  int U;
  const int32_t* used;       // [U] the forest's distinct split columns, sorted
  int C;                     // output columns
  double scale;              // the power of two of the fixed point
  int missing_bin;
  int tile_rows;
  int ustride;               // bytes per staged row (ustride_of(U))
};

// The tile of workgroup blockIdx.x: its first row (>= n: nothing to do) and how many rows it holds.
__device__ __forceinline__ int64_t tile_first_row(const RowTile& t) { return (int64_t)blockIdx.x * t.tile_rows; }
__device__ __forceinline__ int tile_row_count(const RowTile& t, int64_t blk0) {
  return (int)min((int64_t)t.tile_rows, t.n - blk0);
}

__device__ __forceinline__ void zero_tile(unsigned long long* acc, size_t count) {
  for (size_t i = threadIdx.x; i < count; i += kTileThreads) acc[i] = 0ull;
}

// sbin[r][k] = the bin of used column k of the tile's row r, one wave per row
__device__ __forceinline__ void stage_used_bins(const RowTile& t, int64_t blk0, int nrow, uint8_t* sbin) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < nrow; r += kTileThreads / 64) {
    const int64_t row = t.row_list ? t.row_list[blk0 + r] : (blk0 + r);
    const uint8_t* src = t.Xb + row * (int64_t)t.F;
    for (int k = lane; k < t.U; k += 64) sbin[(size_t)r * t.ustride + k] = src[t.used[k]];
  }
}

// A fixed-point sum as fp64 (inv = 1 / scale), and a run of them
__device__ __forceinline__ double tile_value(unsigned long long acc, double inv) {
  return (double)(long long)acc * inv;
}
__device__ __forceinline__ void store_tile_fp64(double* out, const unsigned long long* acc, size_t count,
                                                double inv) {
  for (size_t i = threadIdx.x; i < count; i += kTileThreads) out[i] = tile_value(acc[i], inv);
}

// ---------------------------------------------------------------------------------------------------- launchers
inline int ustride_of(int U) { return (U + 3) & ~3; }

// The tile-size rule: bytes(rows) is the LDS a tile of `rows` rows takes. Halve from kTileMaxRows down to 16 rows
// while the tile exceeds the two-workgroup share, then further down to one row while it exceeds the limit (the
// caller has refused a one-row tile beyond the limit).
template <class Bytes>
int pick_tile_rows(Bytes bytes) {
  int rows = kTileMaxRows;
  while (rows > 16 && bytes(rows) > kTileLdsShare) rows >>= 1;
  while (rows > 1 && bytes(rows) > kTileLdsLimit) rows >>= 1;
  return rows;
}

// Starts Kernel on `blocks` row tiles x `chunks` with `lds` bytes of dynamic LDS. More than 64 KiB needs the
// function attribute, set once per process and kernel (the static below is Kernel's own): -3 when that failed,
// -4 when the grid does not fit, else hipGetLastError().
template <auto Kernel, class... Args>
int launch_lds(int64_t blocks, int64_t chunks, size_t lds, hipStream_t stream, Args... args) {
  static const bool lds_attr = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)kTileLdsLimit) == hipSuccess;
  if (lds > 64 * 1024 && !lds_attr) return -3;
  if (blocks > 0x7FFFFFFF || chunks > 65535) return -4;
  hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks, (unsigned)chunks), dim3(kTileThreads), lds, stream, args...);
  return (int)hipGetLastError();
}

}  // namespace tmog
