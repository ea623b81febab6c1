// One objective pass of P multilayer perceptrons over a sparse design in one kernel (CDNA4, gfx950).
//
// OpMultilayerPerceptronClassifier on a wide, mostly-zero matrix (hashed text, pivots): the matrix is ops/linear.py
// SparseDesign (CSR of the sparse columns, a small dense block Xd [N][nd]); behind it the network is small -- one or two
// sigmoid hidden layers of width <= 64 and a softmax over K <= 16 classes -- so everything after the first layer fits
// in LDS and registers. sparse_mlp_kernel takes a 16-row tile from the non-zeros through every layer, the weighted
// cross-entropy and the whole backward pass. Only the first layer's dZ1 [N][P * h1] leaves the chip (with grad), for
// the X^T dZ1 product of csc_spmm_t_kernel; a value pass writes nothing per row.
//
//   work split   grid (workgroups per problem, P). A workgroup of 4 waves serves problem p = blockIdx.y: it stages
//                that problem's tail weights, zero-padded to the 16-wide MFMA tiles, in LDS once, then its waves walk
//                the 16-row tiles grid-stride, one tile per wave at a time. No workgroup barrier after the staging.
//   first layer  lanes are (row slot) x (hidden unit): H1P = 16, 32 or 64 units (h1 rounded up), 64 / H1P rows at
//                once, as sparse_lr_kernel lays out problem columns. Every non-zero (col, val) of a row reads the
//                contiguous h1 floats of W1s[p][col]; pairs are loaded H1P at a time into a register batch and
//                broadcast in groups of kU whose gathers are issued before their FMAs. Past its own end a row's
//                pairs are (column 0, 0.f) with the loaded weight replaced by 0.f. The dense block's columns are
//                added from Xd and W1d[p]. a1 = sigmoid(z1 + b1) goes to the wave's LDS tile [16][H1P + 4].
//   zero weight  a row whose weight W[row][p] is 0 (outside the fold) skips the gather and the dense block; its loss,
//                its dZ_L and its dZ1 row are set to 0, so it adds exactly 0 to every sum.
//   tail         v_mfma_f32_16x16x4_f32 throughout: a lane (c = lane & 15, q = lane >> 4) supplies A[c][q] and
//                B[q][c] of a 16x4 by 4x16 step and holds D[4q + r][c], r = 0..3 (w2v_kernels.hip). Forward: the
//                activation tile is A, 16-column blocks of the LDS weights are B; bias and sigmoid on the
//                accumulators. Softmax over the K logits of a row by cross-lane moves inside the 16 lanes that hold
//                it. Backward: dW += A_prev^T dZ and db += 1^T dZ accumulate in registers across tiles; dH = dZ W^T
//                reads the same LDS weights transposed; dZ_prev = dH a (1 - a) overwrites the activation it came from.
//   LDS          weight pitches 17 / 49 / 81 floats (the row-wise and the transposed read both spread over the
//                banks), activation pitch width + 4. 64-64-16 needs 63.8 KiB, two workgroups a CU.
//   sums         the loss and db1 add fp32 terms in fp64 per lane. The MFMA accumulators (tail dW, db) are fp32 and
//                are flushed to the wave's own fp64 partial row in global memory every kFlushTiles = 128 tiles (2048
//                rows, the chunk length of the dense path) and at the end; the first flush stores, later ones add: no
//                zero fill, no atomics. sparse_mlp_fold_kernel adds the wave rows in one fixed order, so two calls
//                on the same inputs are bitwise equal.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "hip/tmog_hip_abi.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;          // waves per workgroup
constexpr int kU = 8;              // W1s row gathers in flight per wave
constexpr int kNdMax = 128;        // dense columns served (wider blocks: the dense path is the better tool)
constexpr int kFlushTiles = 128;   // tiles between flushes of the fp32 accumulators: 2048 rows
constexpr int kDzPitch = 20;       // output dZ tile [16][16 + 4]

struct MlpArgs {
  const int64_t* row_ptr; const int32_t* col; const float* val; int64_t N;
  const float* W1s; int ds; const float* Xd; int nd; const float* W1d; const float* b1;
  const float* Wm; const float* bm;          // [P][h1][h2], [P][h2]: the second hidden layer (h2 > 0)
  const float* WL; const float* bL;          // [P][h2 or h1][K], [P][K]: the output layer
  const float* y; const float* W; int ldw; const float* wsum;
  int h1, h2, K;
  float* dZ1; int64_t ldz;
  double* part; int npart;
};

__host__ __device__ constexpr int pad_width(int w) { return w <= 0 ? 0 : w <= 16 ? 16 : w <= 32 ? 32 : 64; }
__host__ __device__ constexpr int weight_pitch(int wp) { return wp == 16 ? 17 : wp == 32 ? 49 : 81; }
// a wave's partial row: loss | db1 [H1P] | dWm [H1P][H2P] | dbm [H2P] | dWL [INL][16] | dbL [16]
__host__ __device__ constexpr int off_db1() { return 1; }
__host__ __device__ constexpr int off_dwm(int h1p) { return 1 + h1p; }
__host__ __device__ constexpr int off_dbm(int h1p, int h2p) { return off_dwm(h1p) + h1p * h2p; }
__host__ __device__ constexpr int off_dwl(int h1p, int h2p) { return off_dbm(h1p, h2p) + h2p; }
__host__ __device__ constexpr int off_dbl(int h1p, int h2p) { return off_dwl(h1p, h2p) + (h2p ? h2p : h1p) * 16; }
__host__ __device__ constexpr int n_part(int h1p, int h2p) { return off_dbl(h1p, h2p) + 16; }

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the formula of mlp_bias_sigmoid_kernel: e^-z = inf gives 0
__device__ __forceinline__ float sigmoidf(float z) { return __builtin_amdgcn_rcpf(1.f + __expf(-z)); }

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
}

// acc holds D[4q + r][c] of a 16x16 block of a [.][ld] matrix of the partial row
__device__ __forceinline__ void flush_block(f32x4& acc, double* dst, int ld, int q, int c, bool first) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double* d = dst + (4 * q + r) * ld + c;
    *d = (first ? 0.0 : *d) + (double)acc[r];
    acc[r] = 0.f;
  }
}

// acc holds the column sums in every row: row 0 leaves
__device__ __forceinline__ void flush_colsum(f32x4& acc, double* dst, int q, int c, bool first) {
  if (q == 0) dst[c] = (first ? 0.0 : dst[c]) + (double)acc[0];
  acc = f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ double fold_q(double v) {      // the four q groups in order, on every lane
  const int c = threadIdx.x & 15;
  return ((__shfl(v, c, 64) + __shfl(v, 16 + c, 64)) + __shfl(v, 32 + c, 64)) + __shfl(v, 48 + c, 64);
}

template <int H1P, int H2P, bool GRAD>
__global__ void __launch_bounds__(64 * kWaves) sparse_mlp_kernel(const MlpArgs a) {
  constexpr int RS = 64 / H1P;                    // row slots of the first layer
  constexpr int INL = H2P ? H2P : H1P;            // padded input width of the output layer
  constexpr int PM = weight_pitch(H2P);
  constexpr int P1 = H1P + 4, P2 = H2P + 4;
  constexpr int PP = H2P ? P2 : P1;               // pitch of the output layer's input tile
  constexpr int T1 = H1P / 16, T2 = H2P / 16, TL = INL / 16;
  __shared__ float sWm[H2P ? H1P * PM : 1];
  __shared__ float sWL[INL * 17];
  __shared__ float sbm[H2P ? H2P : 1];
  __shared__ float sbL[16];
  __shared__ float sA1[kWaves][16 * P1];
  __shared__ float sA2[kWaves][H2P ? 16 * P2 : 1];
  __shared__ float sDz[kWaves][16 * kDzPitch];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int p = blockIdx.y;
  const int h1 = a.h1, h2 = a.h2, K = a.K;
  const int inl = H2P ? h2 : h1;

  // ---- this problem's tail weights, zero-padded to the tiles
  if (H2P) {
    const float* Wm = a.Wm + (int64_t)p * h1 * h2;
    for (int i = threadIdx.x; i < H1P * H2P; i += 64 * kWaves) {
      const int r = i / H2P, cc = i % H2P;
      sWm[r * PM + cc] = (r < h1 && cc < h2) ? Wm[r * h2 + cc] : 0.f;
    }
    if (threadIdx.x < H2P) sbm[threadIdx.x] = (int)threadIdx.x < h2 ? a.bm[p * h2 + threadIdx.x] : 0.f;
  }
  {
    const float* WL = a.WL + (int64_t)p * inl * K;
    for (int i = threadIdx.x; i < INL * 16; i += 64 * kWaves) {
      const int r = i >> 4, cc = i & 15;
      sWL[r * 17 + cc] = (r < inl && cc < K) ? WL[r * K + cc] : 0.f;
    }
    if (threadIdx.x < 16) sbL[threadIdx.x] = (int)threadIdx.x < K ? a.bL[p * K + threadIdx.x] : 0.f;
  }
  __syncthreads();

  float* A1 = sA1[wave];
  float* A2 = sA2[wave];
  float* Dz = sDz[wave];
  float* Ap = H2P ? A2 : A1;

  // first-layer lanes
  const int slot = lane / H1P, j = lane % H1P;
  const int jl = min(j, h1 - 1);                  // a unit that exists: loads need no guard
  const float* w1col = a.W1s + (int64_t)p * a.ds * h1 + jl;
  const float* w1d = a.W1d + (int64_t)p * a.nd * h1 + jl;
  const float b1j = a.b1[p * h1 + jl];
  const float ws = a.wsum[p];
  const float bLc = sbL[c];

  double f_acc = 0.0;
  double db1[T1];
  f32x4 gWm[H2P ? T1 : 1][H2P ? T2 : 1], gbm[H2P ? T2 : 1], gWL[TL], gbL;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < T1; ++i) db1[i] = 0.0;
#pragma unroll
  for (int i = 0; i < (H2P ? T1 : 1); ++i)
#pragma unroll
    for (int k = 0; k < (H2P ? T2 : 1); ++k) gWm[i][k] = zero4;
#pragma unroll
  for (int k = 0; k < (H2P ? T2 : 1); ++k) gbm[k] = zero4;
#pragma unroll
  for (int i = 0; i < TL; ++i) gWL[i] = zero4;
  gbL = zero4;

  double* part = a.part + (((int64_t)p * gridDim.x + blockIdx.x) * kWaves + wave) * a.npart;
  bool first = true;
  int since = 0;
  auto flush = [&]() {
    if (H2P) {
#pragma unroll
      for (int mb = 0; mb < T1; ++mb)
#pragma unroll
        for (int nb = 0; nb < T2; ++nb)
          flush_block(gWm[mb][nb], part + off_dwm(H1P) + 16 * mb * H2P + 16 * nb, H2P, q, c, first);
#pragma unroll
      for (int nb = 0; nb < T2; ++nb) flush_colsum(gbm[nb], part + off_dbm(H1P, H2P) + 16 * nb, q, c, first);
    }
#pragma unroll
    for (int mb = 0; mb < TL; ++mb) flush_block(gWL[mb], part + off_dwl(H1P, H2P) + 16 * mb * 16, 16, q, c, first);
    flush_colsum(gbL, part + off_dbl(H1P, H2P), q, c, first);
    first = false;
  };

  const int64_t ntiles = (a.N + 15) / 16;
  const int64_t tstride = (int64_t)gridDim.x * kWaves;
  for (int64_t t = (int64_t)blockIdx.x * kWaves + wave; t < ntiles; t += tstride) {
    const int64_t r0 = t * 16;

    // ---- first layer: 16 / RS steps of RS rows
    for (int s = 0; s < 16 / RS; ++s) {
      const int tr = s * RS + slot;
      const int64_t row = r0 + tr;
      const bool live = row < a.N && a.W[row * a.ldw + p] != 0.f;
      const int64_t a0 = live ? a.row_ptr[row] : 0;
      const int nrow = live ? (int)(a.row_ptr[row + 1] - a0) : 0;
      int nmax = nrow;                             // the longest row of the wave's slots
      if (RS >= 2) nmax = max(nmax, __shfl_xor(nmax, 32, 64));
      if (RS >= 4) nmax = max(nmax, __shfl_xor(nmax, 16, 64));
      float acc = 0.f;
      for (int base = 0; base < nmax; base += H1P) {
        const bool have = base + j < nrow;
        const int my_i = have ? a.col[a0 + base + j] : 0;
        const float my_v = have ? a.val[a0 + base + j] : 0.f;
        const int n = min(H1P, nmax - base);       // wave-uniform
        for (int u = 0; u < n; u += kU) {
          float xs[kU], vv[kU];
#pragma unroll
          for (int k = 0; k < kU; ++k) {
            const int src = slot * H1P + u + k;    // u + k < H1P: H1P is a multiple of kU
            const int i = __shfl(my_i, src, 64);
            xs[k] = __shfl(my_v, src, 64);
            vv[k] = w1col[(int64_t)i * h1];
          }
#pragma unroll
          for (int k = 0; k < kU; ++k) acc = fmaf(xs[k], base + u + k < nrow ? vv[k] : 0.f, acc);
        }
      }
      float dm = 0.f;
      if (live) {
        const float* xrow = a.Xd + row * (int64_t)a.nd;
        for (int k = 0; k < a.nd; ++k) dm = fmaf(xrow[k], w1d[k * h1], dm);
      }
      A1[tr * P1 + j] = j < h1 ? sigmoidf((acc + dm) + b1j) : 0.f;
    }
    wave_lds_sync();

    // ---- second hidden layer
    if (H2P) {
#pragma unroll
      for (int nb = 0; nb < T2; ++nb) {
        f32x4 z = zero4;
#pragma unroll 4
        for (int kb = 0; kb < H1P / 4; ++kb)
          z = mfma(A1[c * P1 + 4 * kb + q], sWm[(4 * kb + q) * PM + 16 * nb + c], z);
        const float bj = sbm[16 * nb + c];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          A2[(4 * q + r) * P2 + 16 * nb + c] = 16 * nb + c < h2 ? sigmoidf(z[r] + bj) : 0.f;
      }
      wave_lds_sync();
    }

    // ---- output layer, softmax, loss, dZ_L: this lane holds logit [4q + r][c]
    f32x4 lg = zero4;
#pragma unroll 4
    for (int kb = 0; kb < INL / 4; ++kb) lg = mfma(Ap[c * PP + 4 * kb + q], sWL[(4 * kb + q) * 17 + c], lg);
    const bool cv = c < K;
    bool rlive[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = r0 + 4 * q + r;
      const float w = row < a.N ? a.W[row * a.ldw + p] : 0.f;
      const int yc = row < a.N ? (int)a.y[row] : -1;
      rlive[r] = w != 0.f;
      const float z = lg[r] + bLc;
      float mx = cv ? z : -INFINITY;
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
      const float e = cv ? __expf(z - mx) : 0.f;
      float se = e;
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) se += __shfl_xor(se, m, 64);
      const float lse = mx + __logf(se);
      const bool yok = yc >= 0 && yc < K;
      const float zy = __shfl(z, (lane & 48) | (yok ? yc : 0), 64);
      if (c == 0 && rlive[r] && yok) f_acc += (double)(w * (lse - zy));
      if (GRAD) {
        const float pk = e * (1.f / se);
        Dz[(4 * q + r) * kDzPitch + c] = (cv && rlive[r]) ? (w * (pk - (c == yc ? 1.f : 0.f))) / ws : 0.f;
      }
    }

    if (GRAD) {
      wave_lds_sync();
      // dZ1 [4q + r][16 nb + c] leaves from the registers; a row of weight zero leaves as zeros
      auto emit = [&](int nb, int r, float v) {
        const int64_t row = r0 + 4 * q + r;
        const int cc = 16 * nb + c;
        v = rlive[r] ? v : 0.f;
        if (row < a.N && cc < h1) {
          a.dZ1[row * a.ldz + (int64_t)p * h1 + cc] = v;
          db1[nb] += (double)v;
        }
      };
      // ---- output layer: dW += A_prev^T dZ, db += 1^T dZ, dH = dZ W^T
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const float dzb = Dz[(4 * kb + q) * kDzPitch + c];
#pragma unroll
        for (int mb = 0; mb < TL; ++mb) gWL[mb] = mfma(Ap[(4 * kb + q) * PP + 16 * mb + c], dzb, gWL[mb]);
        gbL = mfma(1.f, dzb, gbL);
      }
      float dza[4];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) dza[kb] = Dz[c * kDzPitch + 4 * kb + q];
#pragma unroll
      for (int nb = 0; nb < TL; ++nb) {
        f32x4 dh = zero4;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) dh = mfma(dza[kb], sWL[(16 * nb + c) * 17 + 4 * kb + q], dh);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int at = (4 * q + r) * PP + 16 * nb + c;
          const float av = Ap[at];
          const float dz = dh[r] * (av * (1.f - av));
          if (H2P) Ap[at] = dz;                    // dZ2 over the activation it came from
          else emit(nb, r, dz);
        }
      }
      if (H2P) {
        wave_lds_sync();
        // ---- second hidden layer: A2 now holds dZ2
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
          float a1v[T1];
#pragma unroll
          for (int mb = 0; mb < T1; ++mb) a1v[mb] = A1[(4 * kb + q) * P1 + 16 * mb + c];
#pragma unroll
          for (int nb = 0; nb < (H2P ? T2 : 1); ++nb) {
            const float d2 = A2[(4 * kb + q) * P2 + 16 * nb + c];
#pragma unroll
            for (int mb = 0; mb < T1; ++mb) gWm[mb][nb] = mfma(a1v[mb], d2, gWm[mb][nb]);
            gbm[nb] = mfma(1.f, d2, gbm[nb]);
          }
        }
#pragma unroll
        for (int nb = 0; nb < T1; ++nb) {
          f32x4 dh = zero4;
#pragma unroll 4
          for (int kb = 0; kb < H2P / 4; ++kb)
            dh = mfma(A2[c * P2 + 4 * kb + q], sWm[(16 * nb + c) * PM + 4 * kb + q], dh);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float av = A1[(4 * q + r) * P1 + 16 * nb + c];
            emit(nb, r, dh[r] * (av * (1.f - av)));
          }
        }
      }
      if (++since == kFlushTiles) {
        flush();
        since = 0;
      }
    }
    wave_lds_sync();                               // the next tile overwrites the tiles read here
  }

  // ---- the wave's partial row
  if (GRAD) {
    flush();
#pragma unroll
    for (int nb = 0; nb < T1; ++nb) {
      const double s = fold_q(db1[nb]);
      if (q == 0) part[off_db1() + 16 * nb + c] = s;
    }
  }
  const double fs = ((__shfl(f_acc, 0, 64) + __shfl(f_acc, 16, 64)) + __shfl(f_acc, 32, 64)) + __shfl(f_acc, 48, 64);
  if (lane == 0) part[0] = fs;
}

// out[p][j] = sum over the nslot wave rows of problem p, j < nfold: strand s of 4 adds the rows s, s + 4, ... in
// order, the strands are added in order
__global__ void __launch_bounds__(256) sparse_mlp_fold_kernel(const double* __restrict__ part, int nslot, int npart,
                                                              int nfold, double* __restrict__ out) {
  __shared__ double strand[4][64];
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const int p = blockIdx.y;
  double acc = 0.0;
  if (j < nfold) {
    const double* src = part + (int64_t)p * nslot * npart + j;
    for (int i = s; i < nslot; i += 4) acc += src[(int64_t)i * npart];
  }
  strand[s][lane] = acc;
  __syncthreads();
  if (s == 0 && j < nfold)
    out[(int64_t)p * npart + j] = ((strand[0][lane] + strand[1][lane]) + strand[2][lane]) + strand[3][lane];
}

template <int H1P, int H2P>
int launch(const MlpArgs& a, int P, int grad, int nblk, double* out, hipStream_t stream) {
  const dim3 grid((unsigned)nblk, (unsigned)P);
  if (grad)
    hipLaunchKernelGGL((sparse_mlp_kernel<H1P, H2P, true>), grid, dim3(64 * kWaves), 0, stream, a);
  else
    hipLaunchKernelGGL((sparse_mlp_kernel<H1P, H2P, false>), grid, dim3(64 * kWaves), 0, stream, a);
  const int nfold = grad ? a.npart : 1;
  hipLaunchKernelGGL(sparse_mlp_fold_kernel, dim3((unsigned)((nfold + 63) / 64), (unsigned)P), dim3(256), 0, stream,
                     a.part, nblk * kWaves, a.npart, nfold, out);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int tmog_hip_sparse_mlp_nd_max() { return kNdMax; }

int tmog_hip_sparse_mlp_pad(int width) { return width > 64 ? -1 : pad_width(width); }

int tmog_hip_sparse_mlp_npart(int h1, int h2) { return n_part(pad_width(h1), pad_width(h2)); }

int tmog_hip_sparse_mlp_pass(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N,
                             const float* W1s, int ds, const float* Xd, int nd, const float* W1d, const float* b1,
                             const float* Wm, const float* bm, const float* WL, const float* bL, const float* y,
                             const float* W, int ldw, const float* wsum, int P, int h1, int h2, int K, int grad,
                             float* dZ1, int64_t ldz, double* part, int nblk, double* out, hipStream_t stream) {
  if (P <= 0 || P > 65535 || nblk <= 0 || N < 0 || h1 < 1 || h1 > 64 || h2 < 0 || h2 > 64 || K < 2 || K > 16) return -2;
  if (nd < 0 || nd > kNdMax || (nd > 0 && (Xd == nullptr || W1d == nullptr))) return -2;
  if (h2 > 0 && (Wm == nullptr || bm == nullptr)) return -2;
  if (grad && (dZ1 == nullptr || ldz < (int64_t)P * h1)) return -2;
  const int h1p = pad_width(h1), h2p = pad_width(h2);
  MlpArgs a{row_ptr, col, val, N, W1s, ds, Xd, nd, W1d, b1, Wm, bm, WL, bL, y, W, ldw, wsum, h1, h2, K, dZ1, ldz, part,
            n_part(h1p, h2p)};
#define TM_MLP(A, B) \
  if (h1p == A && h2p == B) return launch<A, B>(a, P, grad, nblk, out, stream)
  TM_MLP(16, 0); TM_MLP(32, 0); TM_MLP(64, 0);
  TM_MLP(16, 16); TM_MLP(32, 16); TM_MLP(64, 16);
  TM_MLP(16, 32); TM_MLP(32, 32); TM_MLP(64, 32);
  TM_MLP(16, 64); TM_MLP(32, 64); TM_MLP(64, 64);
#undef TM_MLP
  return -2;
}

}  // extern "C"
