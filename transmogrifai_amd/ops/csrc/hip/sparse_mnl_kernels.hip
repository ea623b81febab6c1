// Fused multinomial (softmax) objective over the sparse design for OpLogisticRegression (CDNA4, gfx950).
//
// Multinomial logistic regression on a wide, mostly-zero matrix keeps the matrix as ops/linear.py SparseDesign: a CSR
// of the sparse columns and a small dense block Xd [N][nd]. One launch of sparse_mnl_kernel evaluates P problems of K
// classes on it -- the contract of softmax_epilogue_kernel + colsum_kernel (sparse_kernels.hip) without their
// [N][P*K] margin array and [N][P] loss array: with m[i][p][k] = (X v_{p,k})_i + b_{p,k} (the fp32 product plus the
// bias, rounded once),  f_p = sum_i w_ip (lse - m_y),  rsum_{p,k} = sum_i R[i][p][k]  in fp64 and, with grad,
// R[i][p*K + k] = w_ip (softmax_k - [k == y_i]) in fp32 for SparseDesign.tmm. A label outside [0, K) gives loss 0 and
// no one-hot term. A value pass writes nothing per row.
//
//   lanes     The softmax couples the K class columns of a problem, so a lane is (row slot) x (problem) x (padded
//             class): KP = K rounded up to 4, 8 or 16, PW = SW / KP problems side by side in a slot of SW = 16, 32 or
//             64 lanes (the smallest that holds min(P, 64 / KP) problems), RS = 64 / SW rows a wave at once; one
//             problem of 3 classes runs four rows a wave. Lanes k >= K carry a margin of -inf: they add exp(-inf) = 0
//             to the sum and are never stored. The class reductions (max, sum of exponentials, pick of m_y) are
//             cross-lane moves inside the aligned group of KP lanes: no LDS, no barrier. The exponentials are
//             therefore added as a balanced tree over the group, not in class order.
//   chunks    PW problems are a chunk. A lane carries NC <= 4 chunks (its problem of each), so that a row's (col, val)
//             pairs are loaded and broadcast once for NC * PW problems: 24 problems of 6 classes are three chunks of
//             8 problems x 8 lanes in one workgroup column, 3 x 48 = all 144 columns of a V row gathered per
//             non-zero as csr_spmm_kernel does (one chunk a launch column measured 3.9 ms for the value pass against
//             2.7 ms unfused: three times the pair loads and broadcasts). Further chunks go on blockIdx.y.
//   sparse    As sparse_lr_kernel: the SW lanes of a slot load SW (col, val) pairs of their row into a register
//             batch; the pairs are broadcast from it in groups of kU, every group's gathers of Vs[col][p*K + k]
//             issued before its FMAs. The loop bounds are the longest row of the wave's slots; past its own end a
//             row's pairs are (column 0, 0.f) and the loaded value is replaced by 0.f before the FMA, so a V row that
//             is not finite reaches only the rows that hold a non-zero in its column. FMAs keep the pairs' order.
//   dense     Up to kNdMax = 128 dense columns the kernel holds V_d [nd][NC * SW] in LDS and adds the dense block's
//             part itself: 16-byte loads of the Xd row when nd % 4 == 0 and the rows are 16-byte aligned, dword loads
//             otherwise. NC is chosen with nd * NC <= 128, so V_d is 32 KB at most and four workgroups still share a
//             CU. Above the bound the caller computes Xd Vd with the library GEMM and passes it as the addend madd
//             [N][ldm].
//   weights   Problem p reads column wmap[p] of W. In a value pass a row slot whose problems all weigh 0 skips its
//             gathers: its margins stay finite, its loss and residual are multiplied by 0, and +-0 added to the
//             fp64 sums leaves them bit-identical. A gradient pass never skips (R's zeros carry the residual's sign).
//   sums      f and rsum accumulate in fp64 per lane over a persistent row loop (f on the k = 0 lane of a group). Row
//             slots are folded by cross-lane moves, waves through LDS in wave order, and each workgroup writes one
//             fp64 partial per lane of a slot and chunk; mnl_fold_kernel adds them in one fixed order. No atomics:
//             two launches on the same inputs are bitwise equal.
//
// No matrix instructions: the products are gathers of V rows per non-zero (about 40 a row) plus a handful of dense
// columns against per-lane columns of V -- there is no dense tile to feed an MFMA, and the softmax that follows wants
// the margins in exactly this lane layout.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "hip/tmog_hip_abi.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;      // waves per workgroup
constexpr int kU = 8;          // V row gathers in flight per wave and chunk
constexpr int kNdMax = 128;    // dense columns whose V_d stays in LDS (32 KB at NC * SW = 64)
constexpr int kNcMax = 4;      // chunks per lane
constexpr int kKMax = 16;

inline int padded_classes(int K) { return K <= 4 ? 4 : K <= 8 ? 8 : 16; }
// lanes of a row slot: the smallest of 16 / 32 / 64 that holds min(P, 64 / KP) problems of KP lanes
inline int slot_lanes(int P, int K) {
  const int kp = padded_classes(K);
  const int need = kp * (P < 64 / kp ? P : 64 / kp);
  return need <= 16 ? 16 : need <= 32 ? 32 : 64;
}

struct Args {
  const int64_t* row_ptr;
  const int32_t* col;
  const float* val;
  int64_t N;
  const float* Vs;
  int ldv;
  const float* Xd;
  int nd;
  const float* Vd;
  const float* madd;
  int ldm;
  const float* y;
  const float* W;
  int ldw;
  const int32_t* wmap;
  int P, K;
  const float* bias;
  float* R;
  int ldr;
  double* f_part;
  double* r_part;
};

// The dense block's part of the margins: acc[j] += sum_i Xd[row][i] Vd[i][j][q], i in order (sparse_lr_kernels.hip
// dense_part). VW values per lane and batch: 4 -- one 16-byte load; 1 -- a dword load.
template <int SW, int NC, int VW>
__device__ __forceinline__ void dense_part(const float* __restrict__ xrow, bool row_ok, int nd,
                                           const float* __restrict__ Vd, int slot, int q, float* acc) {
  for (int base = 0; base < nd; base += VW * SW) {
    const int i0 = base + VW * q;
    float xv[VW];
#pragma unroll
    for (int u = 0; u < VW; ++u) xv[u] = 0.f;
    if (row_ok && i0 < nd) {
      if (VW == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xrow + i0);
#pragma unroll
        for (int u = 0; u < VW; ++u) xv[u] = t[u];
      } else {
        xv[0] = xrow[i0];
      }
    }
    const int n = min(VW * SW, nd - base);          // wave-uniform; a multiple of VW
    const float* vi = Vd + base * (NC * SW) + q;
    for (int t = 0; t < n; t += VW) {
#pragma unroll
      for (int u = 0; u < VW; ++u) {
        const float x = __shfl(xv[u], slot * SW + t / VW, 64);
#pragma unroll
        for (int j = 0; j < NC; ++j) acc[j] = fmaf(x, vi[(t + u) * (NC * SW) + j * SW], acc[j]);
      }
    }
  }
}

template <int KP, int SW, int NC, bool GRAD>
__global__ void __launch_bounds__(64 * kWaves) sparse_mnl_kernel(const Args a) {
  constexpr int RS = 64 / SW;                      // row slots per wave
  constexpr int PW = SW / KP;                      // problems per chunk
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  double* sf = reinterpret_cast<double*>(lds_raw);                 // [2][kWaves][SW] wave partials of one chunk
  float* Vd = reinterpret_cast<float*>(sf + 2 * kWaves * SW);      // [nd][NC][SW]
  const int64_t* __restrict__ row_ptr = a.row_ptr;
  const int32_t* __restrict__ col = a.col;
  const float* __restrict__ val = a.val;
  const float* __restrict__ Vs = a.Vs;
  const float* __restrict__ W = a.W;
  float* __restrict__ R = a.R;
  const int64_t N = a.N;
  const int P = a.P, K = a.K, ldv = a.ldv, nd = a.nd;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int slot = lane / SW, q = lane % SW;       // q: the lane's place in its slot
  const int k = q % KP;
  const int nchunk = (P + PW - 1) / PW;
  const int chunk0 = blockIdx.y * NC;              // this workgroup's first chunk
  // a column that exists: loads need no guard. A group past P repeats problem P - 1 and a lane past K class K - 1;
  // the former's results are dropped, the latter's margin becomes -inf
  bool live[NC];
  int c[NC], wc[NC];
  float bc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int p = (chunk0 + j) * PW + q / KP;      // this lane's problem of chunk j
    live[j] = p < P && k < K;
    const int pl = p < P ? p : P - 1;
    c[j] = pl * K + (k < K ? k : K - 1);
    bc[j] = a.bias[c[j]];
    wc[j] = a.wmap[pl];
  }
  const bool dense_in = a.Xd != nullptr && nd > 0;
  const bool dense_vec = (nd & 3) == 0 && (reinterpret_cast<uintptr_t>(a.Xd) & 15) == 0;  // 16-byte aligned rows

  if (dense_in) {
    for (int i = threadIdx.x; i < nd * NC * SW; i += 64 * kWaves) {
      const int id = i / (NC * SW), j = (i / SW) % NC, qi = i % SW;
      const int pi = (chunk0 + j) * PW + qi / KP, ki = qi % KP;
      Vd[i] = (pi < P && ki < K) ? a.Vd[(int64_t)id * ldv + pi * K + ki] : 0.f;
    }
    __syncthreads();
  }
  double f_acc[NC], r_acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) f_acc[j] = r_acc[j] = 0.0;

  const int64_t ngroups = (N + RS - 1) / RS;
  const int64_t gstride = (int64_t)gridDim.x * kWaves;
  for (int64_t g = (int64_t)blockIdx.x * kWaves + wave; g < ngroups; g += gstride) {
    const int64_t row = g * RS + slot;
    const bool row_ok = row < N;
    // the row's scalars ride ahead of the gathers
    float w[NC], acc[NC], dm[NC];
    int any = 0;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      w[j] = row_ok ? W[row * a.ldw + wc[j]] : 0.f;
      dm[j] = (a.madd != nullptr && row_ok) ? a.madd[row * a.ldm + c[j]] : 0.f;
      acc[j] = 0.f;
      any |= live[j] && w[j] != 0.f;
    }
    const int yc = row_ok ? (int)a.y[row] : -1;
    const int64_t b0 = row_ok ? row_ptr[row] : 0;
    int nrow = row_ok ? (int)(row_ptr[row + 1] - b0) : 0;
    if (!GRAD) {                                   // a slot whose problems all weigh 0 here: no gathers
#pragma unroll
      for (int s = 1; s < SW; s <<= 1) any |= __shfl_xor(any, s, 64);
      if (!any) nrow = 0;
    }
    int nmax = nrow;                               // the longest row of the wave's slots
    if (RS >= 2) nmax = max(nmax, __shfl_xor(nmax, 32, 64));
    if (RS >= 4) nmax = max(nmax, __shfl_xor(nmax, 16, 64));

    for (int base = 0; base < nmax; base += SW) {
      const bool have = base + q < nrow;
      const int my_i = have ? col[b0 + base + q] : 0;
      const float my_v = have ? val[b0 + base + q] : 0.f;
      const int n = min(SW, nmax - base);          // wave-uniform
      for (int t = 0; t < n; t += kU) {
        float xs[kU], vv[kU][NC];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int src = slot * SW + t + u;       // t + u < SW: SW is a multiple of kU
          const int i = __shfl(my_i, src, 64);
          xs[u] = __shfl(my_v, src, 64);
          const float* vr = Vs + (int64_t)i * ldv;
#pragma unroll
          for (int j = 0; j < NC; ++j) vv[u][j] = vr[c[j]];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const bool in = base + t + u < nrow;
#pragma unroll
          for (int j = 0; j < NC; ++j) acc[j] = fmaf(xs[u], in ? vv[u][j] : 0.f, acc[j]);
        }
      }
    }
    if (dense_in) {                                // the dense block's part: a sum of its own, or the caller's
      const float* xrow = a.Xd + (row_ok ? row : 0) * (int64_t)nd;
#pragma unroll
      for (int j = 0; j < NC; ++j) dm[j] = 0.f;
      if (dense_vec) dense_part<SW, NC, 4>(xrow, row_ok, nd, Vd, slot, q, dm);
      else dense_part<SW, NC, 1>(xrow, row_ok, nd, Vd, slot, q, dm);
    }

    // the softmax of softmax_epilogue_kernel over the group's KP lanes: max-shift, __expf, __logf, one reciprocal
    const bool y_ok = yc >= 0 && yc < K;
    const int y_lane = (lane & ~(KP - 1)) + (y_ok ? yc : 0);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const float m = k < K ? (acc[j] + dm[j]) + bc[j] : -INFINITY;
      float mx = m;
#pragma unroll
      for (int s = 1; s < KP; s <<= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
      const float e = __expf(m - mx);
      float se = e;
#pragma unroll
      for (int s = 1; s < KP; s <<= 1) se += __shfl_xor(se, s, 64);
      const float lse = mx + __logf(se);
      const float m_y = __shfl(m, y_lane, 64);
      if (row_ok && live[j]) {
        const float inv = 1.f / se;
        const float r = w[j] * (e * inv - (k == yc ? 1.f : 0.f));
        r_acc[j] += (double)r;
        if (k == 0) f_acc[j] = fma((double)(lse - (y_ok ? m_y : lse)), (double)w[j], f_acc[j]);
        if (GRAD) R[row * a.ldr + c[j]] = r;
      }
    }
  }

  // row slots by cross-lane moves, waves through LDS in wave order, a chunk at a time
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    if (RS >= 2) {
      f_acc[j] += __shfl_xor(f_acc[j], 32, 64);
      r_acc[j] += __shfl_xor(r_acc[j], 32, 64);
    }
    if (RS >= 4) {
      f_acc[j] += __shfl_xor(f_acc[j], 16, 64);
      r_acc[j] += __shfl_xor(r_acc[j], 16, 64);
    }
    if (slot == 0) {
      sf[wave * SW + q] = f_acc[j];
      sf[(kWaves + wave) * SW + q] = r_acc[j];
    }
    __syncthreads();
    if (threadIdx.x < SW && chunk0 + j < nchunk) {
      double fs = 0.0, rs = 0.0;
      for (int wv = 0; wv < kWaves; ++wv) {
        fs += sf[wv * SW + threadIdx.x];
        rs += sf[(kWaves + wv) * SW + threadIdx.x];
      }
      const int64_t o = ((int64_t)blockIdx.x * nchunk + chunk0 + j) * SW + threadIdx.x;
      a.f_part[o] = fs;
      a.r_part[o] = rs;
    }
    __syncthreads();
  }
}

// f[p] = sum_b f_part[b][lane of (p, 0)], rsum[p*K + k] = sum_b r_part[b][lane of (p, k)] in one fixed order: a wave
// per output, lane t adds the blocks t, t + 64, ... in order, then the 64 lane sums are added in lane order
// (sparse_lr_kernels.hip fold_partials_kernel). A block's partials are [chunk][SW]; out [P + P*K]: f, then rsum.
__global__ void __launch_bounds__(64) mnl_fold_kernel(const double* __restrict__ f_part,
                                                      const double* __restrict__ r_part, int nblk, int width, int P,
                                                      int K, int kp, int sw, double* __restrict__ out) {
  __shared__ double lane_sum[64];
  const int i = blockIdx.x;                        // P + P*K outputs
  const int pw = sw / kp;
  const int p = i < P ? i : (i - P) / K, k = i < P ? 0 : (i - P) % K;
  const double* part = (i < P ? f_part : r_part) + (p / pw) * sw + (p % pw) * kp + k;
  double acc = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) acc += part[(int64_t)b * width];
  lane_sum[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int t = 0; t < 64; ++t) s += lane_sum[t];
    out[i] = s;
  }
}

template <int KP, int SW, int NC>
int launch(const Args& a, int grad, int nblk, double* out, hipStream_t stream) {
  constexpr int PW = SW / KP;
  const int nchunk = (a.P + PW - 1) / PW;
  const dim3 grid((unsigned)nblk, (unsigned)((nchunk + NC - 1) / NC));
  const size_t lds = 2 * kWaves * SW * sizeof(double) + (a.Xd ? (size_t)a.nd * NC * SW * sizeof(float) : 0);
  if (grad) hipLaunchKernelGGL((sparse_mnl_kernel<KP, SW, NC, true>), grid, dim3(64 * kWaves), lds, stream, a);
  else hipLaunchKernelGGL((sparse_mnl_kernel<KP, SW, NC, false>), grid, dim3(64 * kWaves), lds, stream, a);
  hipLaunchKernelGGL(mnl_fold_kernel, dim3((unsigned)(a.P + a.P * a.K)), dim3(64), 0, stream, a.f_part, a.r_part, nblk,
                     nchunk * SW, a.P, a.K, KP, SW, out);
  return (int)hipGetLastError();
}

template <int KP>
int launch_kp(const Args& a, int grad, int nblk, double* out, hipStream_t stream) {
  const int sw = slot_lanes(a.P, a.K);
  if (sw == 16) return launch<KP, 16, 1>(a, grad, nblk, out, stream);      // P problems fit one chunk below 64 lanes
  if (sw == 32) return launch<KP, 32, 1>(a, grad, nblk, out, stream);
  // chunks per lane: as many as V_d leaves room for, spread evenly over the workgroup columns
  const int nchunk = (a.P + 64 / KP - 1) / (64 / KP);
  const int cap = (a.Xd != nullptr && a.nd > 0) ? max(1, min(kNcMax, kNdMax / a.nd)) : kNcMax;
  const int gy = (nchunk + cap - 1) / cap;
  const int nc = (nchunk + gy - 1) / gy;
  if (nc == 1) return launch<KP, 64, 1>(a, grad, nblk, out, stream);
  if (nc == 2) return launch<KP, 64, 2>(a, grad, nblk, out, stream);
  if (nc == 3) return launch<KP, 64, 3>(a, grad, nblk, out, stream);
  return launch<KP, 64, 4>(a, grad, nblk, out, stream);
}

}  // namespace

extern "C" {

int tmog_hip_sparse_mnl_nd_max() { return kNdMax; }

int tmog_hip_sparse_mnl_chunk(int P, int K) {
  if (P <= 0 || K < 2 || K > kKMax) return 0;
  return slot_lanes(P, K) / padded_classes(K);
}

int tmog_hip_sparse_mnl_rows(int P, int K) {
  if (P <= 0 || K < 2 || K > kKMax) return 0;
  return 64 / slot_lanes(P, K);
}

int tmog_hip_sparse_mnl_objective(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N,
                                  const float* Vs, int ldv, const float* Xd, int nd, const float* Vd,
                                  const float* madd, int ldm, const float* y, const float* W, int ldw,
                                  const int32_t* wmap, int P, int K, const float* bias, int grad, float* R, int ldr,
                                  double* f_part, double* r_part, int nblk, double* out, hipStream_t stream) {
  if (P <= 0 || K < 2 || K > kKMax || nblk <= 0 || N < 0) return -2;
  if (Xd != nullptr && (nd < 0 || nd > kNdMax || Vd == nullptr)) return -2;
  if (grad && R == nullptr) return -2;
  const Args a{row_ptr, col, val, N, Vs, ldv, Xd, nd, Vd, madd, ldm, y, W, ldw, wmap, P, K, bias, R, ldr, f_part, r_part};
  const int kp = padded_classes(K);
  if (kp == 4) return launch_kp<4>(a, grad, nblk, out, stream);
  if (kp == 8) return launch_kp<8>(a, grad, nblk, out, stream);
  return launch_kp<16>(a, grad, nblk, out, stream);
}

}  // extern "C"
